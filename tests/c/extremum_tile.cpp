// csrc/ecc_extremum_tile.h on the host (g++, built and run by tests/test_extremum_tile.py): the tile, halo and clamp arithmetic of
// line_weights_kernel.hip walked tile by tile and "thread" by "thread" exactly as the kernels walk it -- load, barrier, row pass,
// barrier, column pass -- against a brute-force window loop, bit for bit:
//   the maximum form over an image (no border, no padding), as dilate_max_kernel uses it;
//   the clip + minimum form over a slab of the private layout (one replicated border position per side, zeros in the pitch padding),
//     as clip_min_kernel uses it: every float of the destination slab is stored exactly once, and of the source slab only the
//     elements are read.
// With a file argument (written by the wrapper from numpy): records of lengths and line_weights_from_lengths' result for them; the
// clip + minimum form must reproduce those bits.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "ecc_extremum_tile.h"

using namespace ecc_extremum;

namespace {

int pitch_of(int n_t) { return ((n_t + 2) + 31) / 32 * 32; }  // ecc_layout_pitch

bool same_bits(float a, float b)
{
    uint32_t x, y;
    std::memcpy(&x, &a, 4);
    std::memcpy(&y, &b, 4);
    return x == y;
}

int clampi(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// deterministic values without a library generator: a mix of zeros, values in [0, 3) and a few large ones
float value_at(unsigned k, unsigned seed)
{
    unsigned x = (k + 1) * 2654435761u ^ (seed * 40503u + 12345u);
    x ^= x >> 13;
    x *= 2246822519u;
    x ^= x >> 16;
    if (x % 5 < 2) return 0.0f;
    return (float)(x % 3001) / 1000.0f;
}

// one tile through the three phases, threads one after the other with the "barriers" between the loops
template <class Op, class Load, class Store>
void walk_tile(const Tile& t, std::vector<float>& in, std::vector<float>& tmp, Load load, Store store)
{
    const float nan = std::numeric_limits<float>::quiet_NaN();
    std::fill(in.begin(), in.end(), nan);
    std::fill(tmp.begin(), tmp.end(), nan);
    for (int tid = 0; tid < THREADS; ++tid) load_tile(t, tid, THREADS, in.data(), load);
    for (int tid = 0; tid < THREADS; ++tid) row_pass<Op>(t, tid, THREADS, in.data(), tmp.data());
    for (int tid = 0; tid < THREADS; ++tid) col_pass<Op>(t, tid, THREADS, tmp.data(), store);
}

// the maximum form: h x w image -> h x w image
int check_max(int h, int w, int R, unsigned seed)
{
    std::vector<float> f((size_t)h * w), got((size_t)h * w, -7.0f);
    std::vector<int> stores((size_t)h * w, 0);
    for (size_t k = 0; k < f.size(); ++k) f[k] = value_at((unsigned)k, seed) - 1.0f;  // negative values too
    std::vector<float> in(lds_in_floats(DILATE_MAX, 0)), tmp(lds_tmp_floats(DILATE_MAX, 0));
    int bad = 0;
    for (int ty = 0; ty < Axis::tiles(h, 0, 0, TILE_ROWS); ++ty)
        for (int tx = 0; tx < Axis::tiles(w, 0, 0, TILE_COLS); ++tx) {
            Tile t;
            t.rows = make_axis(h, 0, 0, R, ty, TILE_ROWS);
            t.cols = make_axis(w, 0, 0, R, tx, TILE_COLS);
            if (t.rows.extent(TILE_ROWS) * t.cols.extent(TILE_COLS) > (int)in.size()) return 1000;
            walk_tile<Max>(
                t, in, tmp,
                [&](int r, int c) {
                    if (r < 0 || r >= h || c < 0 || c >= w) ++bad;
                    return f[(size_t)clampi(r, h) * w + clampi(c, w)];
                },
                [&](int r, int c, float v) {
                    if (r < 0 || r >= h || c < 0 || c >= w) {
                        ++bad;
                        return;
                    }
                    got[(size_t)r * w + c] = v;
                    ++stores[(size_t)r * w + c];
                });
        }
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
            float want = f[(size_t)r * w + c];
            for (int dr = -R; dr <= R; ++dr)
                for (int dc = -R; dc <= R; ++dc) {
                    const float x = f[(size_t)clampi(r + dr, h) * w + clampi(c + dc, w)];
                    if (x > want) want = x;
                }
            if (!same_bits(got[(size_t)r * w + c], want) || stores[(size_t)r * w + c] != 1) ++bad;
        }
    return bad;
}

// the clip + minimum form on a slab: element (r, c) of `lengths` (n_rows x n_cols, read through at()) -> a complete slab.
// want: the expected elements (n_rows x n_cols, row-major) or null for the brute-force loop.
int check_min(int n_rows, int n_cols, int R, float zero_at, const std::vector<float>& lengths, const float* want_elements)
{
    const int pitch = pitch_of(n_cols), rows = n_rows + 2;
    const float poison = 1e30f;  // in the source's border and padding: read, it would clip to 0 and lower a minimum
    std::vector<float> src((size_t)rows * pitch, poison), got((size_t)rows * pitch, -7.0f);
    std::vector<int> stores((size_t)rows * pitch, 0);
    for (int r = 0; r < n_rows; ++r)
        for (int c = 0; c < n_cols; ++c) src[(size_t)(r + 1) * pitch + c + 1] = lengths[(size_t)r * n_cols + c];
    std::vector<float> in(lds_in_floats(GUARD_MAX, 1)), tmp(lds_tmp_floats(GUARD_MAX, 1));
    int bad = 0;
    for (int ty = 0; ty < Axis::tiles(n_rows, 1, 0, TILE_ROWS); ++ty)
        for (int tx = 0; tx < Axis::tiles(n_cols, 1, pitch - 1, TILE_COLS); ++tx) {
            Tile t;
            t.rows = make_axis(n_rows, 1, 0, R, ty, TILE_ROWS);
            t.cols = make_axis(n_cols, 1, pitch - 1, R, tx, TILE_COLS);
            if (t.rows.extent(TILE_ROWS) * t.cols.extent(TILE_COLS) > (int)in.size()) return 1000;
            walk_tile<Min>(
                t, in, tmp,
                [&](int r, int c) {
                    if (r < 0 || r >= n_rows || c < 0 || c >= n_cols) {
                        ++bad;
                        return 0.0f;
                    }
                    return clip_weight(src[(size_t)(r + 1) * pitch + (c + 1)], zero_at);
                },
                [&](int r, int c, float v) {
                    if (r < -1 || r > n_rows || c < -1 || c + 1 >= pitch) {
                        ++bad;
                        return;
                    }
                    got[(size_t)(r + 1) * pitch + (c + 1)] = v;
                    ++stores[(size_t)(r + 1) * pitch + (c + 1)];
                });
        }
    std::vector<float> want((size_t)n_rows * n_cols);
    for (int r = 0; r < n_rows; ++r)
        for (int c = 0; c < n_cols; ++c) {
            if (want_elements) {
                want[(size_t)r * n_cols + c] = want_elements[(size_t)r * n_cols + c];
                continue;
            }
            float m = 2.0f;
            for (int dr = -R; dr <= R; ++dr)
                for (int dc = -R; dc <= R; ++dc) {
                    const float L = lengths[(size_t)clampi(r + dr, n_rows) * n_cols + clampi(c + dc, n_cols)];
                    const float q = L / zero_at;
                    float w = 1.0f - q;
                    w = w < 0.0f ? 0.0f : (w > 1.0f ? 1.0f : w);
                    if (w < m) m = w;
                }
            want[(size_t)r * n_cols + c] = m;
        }
    // the whole slab: elements, replicated border, zero padding; every float stored once
    for (int pr = 0; pr < rows; ++pr)
        for (int pc = 0; pc < pitch; ++pc) {
            const float expect = pc >= n_cols + 2 ? 0.0f : want[(size_t)clampi(pr - 1, n_rows) * n_cols + clampi(pc - 1, n_cols)];
            if (!same_bits(got[(size_t)pr * pitch + pc], expect) || stores[(size_t)pr * pitch + pc] != 1) ++bad;
        }
    return bad;
}

int check_min_generated(int n_rows, int n_cols, int R, float zero_at, unsigned seed)
{
    std::vector<float> L((size_t)n_rows * n_cols);
    for (size_t k = 0; k < L.size(); ++k) L[k] = value_at((unsigned)k, seed);
    return check_min(n_rows, n_cols, R, zero_at, L, nullptr);
}

// records: int32 n_t, n_alpha, guard; float zero_at; n_t * n_alpha lengths; n_t * n_alpha weights (both (n_t, n_alpha), alpha fastest)
int check_file(const char* path)
{
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return -1;
    int records = 0, bad = 0;
    for (;;) {
        int32_t head[3];
        float zero_at;
        if (std::fread(head, 4, 3, f) != 3) break;
        if (std::fread(&zero_at, 4, 1, f) != 1) return -1;
        const int n_t = head[0], n_alpha = head[1], g = head[2];
        std::vector<float> L((size_t)n_t * n_alpha), W(L.size()), Ls(L.size()), Ws(L.size());
        if (std::fread(L.data(), 4, L.size(), f) != L.size() || std::fread(W.data(), 4, W.size(), f) != W.size()) return -1;
        // the slab's rows are angle bins, its columns distance bins
        for (int ix = 0; ix < n_alpha; ++ix)
            for (int iy = 0; iy < n_t; ++iy) {
                Ls[(size_t)ix * n_t + iy] = L[(size_t)iy * n_alpha + ix];
                Ws[(size_t)ix * n_t + iy] = W[(size_t)iy * n_alpha + ix];
            }
        const int b = check_min(n_alpha, n_t, g, zero_at, Ls, Ws.data());
        if (b) std::printf("record %d (n_t %d, n_alpha %d, guard %d, zero_at %g): %d mismatches\n", records, n_t, n_alpha, g, zero_at, b);
        bad += b;
        ++records;
    }
    std::fclose(f);
    std::printf("%d records from numpy\n", records);
    return records > 0 ? bad : -1;
}

}  // namespace

int main(int argc, char** argv)
{
    // height x width; for the slab form: angle bins x distance bins (30, 62: no pitch padding beyond the border; 31: 31 floats of it)
    const int sizes[][2] = {{33, 97}, {13, 17}, {1, 1}, {1, 40}, {3, 5}, {TILE_ROWS, TILE_COLS}, {TILE_ROWS + 1, TILE_COLS + 1},
                            {7, 30}, {7, 31}, {5, 62}, {TILE_ROWS - 1, TILE_COLS - 1}, {40, 2}};
    int failures = 0, cases = 0;
    for (const auto& s : sizes) {
        const int max_radii[] = {0, 1, 2, DILATE_MAX};       // DILATE_MAX is larger than most of the arrays
        const int min_radii[] = {0, 1, 2, 5, GUARD_MAX};     // 5 and GUARD_MAX are larger than the 3 x 5 and 1 x 1 arrays
        for (int R : max_radii) {
            const int b = check_max(s[0], s[1], R, 7u + (unsigned)R);
            if (b) std::printf("max %d x %d radius %d: %d mismatches\n", s[0], s[1], R, b);
            failures += b != 0;
            ++cases;
        }
        for (int R : min_radii)
            for (float z : {1.0f, 2.5f}) {
                const int b = check_min_generated(s[0], s[1], R, z, 11u + (unsigned)R);
                if (b) std::printf("clip+min %d x %d radius %d zero_at %g: %d mismatches\n", s[0], s[1], R, z, b);
                failures += b != 0;
                ++cases;
            }
    }
    if (argc > 1) {
        const int b = check_file(argv[1]);
        if (b) std::printf("numpy records: %d\n", b);
        failures += b != 0;
        ++cases;
    }
    std::printf("%d cases, %d failures\n", cases, failures);
    if (!failures) std::printf("extremum tile ok\n");
    return failures ? 1 : 0;
}
