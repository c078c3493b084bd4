// ecc_extremum_tile.h -- a separable running extremum over a 2-D float array with clamped edges, one tile at a time (host and device).
//
// out(r, c) = extremum of f over the (2 R + 1)^2 square around (r, c), indices clamped to the array: numpy pad(mode="edge") followed
// by the window.  Two users (line_weights_kernel.hip): the dilation of a flagged-pixel image (maximum, f = the image) and the guard
// minimum of the line weights (minimum, f = clip(1 - L / zero_at_px, 0, 1) of a length intermediate, applied as the tile is loaded).
//
// An axis of the array has n elements.  The OUTPUT of an axis may be longer than the array: `border` replicated positions on either
// side (the border rows and columns of ecc_layout.h: output -1 is output 0, output n is output n - 1), then zeros up to `pad_end` (the
// pitch padding of a slab).  So the outputs of an axis are the coordinates [-border, pad_end), cut into tiles of T from -border.
//
// One tile, three phases with a barrier between them (a workgroup's threads, or a host loop over tid):
//   load      LDS position j of an axis holds element clamp(origin - halo + j), halo = R + border: T + 2 halo positions per axis;
//   row_pass  for every LDS row and every output column k: the extremum over the 2 R + 1 positions around centre(k) of that row;
//   col_pass  for every output: the extremum over the 2 R + 1 rows around centre(r) of the row pass's column, ONE store.
// centre(k) is the LDS position of the CLAMPED output coordinate: the window of a border output is the window of the element it
// replicates, not a window around the position outside the array (which would miss one element on the far side).  The clamp moves a
// centre by at most `border` positions, which is why the halo is R + border.
//
// Readers: line_weights_kernel.hip and tests/c/extremum_tile.cpp, which walks the same three functions on the host.
#ifndef ECC_EXTREMUM_TILE_H
#define ECC_EXTREMUM_TILE_H

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ECC_EXTREMUM_HD __host__ __device__ __forceinline__
#else
#define ECC_EXTREMUM_HD inline
#endif

namespace ecc_extremum {

constexpr int TILE_ROWS = 16;  // outputs of a tile along the slow axis
constexpr int TILE_COLS = 64;  // ... along the fast axis: one wave reads and writes 256 contiguous bytes
constexpr int THREADS = 256;   // four outputs per thread
constexpr int DILATE_MAX = 16;  // cap of dilate_px (ecc_preprocess' half kernel width)
constexpr int GUARD_MAX = 8;    // cap of guard_bins

// Floats of the two LDS arrays of a tile for radii up to r_max: the loaded tile, then the row pass's result.
constexpr int lds_in_floats(int r_max, int border) { return (TILE_ROWS + 2 * (r_max + border)) * (TILE_COLS + 2 * (r_max + border)); }
constexpr int lds_tmp_floats(int r_max, int border) { return (TILE_ROWS + 2 * (r_max + border)) * TILE_COLS; }

struct Max {
    static ECC_EXTREMUM_HD float combine(float a, float b) { return b > a ? b : a; }
};
struct Min {
    static ECC_EXTREMUM_HD float combine(float a, float b) { return b < a ? b : a; }
};

// Step 3 of the line weights: one IEEE binary32 division, one subtraction, the clip.
ECC_EXTREMUM_HD float clip_weight(float length, float zero_at_px)
{
    const float q = length / zero_at_px;
    const float w = 1.0f - q;
    return w < 0.0f ? 0.0f : (w > 1.0f ? 1.0f : w);
}

struct Axis {
    int n;        // elements of the array
    int border;   // replicated outputs on either side
    int pad_end;  // outputs [n + border, pad_end) are zeros; n + border where there are none
    int radius;   // R
    int origin;   // output coordinate of the tile's first output: tile * T - border

    ECC_EXTREMUM_HD int halo() const { return radius + border; }
    ECC_EXTREMUM_HD int extent(int T) const { return T + 2 * halo(); }
    static ECC_EXTREMUM_HD int clamp(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }
    // the element LDS position j holds
    ECC_EXTREMUM_HD int source(int j) const { return clamp(origin - halo() + j, n); }
    // output k of the tile is an extremum (an element or a replicated border position)
    ECC_EXTREMUM_HD bool inside(int k) const { return origin + k < n + border; }
    // ... or a zero of the padding
    ECC_EXTREMUM_HD bool padding(int k) const { return origin + k >= n + border && origin + k < pad_end; }
    // LDS position of the centre of output k's window (inside(k) only); the window is centre - R .. centre + R
    ECC_EXTREMUM_HD int centre(int k) const { return clamp(origin + k, n) - (origin - halo()); }
    static ECC_EXTREMUM_HD int tiles(int n, int border, int pad_end, int T) { return ((pad_end > n + border ? pad_end : n + border) + border + T - 1) / T; }
};

struct Tile {
    Axis rows, cols;
};

ECC_EXTREMUM_HD Axis make_axis(int n, int border, int pad_end, int radius, int tile, int T)
{
    Axis a;
    a.n = n;
    a.border = border;
    a.pad_end = pad_end > n + border ? pad_end : n + border;
    a.radius = radius;
    a.origin = tile * T - border;
    return a;
}

// load(r, c): the value of element (r, c), 0 <= r < rows.n, 0 <= c < cols.n.
template <class Load>
ECC_EXTREMUM_HD void load_tile(const Tile& t, int tid, int n_threads, float* in, Load load)
{
    const int h = t.rows.extent(TILE_ROWS), w = t.cols.extent(TILE_COLS);
    for (int i = tid; i < h * w; i += n_threads) {
        const int j = i / w, c = i - j * w;
        in[i] = load(t.rows.source(j), t.cols.source(c));
    }
}

template <class Op>
ECC_EXTREMUM_HD void row_pass(const Tile& t, int tid, int n_threads, const float* in, float* tmp)
{
    const int h = t.rows.extent(TILE_ROWS), w = t.cols.extent(TILE_COLS), R = t.cols.radius;
    for (int i = tid; i < h * TILE_COLS; i += n_threads) {
        const int j = i / TILE_COLS, k = i - j * TILE_COLS;
        if (!t.cols.inside(k)) continue;
        const float* p = in + j * w + t.cols.centre(k) - R;
        float v = p[0];
        for (int d = 1; d <= 2 * R; ++d) v = Op::combine(v, p[d]);
        tmp[i] = v;
    }
}

// store(r, c, value): output coordinates, -border <= r < rows.n + border, -border <= c < cols.pad_end; called once per output.
template <class Op, class Store>
ECC_EXTREMUM_HD void col_pass(const Tile& t, int tid, int n_threads, const float* tmp, Store store)
{
    const int R = t.rows.radius;
    for (int i = tid; i < TILE_ROWS * TILE_COLS; i += n_threads) {
        const int r = i / TILE_COLS, k = i - r * TILE_COLS;
        if (!t.rows.inside(r)) continue;
        if (t.cols.padding(k)) store(t.rows.origin + r, t.cols.origin + k, 0.0f);
        if (!t.cols.inside(k)) continue;
        const float* p = tmp + (t.rows.centre(r) - R) * TILE_COLS + k;
        float v = p[0];
        for (int d = 1; d <= 2 * R; ++d) v = Op::combine(v, p[d * TILE_COLS]);
        store(t.rows.origin + r, t.cols.origin + k, v);
    }
}

}  // namespace ecc_extremum

#endif
