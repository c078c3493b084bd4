// Driver for the S-column segmented sums (epipolarconsistency_amd/csrc/form_sums_kernel.hip), CPU only; its own main, so it is also
// built with -fsanitize=address,undefined as a stand-alone program.  Both kernels are emulated thread by thread with this file's own
// loops, for S = 3 random columns, and every column must have the bits of ecc_sum::sum_on_host:
//   (a) sum_form_poses_kernel: slices, chunks of CHUNK_F4 = ecc_sum::THREADS float4 of EACH base column copied into S stages, the
//       pose's c n entries walked ONCE per chunk -- position() once per entry, the entry's S values put over the S stages, the tail in
//       its own S x 4 slots --, thread t adding float4 t of every stage into that column's four accumulators, which run across the
//       chunks; then per column the combine, the tail by thread 0 of the last slice, the shuffle-down tree, wave sums and slice sums
//       in order.  Against sum_on_host over each SUBSTITUTED column.  Pair counts 1, 3, 36, 2 211 (tail 3), 8 385 (several chunks,
//       tail 1), 32 896 / 33 153 (sixteen slices without and with a tail), 134 940 (a slice longer than a chunk); moved sets of 0, 1
//       and 4 views, a pair of two moved views among them.
//   (b) sum_form_transforms_kernel: thread t's float4 kk = lo + t, lo + t + 1024, ...: the four entries formed once
//       (ecc_transform_grid::entry) and read in each of the S columns; the tail by value().  Against sum_on_host over each TRANSPOSED
//       column, for every transform: count in {1, 6, 529, 2 211, 32 942} x K in {1, 5, 9}.
// Every column is a vector of exactly the needed size: a read past a column's end is the sanitizer's to find.
// Built by tests/test_weighted_robust_batches_abi.py with -Wall -Werror.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../epipolarconsistency_amd/csrc/ecc_pose_scatter.h"
#include "../../epipolarconsistency_amd/csrc/ecc_transform_grid.h"

namespace {

constexpr int S = 3;
constexpr int CHUNK_F4 = ecc_sum::THREADS;  // (form_sums_kernel.hip: 16 KiB per column)
typedef std::vector<std::vector<float>> Columns;

int failures = 0;
void check(bool ok, const char* what, long long count, int a, int b)
{
    if (ok) return;
    if (++failures <= 20) std::printf("FAIL %s: count=%lld %d %d\n", what, count, a, b);
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// The end of a workgroup for one column: lane values -> the slice's sum.  acc: 4 accumulators per thread.
double slice_sum(const std::vector<double>& acc, bool owns_tail, const float* tail, long long n4, long long count)
{
    const int T = ecc_sum::THREADS;
    double part = 0.0;
    for (int w = 0; w < T / 64; ++w) {
        double lane[64];
        for (int l = 0; l < 64; ++l) {
            const size_t t = 64 * (size_t)w + l;
            lane[l] = (acc[4 * t] + acc[4 * t + 1]) + (acc[4 * t + 2] + acc[4 * t + 3]);
            if (owns_tail && t == 0)
                for (long long k = 4 * n4; k < count; ++k) lane[l] += (double)tail[k - 4 * n4];
        }
        for (int off = 32; off > 0; off >>= 1)
            for (int l = 0; l < off; ++l) lane[l] += lane[l + off];
        part += lane[0];
    }
    return part;
}

// (a) the workgroups (slice, pose) of one pose.  vals[col]: entry (u, a) at u * c + a.  out[col]: the pose's sum of column col.
void emulate_pose(const Columns& base, long long count, int slices, int n, const std::vector<int>& M, const Columns& vals, double out[S],
                  long long* positions_evaluated)
{
    const int T = ecc_sum::THREADS, c = (int)M.size();
    const long long n4 = count / 4;
    for (int col = 0; col < S; ++col) out[col] = 0.0;
    for (int slice = 0; slice < slices; ++slice) {
        long long lo, hi;
        ecc_sum::slice_bounds(n4, slices, slice, &lo, &hi);
        const bool owns_tail = slice == slices - 1;
        std::vector<float> stage[S];
        float tail[S][4];
        std::vector<double> acc[S];
        for (int col = 0; col < S; ++col) {
            stage[col].assign(4 * (size_t)CHUNK_F4, 0.f);
            acc[col].assign(4 * (size_t)T, 0.0);
            for (int q = 0; q < 4; ++q) tail[col][q] = owns_tail && 4 * n4 + q < count ? base[col][(size_t)(4 * n4 + q)] : 0.f;
        }
        bool first_chunk = true;
        for (long long c0 = lo; c0 < hi || first_chunk; c0 += CHUNK_F4) {
            const long long ce = std::min(hi, c0 + CHUNK_F4);
            for (int t = 0; t < T; ++t)
                if (c0 + t < ce)
                    for (int col = 0; col < S; ++col)
                        for (int q = 0; q < 4; ++q) stage[col][4 * (size_t)t + q] = base[col][(size_t)(4 * (c0 + t) + q)];
            for (int e = 0; e < c * n; ++e) {  // one walk for the S columns
                const int a = e / n, u = e - a * n;
                const long long ij = ecc_pose_scatter::position(u, a, M.data(), n);
                ++*positions_evaluated;
                if (ij == ecc_pose_scatter::HOLE) continue;
                const bool in_chunk = ij >= 4 * c0 && ij < 4 * ce;
                const bool in_tail = owns_tail && first_chunk && ij >= 4 * n4;
                if (!in_chunk && !in_tail) continue;
                for (int col = 0; col < S; ++col) {
                    const float val = vals[col][(size_t)u * c + a];
                    if (in_chunk) stage[col][(size_t)(ij - 4 * c0)] = val;
                    else tail[col][ij - 4 * n4] = val;
                }
            }
            for (int t = 0; t < T; ++t)
                if (c0 + t < ce)
                    for (int col = 0; col < S; ++col)
                        for (int q = 0; q < 4; ++q) acc[col][4 * (size_t)t + q] += (double)stage[col][4 * (size_t)t + q];
            first_chunk = false;
        }
        for (int col = 0; col < S; ++col) out[col] += slice_sum(acc[col], owns_tail, tail[col], n4, count);
    }
}

float draw(std::mt19937& rng)
{
    std::uniform_real_distribution<float> mant(0.5f, 1.0f);
    std::uniform_int_distribution<int> expo(-20, 20), sign(0, 1);
    return std::ldexp(mant(rng), expo(rng)) * (sign(rng) ? 1.f : -1.f);
}

void check_poses(int n, std::mt19937& rng)
{
    const long long count = (long long)n * (n - 1) / 2;
    Columns base(S, std::vector<float>((size_t)count));
    for (auto& col : base)
        for (auto& v : col) v = draw(rng);
    std::vector<std::vector<int>> sets = {{}, {n - 1}, {n / 2}};
    if (n >= 4) sets.push_back({0, 1, n / 2, n - 1});  // {0, 1}: a pair of two moved views (and more)
    for (const auto& M : sets) {
        const int c = (int)M.size();
        Columns vals(S, std::vector<float>((size_t)n * c)), subst(base);
        for (int col = 0; col < S; ++col) {
            for (auto& v : vals[col]) v = draw(rng);
            for (int a = 0; a < c; ++a)
                for (int u = 0; u < n; ++u) {
                    const long long ij = ecc_pose_scatter::position(u, a, M.data(), n);
                    if (ij != ecc_pose_scatter::HOLE) subst[col][(size_t)ij] = vals[col][(size_t)u * c + a];
                }
        }
        for (int slices : {1, ecc_sum::SLICES}) {
            double got[S];
            long long walked = 0, chunks = 0;
            emulate_pose(base, count, slices, n, M, vals, got, &walked);
            for (int slice = 0; slice < slices; ++slice) {
                long long lo, hi;
                ecc_sum::slice_bounds(count / 4, slices, slice, &lo, &hi);
                chunks += std::max<long long>(1, (hi - lo + CHUNK_F4 - 1) / CHUNK_F4);
            }
            check(walked == chunks * c * n, "position() not once per entry and chunk", count, c, slices);
            for (int col = 0; col < S; ++col) {
                const double want = ecc_sum::sum_on_host(subst[col].data(), count, slices);
                check(same_bits(want, got[col]), slices == 1 ? "pose sum, one slice" : "pose sum, sixteen slices", count, c, col);
                if (c > 0) check(!same_bits(want, ecc_sum::sum_on_host(base[col].data(), count, slices)), "the substitution changed nothing", count, c, col);
            }
            check(!same_bits(got[0], got[1]) && !same_bits(got[1], got[2]), "the columns have the same sum", count, c, slices);
        }
    }
}

// (b) the workgroups (slice, transform k).  cols[col]: a column of the grid, count K floats.
void emulate_transform(const Columns& cols, long long count, int K, int k, int slices, double out[S])
{
    const int T = ecc_sum::THREADS;
    const long long n4 = count / 4;
    for (int col = 0; col < S; ++col) out[col] = 0.0;
    for (int slice = 0; slice < slices; ++slice) {
        long long lo, hi;
        ecc_sum::slice_bounds(n4, slices, slice, &lo, &hi);
        const bool owns_tail = slice == slices - 1;
        std::vector<double> acc[S];
        for (int col = 0; col < S; ++col) acc[col].assign(4 * (size_t)T, 0.0);
        for (int t = 0; t < T; ++t)
            for (long long kk = lo + t; kk < hi; kk += T) {
                long long e[4];  // once for the S columns
                for (int q = 0; q < 4; ++q) e[q] = ecc_transform_grid::entry(4 * kk + q, k, K);
                for (int col = 0; col < S; ++col)
                    for (int q = 0; q < 4; ++q) acc[col][4 * (size_t)t + q] += (double)cols[col][(size_t)e[q]];
            }
        for (int col = 0; col < S; ++col) {
            float tail[4] = {0.f, 0.f, 0.f, 0.f};
            if (owns_tail)
                for (int q = 0; q < 4; ++q) tail[q] = 4 * n4 + q < count ? ecc_transform_grid::value(cols[col].data(), 4 * n4 + q, k, K) : 0.f;
            out[col] += slice_sum(acc[col], owns_tail, tail, n4, count);  // (one slice: 0.0 + part)
        }
    }
}

void check_transforms(long long count, int K, std::mt19937& rng)
{
    Columns cols(S, std::vector<float>((size_t)(count * K)));
    for (auto& col : cols)
        for (auto& v : col) v = draw(rng);
    const int split = ecc_sum::slices(count, true);
    for (int k = 0; k < K; ++k) {
        Columns side_by_side(S, std::vector<float>((size_t)count));
        for (int col = 0; col < S; ++col)
            for (long long q = 0; q < count; ++q) side_by_side[col][(size_t)q] = cols[col][(size_t)(q * K + k)];
        for (int s : {1, split}) {
            double got[S];
            emulate_transform(cols, count, K, k, s, got);
            for (int col = 0; col < S; ++col)
                check(same_bits(ecc_sum::sum_on_host(side_by_side[col].data(), count, s), got[col]),
                      s == 1 ? "transform sum, one slice" : "transform sum, sixteen slices", count, K, 16 * k + col);
            check(!same_bits(got[0], got[1]) && !same_bits(got[1], got[2]), "the columns have the same sum", count, K, k);
        }
    }
}

}  // namespace

int main()
{
    std::mt19937 rng(20250311u);
    const int ns[] = {2, 3, 9, 67, 130, 257, 258, 520};
    for (int n : ns) check_poses(n, rng);
    const long long counts[] = {1, 6, 529, 2211, 32942};
    const int Ks[] = {1, 5, 9};
    int grids = 0;
    for (long long count : counts)
        for (int K : Ks) {
            check_transforms(count, K, rng);
            ++grids;
        }
    static_assert(CHUNK_F4 % ecc_sum::THREADS == 0, "a thread's float4 stay its own across chunks");
    static_assert(ecc_sum::slices(32942, true) == ecc_sum::SLICES && ecc_sum::slices(2211, true) == 1, "the counts reach both forms");
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok: %d pair counts x 3 columns summed per pose, %d grids x 3 columns per transform\n", (int)(sizeof(ns) / sizeof(ns[0])), grids);
    return 0;
}
