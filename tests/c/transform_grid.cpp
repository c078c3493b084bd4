// Driver for the entry rule of a transform batch's grid (epipolarconsistency_amd/csrc/ecc_transform_grid.h), CPU only; its own
// main, so it can also be built with -fsanitize=address,undefined as a stand-alone program.
//   (a) entry(q, k, K) is the inverse of transform_list_kernel's statement q = e / K, k = e - q K, and covers [0, count K) once;
//   (b) the segmented sum of sum_weighted_transforms_kernel, emulated thread by thread with this file's own loops -- slices, thread
//       t's float4 kk = lo + t, lo + t + 1024, ... gathered K floats apart by gather4(), the tail by value(), 1024 lane accumulators,
//       the shuffle-down tree, wave sums and slice sums in order, the slice sums added to 0.0 -- gives the bits of
//       ecc_sum::sum_on_host over the TRANSPOSED column (the transform's values side by side), for every transform of the grid:
//       count in {1, 6, 506, 529, 2 211, 4 160, 32 942} x K in {1, 5, 9} -- a tail only, one float4 and a tail of 2, fewer and more
//       float4 than threads, a tail of 3, whole float4s, sixteen slices.  The grid's column has exactly count K floats (a vector of
//       that size: a gather past the end is the sanitizer's to find).
// Built by tests/test_weighted_transforms_abi.py with -Wall -Werror.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../epipolarconsistency_amd/csrc/ecc_sum_order.h"
#include "../../epipolarconsistency_amd/csrc/ecc_transform_grid.h"

namespace {

int failures = 0;
void check(bool ok, const char* what, long long count, int K, int k)
{
    if (ok) return;
    if (++failures <= 20) std::printf("FAIL %s: count=%lld K=%d k=%d\n", what, count, K, k);
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// Workgroups (slice = 0 .. slices - 1, transform k) of the segmented sum, thread by thread, and the finish.
double emulate(const std::vector<float>& col, long long count, int K, int k, int slices)
{
    const int T = ecc_sum::THREADS;
    const long long n4 = count / 4;
    double tot = 0.0;
    for (int slice = 0; slice < slices; ++slice) {
        long long lo, hi;
        ecc_sum::slice_bounds(n4, slices, slice, &lo, &hi);
        std::vector<double> acc(4 * (size_t)T, 0.0);
        for (int t = 0; t < T; ++t)
            for (long long kk = lo + t; kk < hi; kk += T) {
                float f[4];
                ecc_transform_grid::gather4(col.data(), kk, k, K, f);
                for (int q = 0; q < 4; ++q) acc[4 * (size_t)t + q] += (double)f[q];
            }
        float tail[4] = {0.f, 0.f, 0.f, 0.f};
        if (slice == slices - 1)
            for (int c = 0; c < 4; ++c) tail[c] = 4 * n4 + c < count ? ecc_transform_grid::value(col.data(), 4 * n4 + c, k, K) : 0.f;
        double part = 0.0;
        for (int w = 0; w < T / 64; ++w) {
            double lane[64];
            for (int l = 0; l < 64; ++l) {
                const size_t t = 64 * (size_t)w + l;
                lane[l] = (acc[4 * t] + acc[4 * t + 1]) + (acc[4 * t + 2] + acc[4 * t + 3]);
                if (slice == slices - 1 && t == 0)
                    for (long long q = 4 * n4; q < count; ++q) lane[l] += (double)tail[q - 4 * n4];
            }
            for (int off = 32; off > 0; off >>= 1)
                for (int l = 0; l < off; ++l) lane[l] += lane[l + off];
            part += lane[0];
        }
        tot += part;  // (one slice: 0.0 + part)
    }
    return tot;
}

void check_grid(long long count, int K, std::mt19937& rng)
{
    // (a) the entry rule against the list kernel's statement
    std::vector<char> seen((size_t)(count * K), 0);
    for (long long q = 0; q < count; ++q)
        for (int k = 0; k < K; ++k) {
            const long long e = ecc_transform_grid::entry(q, k, K);
            check(e >= 0 && e < count * K, "entry out of range", count, K, k);
            if (e < 0 || e >= count * K) continue;
            check(e / K == q && e - (e / K) * K == k, "entry is not the inverse of q = e / K, k = e - q K", count, K, k);
            check(!seen[(size_t)e], "entry hit twice", count, K, k);
            seen[(size_t)e] = 1;
        }
    // (b) the sums
    std::uniform_real_distribution<float> mant(0.5f, 1.0f);
    std::uniform_int_distribution<int> expo(-20, 20), sign(0, 1);
    std::vector<float> col((size_t)(count * K));
    for (auto& v : col) v = std::ldexp(mant(rng), expo(rng)) * (sign(rng) ? 1.f : -1.f);
    const int slices = ecc_sum::slices(count, true);
    double first = 0.0;
    bool differ = K == 1;
    for (int k = 0; k < K; ++k) {
        std::vector<float> side_by_side((size_t)count);
        for (long long q = 0; q < count; ++q) side_by_side[(size_t)q] = col[(size_t)(q * K + k)];
        for (int s : {1, slices}) {
            const double want = ecc_sum::sum_on_host(side_by_side.data(), count, s);
            check(same_bits(want, emulate(col, count, K, k, s)), s == 1 ? "strided sum, one slice" : "strided sum, sixteen slices", count, K, k);
        }
        const double mine = emulate(col, count, K, k, slices);
        if (k == 0) first = mine;
        else differ = differ || !same_bits(mine, first);
    }
    check(differ, "every transform of the grid has the same sum: the stride changed nothing", count, K, -1);
}

}  // namespace

int main()
{
    std::mt19937 rng(20240923u);
    const long long counts[] = {1, 6, 506, 529, 2211, 4160, 32942};
    const int Ks[] = {1, 5, 9};
    int grids = 0;
    for (long long count : counts)
        for (int K : Ks) {
            check_grid(count, K, rng);
            ++grids;
        }
    static_assert(ecc_sum::slices(32942, true) == ecc_sum::SLICES && ecc_sum::slices(4160, true) == 1, "the counts reach both forms");
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok: %d grids, every transform's two forms summed\n", grids);
    return 0;
}
