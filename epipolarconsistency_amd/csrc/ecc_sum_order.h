// ecc_sum_order.h -- THE order in which the float64 total of `count` pair values is added (ref:
// ...RadonIntermediate.cpp:216-224: the reference's host loop; all weights are 1).
//
// Every promise of "the same bits as set_projections + evaluate_all" (pose batches, the one-launch evaluation, the pose-delta
// mode) is a promise about this order, so it is stated here once and used by sum_pairs_kernel / sum_pairs_split_kernel
// (sum_kernel.hip), sum_poses_kernel / finish_poses_kernel (ecc_poses.hip), sum_weighted_poses_kernel (weighted_poses_kernel.hip),
// sum_form_poses_kernel / sum_form_transforms_kernel (form_sums_kernel.hip) and the host (sum_on_host, ecc_evaluate.hip):
//   * the values are read as float4 k = 0 .. n4 - 1, n4 = count / 4, cut into `slices` contiguous slices of
//     per = ceil(n4 / slices) float4 (slice_bounds); slices = 1 below SPLIT_MIN_COUNT values, else SLICES (slices);
//   * a slice is added by THREADS threads: thread t adds the components x, y, z, w of its float4 k = lo + t, lo + t + THREADS,
//     ... into four accumulators that start at 0.0 (add), then forms (a0 + a1) + (a2 + a3) (combine);
//   * thread 0 of the LAST slice then adds the up to three values past the last float4, in index order (add_tail);
//   * the 64 threads of a wave are combined by the shuffle-down tree, offsets 32, 16, ... 1 (wave_sum: lane 0 has the sum),
//     and the THREADS / 64 wave sums are added to 0.0 in wave order (waves_in_order): the slice's sum;
//   * the slice sums are added to 0.0 in slice order (one slice: 0.0 + its sum, the same number -- the sum kernels skip it).
// IEEE binary64 additions in the same order give the same bits, whoever performs them.  How many loads a kernel keeps in
// flight, or whether it stages values in LDS first, is scheduling and stays with the kernel.
#ifndef ECC_SUM_ORDER_H
#define ECC_SUM_ORDER_H

#include <cstdint>

namespace ecc_sum {

constexpr int THREADS = 1024;                 // threads of a sum workgroup
constexpr int WAVES = THREADS / 64;
constexpr int SLICES = 16;                    // slices (workgroups) of the split form
constexpr long long SPLIT_MIN_COUNT = 32768;  // counts from here on are added in SLICES slices
static_assert(THREADS % 64 == 0, "a sum workgroup is whole waves");

// have_scratch: the caller owns the split form's scratch (ecc_sum_scratch_bytes()); without it every count is one slice.
// (constexpr: for host and device code alike)
constexpr int slices(long long count, bool have_scratch) { return have_scratch && count >= SPLIT_MIN_COUNT ? SLICES : 1; }

// Slice `slice` of `n_slices` covers the float4 [lo, hi) of the n4.
template <class Index>
constexpr void slice_bounds(long long n4, int n_slices, Index slice, long long* lo, long long* hi)
{
    const long long per = (n4 + n_slices - 1) / n_slices;
    *lo = (long long)slice * per;
    *hi = n4 < *lo + per ? n4 : *lo + per;
}

// The total of v[0 .. count) in `n_slices` (1 or SLICES) slices, on the host.
inline double sum_on_host(const float* v, int64_t count, int n_slices)
{
    const long long n4 = count >> 2;
    double tot = 0.0;
    for (int s = 0; s < n_slices; ++s) {
        long long lo, hi;
        slice_bounds(n4, n_slices, s, &lo, &hi);
        double part = 0.0;
        for (int w = 0; w < WAVES; ++w) {
            double a[64];
            for (int l = 0; l < 64; ++l) {
                const int t = 64 * w + l;
                double c[4] = {0.0, 0.0, 0.0, 0.0};
                for (long long k = lo + t; k < hi; k += THREADS)
                    for (int q = 0; q < 4; ++q) c[q] += (double)v[4 * k + q];
                a[l] = (c[0] + c[1]) + (c[2] + c[3]);
                if (s == n_slices - 1 && t == 0)
                    for (long long k = n4 << 2; k < count; ++k) a[l] += (double)v[k];
            }
            for (int off = 32; off > 0; off >>= 1)
                for (int l = 0; l < off; ++l) a[l] += a[l + off];  // what lane 0 of wave_sum's tree ends up with
            part += a[0];
        }
        tot += part;
    }
    return tot;
}

#if defined(__HIPCC__)
struct Acc4 { double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0; };

__device__ __forceinline__ void add(Acc4& a, const float4& v)
{
    a.a0 += (double)v.x;
    a.a1 += (double)v.y;
    a.a2 += (double)v.z;
    a.a3 += (double)v.w;
}

__device__ __forceinline__ double combine(const Acc4& a) { return (a.a0 + a.a1) + (a.a2 + a.a3); }

// By thread 0 of the last slice: tail[0 .. count - 4 * n4) are the values past the last float4.
__device__ __forceinline__ void add_tail(double& acc, const float* tail, long long n4, long long count)
{
    for (long long q = n4 << 2; q < count; ++q) acc += (double)tail[q - (n4 << 2)];
}

__device__ __forceinline__ void wave_sum(double& acc)
{
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
}

// Every thread of the workgroup calls this with its combined value; the wave sums are in s[WAVES] (LDS) afterwards.
__device__ __forceinline__ void stage_wave_sums(double acc, double* s)
{
    wave_sum(acc);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
    __syncthreads();
}

// By one thread, after stage_wave_sums: the slice's sum.
__device__ __forceinline__ double waves_in_order(const double* s)
{
    double tot = 0.0;
    for (int w = 0; w < WAVES; w++) tot += s[w];
    return tot;
}
#endif

}  // namespace ecc_sum

#endif
