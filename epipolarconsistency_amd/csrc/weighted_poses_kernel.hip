// weighted_poses_kernel.hip -- the segmented float64 sums of ecc_metric_evaluate_weighted_pose_deltas (gfx950): per pose the sums of
// BOTH columns {c, u} over all n (n - 1) / 2 pairs -- the base's column with the pose's own entries substituted -- in the order of
// ecc_sum_order.h, so that sum c / sum u of a pose has the bits of ecc_metric_set_projections + ecc_metric_evaluate_weighted.
// Nothing here knows about line weights: the kernel sums columns 0 and 1 of any column-form buffer, and
// ecc_metric_evaluate_robust_pose_deltas (ecc_robust_batches.hip) uses it for {c, u} of its three columns {c, u, r}.
//
// sum_weighted_poses_kernel<SLICES> is sum_poses_kernel (ecc_poses.hip) for column `col` of the base (base + col * base_stride) and
// column `col` of the grid's values (vals + col * vals_stride): workgroup (slice, pose, column); the slice is staged through LDS in
// chunks of ecc_pose_scatter::STAGE_F4 float4, the pose's entries that fall into the chunk are put over the base's
// (ecc_pose_scatter.h: holes skipped, a pair of two moved views once), and the 1024 threads add from LDS.
// The slice sums of a (pose, column) are added to 0.0 in slice order -- also the single one of the one-slice form, because
// ecc_metric_evaluate_weighted's host loop adds its one slice sum to 0.0 (-0.0 becomes +0.0 there, and so it does here).
// Results: 2 K float64 words in pinned host memory, word 2 k + col, system-scope stores.  Plain vector loads and stores, no atomics
// on data, no inline assembly.
#include <hip/hip_runtime.h>

#include "ecc_pose_scatter.h"
#include "ecc_sum_order.h"

#ifndef ECC_POSE_BATCH_MAX_MOVED
#define ECC_POSE_BATCH_MAX_MOVED 32  // (ecc_poses.hip)
#endif

namespace {

constexpr int SUM_THREADS = ecc_sum::THREADS, STAGE_F4 = ecc_pose_scatter::STAGE_F4;

__device__ __forceinline__ void store_result(double* out_host, long long word, double v)
{
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(out_host) + word, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}

// lists_d: pose_list_kernel's copy of the lists (n_poses + 1 offsets, then the Q moved views).  vals: entry (u, q) at u * Q + q.
template <int SLICES>
__global__ __launch_bounds__(SUM_THREADS) void sum_weighted_poses_kernel(const float* __restrict__ base_cols, long long base_stride, long long count,
                                                                         int n, int Q, const int32_t* __restrict__ lists_d, int n_poses,
                                                                         const float* __restrict__ val_cols, long long vals_stride,
                                                                         double* __restrict__ partial, double* __restrict__ out_host)
{
    __shared__ float stage[4 * STAGE_F4];
    __shared__ float tail[4];
    __shared__ int M[ECC_POSE_BATCH_MAX_MOVED];
    __shared__ double s[SUM_THREADS / 64];
    const int k = blockIdx.y, slice = blockIdx.x, col = blockIdx.z, t = threadIdx.x;
    const float* __restrict__ base = base_cols + (long long)col * base_stride;
    const float* __restrict__ vals = val_cols + (long long)col * vals_stride;
    const int o0 = lists_d[k], c = lists_d[k + 1] - o0;
    if (t < c) M[t] = lists_d[n_poses + 1 + o0 + t];
    const long long n4 = count >> 2;
    long long lo, hi;
    ecc_sum::slice_bounds(n4, SLICES, slice, &lo, &hi);
    const bool owns_tail = slice == SLICES - 1;
    const float4* __restrict__ b4 = reinterpret_cast<const float4*>(base);
    ecc_sum::Acc4 acc4;
    if (owns_tail && t < 4) tail[t] = (n4 << 2) + t < count ? base[(n4 << 2) + t] : 0.f;
    bool first_chunk = true;
    for (long long c0 = lo; c0 < hi || first_chunk; c0 += STAGE_F4) {
        const long long ce = min(hi, c0 + STAGE_F4);
        for (long long kk = c0 + t; kk < ce; kk += SUM_THREADS) reinterpret_cast<float4*>(stage)[kk - c0] = b4[kk];
        __syncthreads();  // the chunk of the base (and M, tail) is in LDS
        for (int e = t; e < c * n; e += SUM_THREADS) {
            const int a = e / n, u = e - a * n;
            const long long ij = ecc_pose_scatter::position(u, a, M, n);
            if (ij == ecc_pose_scatter::HOLE) continue;
            const bool in_chunk = ij >= (c0 << 2) && ij < (ce << 2);
            const bool in_tail = owns_tail && first_chunk && ij >= (n4 << 2);
            if (in_chunk || in_tail) {
                const float val = vals[(size_t)u * Q + o0 + a];
                if (in_chunk) stage[ij - (c0 << 2)] = val;
                else tail[ij - (n4 << 2)] = val;
            }
        }
        __syncthreads();
        for (long long kk = c0 + t; kk < ce; kk += SUM_THREADS) ecc_sum::add(acc4, reinterpret_cast<const float4*>(stage)[kk - c0]);
        __syncthreads();  // before the next chunk overwrites the stage
        first_chunk = false;
    }
    double acc = ecc_sum::combine(acc4);
    if (owns_tail && t == 0) ecc_sum::add_tail(acc, tail, n4, count);
    ecc_sum::stage_wave_sums(acc, s);
    if (t == 0) {
        const double part = ecc_sum::waves_in_order(s);
        const long long word = 2ll * k + col;
        if (SLICES == 1) store_result(out_host, word, 0.0 + part);  // one slice: added to 0.0 as the host loop of ecc_weighted.hip adds it
        else partial[word * SLICES + slice] = part;
    }
}

// The sixteen-slice form's finish: the slice sums of (pose, column) word = 2 k + col added to 0.0 in slice order.
__global__ __launch_bounds__(256) void finish_weighted_poses_kernel(const double* __restrict__ partial, int slices, int n_words,
                                                                    double* __restrict__ out_host)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    double tot = 0.0;
    for (int b = 0; b < slices; ++b) tot += partial[(size_t)w * slices + b];
    store_result(out_host, w, tot);
}

}  // namespace

// K poses (1 .. 2^19 / (2 SLICES)), the lists in lists_d, the grid's two columns in val_cols (n Q entries each, vals_stride apart), the
// base's two columns of `count` = n (n - 1) / 2 values in base_cols (base_stride apart, a multiple of 4).  slices: 1 or
// ecc_sum::SLICES.  partial_d: 2 K ecc_sum::SLICES doubles.  out_host_dev: the device address of 2 K pinned result words.
extern "C" hipError_t ecc_launch_sum_weighted_poses(const float* base_cols, long long base_stride, long long count, int n, int Q,
                                                    const int32_t* lists_d, int K, const float* val_cols, long long vals_stride, int slices,
                                                    double* partial_d, double* out_host_dev, hipStream_t stream)
{
    if (K < 1 || (long long)K * 2 * ecc_sum::SLICES > (1ll << 19) || n < 2 || count != (long long)n * (n - 1) / 2 || Q < 0 ||
        base_stride < count || (base_stride & 3) || vals_stride < (long long)n * Q || (slices != 1 && slices != ecc_sum::SLICES) || !base_cols ||
        !val_cols || !lists_d || !partial_d || !out_host_dev)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)slices, (unsigned)K, 2u);
    if (slices == 1)
        hipLaunchKernelGGL(sum_weighted_poses_kernel<1>, grid, dim3(SUM_THREADS), 0, stream, base_cols, base_stride, count, n, Q, lists_d, K, val_cols,
                           vals_stride, partial_d, out_host_dev);
    else
        hipLaunchKernelGGL((sum_weighted_poses_kernel<ecc_sum::SLICES>), grid, dim3(SUM_THREADS), 0, stream, base_cols, base_stride, count, n, Q, lists_d,
                           K, val_cols, vals_stride, partial_d, out_host_dev);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || slices == 1) return e;
    hipLaunchKernelGGL(finish_weighted_poses_kernel, dim3((unsigned)((2 * K + 255) / 256)), dim3(256), 0, stream, partial_d, slices, 2 * K, out_host_dev);
    return hipGetLastError();
}
