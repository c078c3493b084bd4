// weighted_transforms_kernel.hip -- the segmented float64 sums of ecc_metric_evaluate_weighted_transforms (gfx950): per transform the
// sums of BOTH columns {c, u} over its `count` = n_source n_target cross pairs in the order of ecc_sum_order.h, so that
// sum c / sum u of a transform has the bits of ecc_metric_set_projections(composed matrices) + ecc_metric_evaluate_weighted_pairs.
// Nothing here knows about line weights: the kernel sums columns 0 and 1 of any column-form buffer, and
// ecc_metric_evaluate_robust_transforms (ecc_robust_batches.hip) uses it for {c, u} of its three columns {c, u, r}.
//
// sum_weighted_transforms_kernel<SLICES>: workgroup (slice, transform, column).  The weighted pair launch has no value slots: it
// leaves column `col` of grid entry e at val_cols[col * col_stride + e], and the grid is pair-major (ecc_transform_grid.h), so the
// values of transform k lie K floats apart.  The kernel reads them where they are: thread t gathers the four entries of its float4
// kk = lo + t, lo + t + 1024, ... with four scalar loads and adds them as ecc_sum::add does.  No transposition through LDS: a
// transform's neighbours k + 1, k + 2, ... are the neighbouring workgroups and read the same cache lines, the two columns of a
// batch are at most 8 MB (2 x 2^20 floats) and were written by the launch in front, and the sum is a few percent of a batch
// (DESIGN.md 4.17 has the measurement).
// The slice sums of a (transform, column) are added to 0.0 in slice order -- also the single one of the one-slice form, because
// ecc_metric_evaluate_weighted_pairs' host loop adds its one slice sum to 0.0 (-0.0 becomes +0.0 there, and so it does here).
// Results: 2 K float64 words in pinned host memory, word 2 k + col, system-scope stores.  Plain vector loads and stores, no atomics
// on data, no inline assembly.
#include <hip/hip_runtime.h>

#include "ecc_sum_order.h"
#include "ecc_transform_grid.h"

namespace {

constexpr int SUM_THREADS = ecc_sum::THREADS;

__device__ __forceinline__ void store_result(double* out_host, long long word, double v)
{
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(out_host) + word, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}

template <int SLICES>
__global__ __launch_bounds__(SUM_THREADS) void sum_weighted_transforms_kernel(const float* __restrict__ val_cols, long long col_stride,
                                                                              long long count, int K, double* __restrict__ partial,
                                                                              double* __restrict__ out_host)
{
    __shared__ float tail[4];
    __shared__ double s[SUM_THREADS / 64];
    const int k = blockIdx.y, slice = blockIdx.x, col = blockIdx.z, t = threadIdx.x;
    const float* __restrict__ v = val_cols + (long long)col * col_stride;
    const long long n4 = count >> 2;
    long long lo, hi;
    ecc_sum::slice_bounds(n4, SLICES, slice, &lo, &hi);
    ecc_sum::Acc4 acc4;
    for (long long kk = lo + t; kk < hi; kk += SUM_THREADS) {
        float f[4];
        ecc_transform_grid::gather4(v, kk, k, K, f);
        ecc_sum::add(acc4, make_float4(f[0], f[1], f[2], f[3]));
    }
    double acc = ecc_sum::combine(acc4);
    if (slice == SLICES - 1 && t == 0) {  // the up to three values past the last float4 (written and read by this thread alone)
        for (int c = 0; c < 4; ++c) tail[c] = (n4 << 2) + c < count ? ecc_transform_grid::value(v, (n4 << 2) + c, k, K) : 0.f;
        ecc_sum::add_tail(acc, tail, n4, count);
    }
    ecc_sum::stage_wave_sums(acc, s);
    if (t == 0) {
        const double part = ecc_sum::waves_in_order(s);
        const long long word = 2ll * k + col;
        if (SLICES == 1) store_result(out_host, word, 0.0 + part);  // one slice: added to 0.0 as the host loop of the list call adds it
        else partial[word * SLICES + slice] = part;
    }
}

// The sixteen-slice form's finish: the slice sums of (transform, column) word = 2 k + col added to 0.0 in slice order.
__global__ __launch_bounds__(256) void finish_weighted_transforms_kernel(const double* __restrict__ partial, int slices, int n_words,
                                                                         double* __restrict__ out_host)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    double tot = 0.0;
    for (int b = 0; b < slices; ++b) tot += partial[(size_t)w * slices + b];
    store_result(out_host, w, tot);
}

}  // namespace

// K transforms (1 .. 32768) over `count` pairs each: the grid's two columns in val_cols (count K entries each, col_stride apart).
// slices: 1 or ecc_sum::SLICES.  partial_d: 2 K ecc_sum::SLICES doubles.  out_host_dev: the device address of 2 K pinned result words.
extern "C" hipError_t ecc_launch_sum_weighted_transforms(const float* val_cols, long long col_stride, long long count, int K, int slices,
                                                         double* partial_d, double* out_host_dev, hipStream_t stream)
{
    if (K < 1 || K > 32768 || count < 1 || col_stride < count * K || (slices != 1 && slices != ecc_sum::SLICES) || !val_cols || !partial_d ||
        !out_host_dev)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)slices, (unsigned)K, 2u);
    if (slices == 1)
        hipLaunchKernelGGL(sum_weighted_transforms_kernel<1>, grid, dim3(SUM_THREADS), 0, stream, val_cols, col_stride, count, K, partial_d,
                           out_host_dev);
    else
        hipLaunchKernelGGL((sum_weighted_transforms_kernel<ecc_sum::SLICES>), grid, dim3(SUM_THREADS), 0, stream, val_cols, col_stride, count, K,
                           partial_d, out_host_dev);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || slices == 1) return e;
    hipLaunchKernelGGL(finish_weighted_transforms_kernel, dim3((unsigned)((2 * K + 255) / 256)), dim3(256), 0, stream, partial_d, slices, 2 * K,
                       out_host_dev);
    return hipGetLastError();
}
