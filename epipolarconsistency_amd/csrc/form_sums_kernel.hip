// form_sums_kernel.hip -- the segmented float64 sums of a pair form with S summed columns, all S in ONE walk (gfx950): per pose the
// sums of columns 0 .. S - 1 over all n (n - 1) / 2 pairs with the pose's own entries substituted, per transform the sums of the
// same columns over its cross list, each column in the order of ecc_sum_order.h.  The weighted-robust batches
// (ecc_weighted_robust_batches.hip) sum S = 3 columns {c, u, k} of their four; S is a template parameter and only S = 3 is
// instantiated.  The two-column sums (weighted_poses_kernel.hip, weighted_transforms_kernel.hip) stay as they are: they give one
// workgroup to every (slice, pose, column), so every column walks the pose's grid entries through position() again, and calling
// them twice for three columns would also sum a column nobody adds.
//
// sum_form_poses_kernel<SLICES, S>       workgroup (slice, pose).  Per chunk of CHUNK_F4 float4 of the slice: the chunk of EACH of
//                                        the S base columns is staged in LDS (S x 16 KiB); the pose's c n grid entries are walked
//                                        ONCE, ecc_pose_scatter::position() once per entry, and the entry's S values are put over the
//                                        S staged columns (holes skipped, a pair of two moved views once); then thread t adds its
//                                        float4 of every column from LDS into that column's ecc_sum::Acc4.  CHUNK_F4 == THREADS:
//                                        thread t's float4 of chunk i is lo + t + i THREADS, its own order of ecc_sum_order.h.
// sum_form_transforms_kernel<SLICES, S>  workgroup (slice, transform).  The grid is pair-major (ecc_transform_grid.h): the four
//                                        entries of float4 kk of transform k are formed once and used for S loads each, col_stride
//                                        apart.
// finish_form_sums_kernel                the sixteen-slice forms' finish: the slice sums of a word added to 0.0 in slice order.
// Per column the additions are those of the two-column kernels: Acc4 per thread, combine, the up to three values past the last
// float4 by thread 0 of the last slice, stage_wave_sums, waves_in_order, the slice sums added to 0.0 in slice order (the single one
// too: -0.0 becomes +0.0 as in the host loops of the sequential calls).
// Results: S K float64 words in pinned host memory, word S k + col, system-scope stores.  Plain vector loads and stores, no atomics
// on data, no inline assembly.
#include <hip/hip_runtime.h>

#include "ecc_pose_scatter.h"
#include "ecc_sum_order.h"
#include "ecc_transform_grid.h"

#ifndef ECC_POSE_BATCH_MAX_MOVED
#define ECC_POSE_BATCH_MAX_MOVED 32  // (ecc_poses.hip)
#endif

namespace {

constexpr int SUM_THREADS = ecc_sum::THREADS;
// float4 per staged chunk and column: 16 KiB per column, 48 KiB for S = 3 -- under 64 KiB, so two workgroups fit on a CU.  A
// multiple of THREADS, so a thread's own order is kept across chunks.
constexpr int CHUNK_F4 = ecc_sum::THREADS;
static_assert(CHUNK_F4 % ecc_sum::THREADS == 0, "a thread's float4 stay its own across chunks");

__device__ __forceinline__ void store_result(double* out_host, long long word, double v)
{
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(out_host) + word, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}

// lists_d: pose_list_kernel's copy of the lists (n_poses + 1 offsets, then the Q moved views).  vals: entry (u, q) at u * Q + q.
template <int SLICES, int S>
__global__ __launch_bounds__(SUM_THREADS) void sum_form_poses_kernel(const float* __restrict__ base_cols, long long base_stride, long long count,
                                                                     int n, int Q, const int32_t* __restrict__ lists_d, int n_poses,
                                                                     const float* __restrict__ val_cols, long long vals_stride,
                                                                     double* __restrict__ partial, double* __restrict__ out_host)
{
    __shared__ float stage[S][4 * CHUNK_F4];
    __shared__ float tail[S][4];
    __shared__ int M[ECC_POSE_BATCH_MAX_MOVED];
    __shared__ double s[S][SUM_THREADS / 64];
    const int k = blockIdx.y, slice = blockIdx.x, t = threadIdx.x;
    const int o0 = lists_d[k], c = lists_d[k + 1] - o0;
    if (t < c) M[t] = lists_d[n_poses + 1 + o0 + t];
    const long long n4 = count >> 2;
    long long lo, hi;
    ecc_sum::slice_bounds(n4, SLICES, slice, &lo, &hi);
    const bool owns_tail = slice == SLICES - 1;
    ecc_sum::Acc4 acc4[S];
    if (owns_tail && t < 4 * S) {
        const int col = t >> 2, q = t & 3;
        tail[col][q] = (n4 << 2) + q < count ? base_cols[(long long)col * base_stride + (n4 << 2) + q] : 0.f;
    }
    bool first_chunk = true;
    for (long long c0 = lo; c0 < hi || first_chunk; c0 += CHUNK_F4) {
        const long long ce = min(hi, c0 + CHUNK_F4);
        const bool mine = c0 + t < ce;  // this thread's float4 of the chunk: c0 + t
        if (mine) {
#pragma unroll
            for (int col = 0; col < S; ++col)
                reinterpret_cast<float4*>(stage[col])[t] = reinterpret_cast<const float4*>(base_cols + (long long)col * base_stride)[c0 + t];
        }
        __syncthreads();  // the chunk of the base's columns (and M, tail) is in LDS
        for (int e = t; e < c * n; e += SUM_THREADS) {
            const int a = e / n, u = e - a * n;
            const long long ij = ecc_pose_scatter::position(u, a, M, n);
            if (ij == ecc_pose_scatter::HOLE) continue;
            const bool in_chunk = ij >= (c0 << 2) && ij < (ce << 2);
            const bool in_tail = owns_tail && first_chunk && ij >= (n4 << 2);
            if (in_chunk || in_tail) {
                const float* __restrict__ v = val_cols + (size_t)u * Q + o0 + a;
#pragma unroll
                for (int col = 0; col < S; ++col) {
                    const float val = v[(long long)col * vals_stride];
                    if (in_chunk) stage[col][ij - (c0 << 2)] = val;
                    else tail[col][ij - (n4 << 2)] = val;
                }
            }
        }
        __syncthreads();
        if (mine) {
#pragma unroll
            for (int col = 0; col < S; ++col) ecc_sum::add(acc4[col], reinterpret_cast<const float4*>(stage[col])[t]);
        }
        __syncthreads();  // before the next chunk overwrites the stage
        first_chunk = false;
    }
#pragma unroll
    for (int col = 0; col < S; ++col) {
        double acc = ecc_sum::combine(acc4[col]);
        if (owns_tail && t == 0) ecc_sum::add_tail(acc, tail[col], n4, count);
        ecc_sum::stage_wave_sums(acc, s[col]);
    }
    if (t < S) {
        const double part = ecc_sum::waves_in_order(s[t]);
        const long long word = (long long)S * k + t;
        if (SLICES == 1) store_result(out_host, word, 0.0 + part);  // one slice: added to 0.0 as the host loop of the all-pairs call adds it
        else partial[word * SLICES + slice] = part;
    }
}

template <int SLICES, int S>
__global__ __launch_bounds__(SUM_THREADS) void sum_form_transforms_kernel(const float* __restrict__ val_cols, long long col_stride, long long count,
                                                                          int K, double* __restrict__ partial, double* __restrict__ out_host)
{
    __shared__ float tail[S][4];
    __shared__ double s[S][SUM_THREADS / 64];
    const int k = blockIdx.y, slice = blockIdx.x, t = threadIdx.x;
    const long long n4 = count >> 2;
    long long lo, hi;
    ecc_sum::slice_bounds(n4, SLICES, slice, &lo, &hi);
    ecc_sum::Acc4 acc4[S];
    for (long long kk = lo + t; kk < hi; kk += SUM_THREADS) {
        long long e[4];  // the entries of gather4, once for the S columns
#pragma unroll
        for (int q = 0; q < 4; ++q) e[q] = ecc_transform_grid::entry(4 * kk + q, k, K);
#pragma unroll
        for (int col = 0; col < S; ++col) {
            const float* __restrict__ v = val_cols + (long long)col * col_stride;
            ecc_sum::add(acc4[col], make_float4(v[e[0]], v[e[1]], v[e[2]], v[e[3]]));
        }
    }
#pragma unroll
    for (int col = 0; col < S; ++col) {
        double acc = ecc_sum::combine(acc4[col]);
        if (slice == SLICES - 1 && t == 0) {  // the up to three values past the last float4 (written and read by this thread alone)
            const float* __restrict__ v = val_cols + (long long)col * col_stride;
            for (int q = 0; q < 4; ++q) tail[col][q] = (n4 << 2) + q < count ? ecc_transform_grid::value(v, (n4 << 2) + q, k, K) : 0.f;
            ecc_sum::add_tail(acc, tail[col], n4, count);
        }
        ecc_sum::stage_wave_sums(acc, s[col]);
    }
    if (t < S) {
        const double part = ecc_sum::waves_in_order(s[t]);
        const long long word = (long long)S * k + t;
        if (SLICES == 1) store_result(out_host, word, 0.0 + part);  // one slice: added to 0.0 as the host loop of the list call adds it
        else partial[word * SLICES + slice] = part;
    }
}

// The sixteen-slice forms' finish: the slice sums of word = S k + col added to 0.0 in slice order.
__global__ __launch_bounds__(256) void finish_form_sums_kernel(const double* __restrict__ partial, int slices, int n_words,
                                                               double* __restrict__ out_host)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    double tot = 0.0;
    for (int b = 0; b < slices; ++b) tot += partial[(size_t)w * slices + b];
    store_result(out_host, w, tot);
}

hipError_t finish_form_sums(int words, int slices, const double* partial_d, double* out_host_dev, hipStream_t stream)
{
    hipLaunchKernelGGL(finish_form_sums_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, partial_d, slices, words, out_host_dev);
    return hipGetLastError();
}

}  // namespace

// K poses (1 .. 16384), the lists in lists_d, the grid's S columns in val_cols (n Q entries each, vals_stride apart), the base's S
// columns of `count` = n (n - 1) / 2 values in base_cols (base_stride apart, a multiple of 4).  S: 3.  slices: 1 or
// ecc_sum::SLICES.  partial_d: S K ecc_sum::SLICES doubles.  out_host_dev: the device address of S K pinned result words.
extern "C" hipError_t ecc_launch_sum_form_poses(const float* base_cols, long long base_stride, long long count, int n, int Q,
                                                const int32_t* lists_d, int K, const float* val_cols, long long vals_stride, int S, int slices,
                                                double* partial_d, double* out_host_dev, hipStream_t stream)
{
    if (S != 3 || K < 1 || K > 16384 || n < 2 || count != (long long)n * (n - 1) / 2 || Q < 0 || base_stride < count || (base_stride & 3) ||
        vals_stride < (long long)n * Q || (slices != 1 && slices != ecc_sum::SLICES) || !base_cols || !val_cols || !lists_d || !partial_d ||
        !out_host_dev)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)slices, (unsigned)K);
    if (slices == 1)
        hipLaunchKernelGGL((sum_form_poses_kernel<1, 3>), grid, dim3(SUM_THREADS), 0, stream, base_cols, base_stride, count, n, Q, lists_d, K, val_cols,
                           vals_stride, partial_d, out_host_dev);
    else
        hipLaunchKernelGGL((sum_form_poses_kernel<ecc_sum::SLICES, 3>), grid, dim3(SUM_THREADS), 0, stream, base_cols, base_stride, count, n, Q,
                           lists_d, K, val_cols, vals_stride, partial_d, out_host_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || slices == 1) return e;
    return finish_form_sums(S * K, slices, partial_d, out_host_dev, stream);
}

// K transforms (1 .. 32768) over `count` pairs each: the grid's S columns in val_cols (count K entries each, col_stride apart).
// S: 3.  slices: 1 or ecc_sum::SLICES.  partial_d: S K ecc_sum::SLICES doubles.  out_host_dev: the device address of S K pinned
// result words.
extern "C" hipError_t ecc_launch_sum_form_transforms(const float* val_cols, long long col_stride, long long count, int K, int S, int slices,
                                                     double* partial_d, double* out_host_dev, hipStream_t stream)
{
    if (S != 3 || K < 1 || K > 32768 || count < 1 || col_stride < count * K || (slices != 1 && slices != ecc_sum::SLICES) || !val_cols ||
        !partial_d || !out_host_dev)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)slices, (unsigned)K);
    if (slices == 1)
        hipLaunchKernelGGL((sum_form_transforms_kernel<1, 3>), grid, dim3(SUM_THREADS), 0, stream, val_cols, col_stride, count, K, partial_d,
                           out_host_dev);
    else
        hipLaunchKernelGGL((sum_form_transforms_kernel<ecc_sum::SLICES, 3>), grid, dim3(SUM_THREADS), 0, stream, val_cols, col_stride, count, K,
                           partial_d, out_host_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || slices == 1) return e;
    return finish_form_sums(S * K, slices, partial_d, out_host_dev, stream);
}
