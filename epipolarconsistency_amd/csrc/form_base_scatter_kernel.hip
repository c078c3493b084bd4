// form_base_scatter_kernel.hip -- the refresh of kept base columns (ecc_metric_set_form_incremental; gfx950): the T
// columns of a pose grid whose ONE pose is "the changed views at their current matrices" are copied to the all-pairs positions of the
// metric's kept columns, so that the kept columns are again those of an all-pairs launch at the current matrices.
//
// The grid is the pose batch's (ecc_poses.hip, ecc_form_call.h): c columns, one per changed view M[a] (ascending), entry (partner u,
// column a) at vals[col * vals_stride + u * c + a] -- the layout sum_weighted_poses_kernel reads with o0 = 0 and Q = c.  Where it
// goes: ecc_pose_scatter::position (holes skipped, a pair of two changed views once, from the column of the lower view).  The
// positions of the non-hole entries are pairwise different (tests/test_form_incremental_abi.py), so every destination has one
// writer: one thread per entry, one pass over the T columns, plain 4-byte vector loads and stores.  No atomics, no LDS beyond the
// changed views, no inline assembly, no scratch.  Neighbouring threads read neighbouring entries; the stores of one column of the grid
// are a run of a row or a stride through a column of the pair triangle, n - 1 values per changed view.
#include <hip/hip_runtime.h>

#include "ecc_pose_scatter.h"

#ifndef ECC_POSE_BATCH_MAX_MOVED
#define ECC_POSE_BATCH_MAX_MOVED 32  // (ecc_poses.hip)
#endif

namespace {

constexpr int SCATTER_THREADS = 256;

__global__ __launch_bounds__(SCATTER_THREADS) void form_base_scatter_kernel(const float* __restrict__ vals, long long vals_stride, int n, int c,
                                                                            const int32_t* __restrict__ M_d, int T,
                                                                            float* __restrict__ base_cols, long long base_stride)
{
    __shared__ int M[ECC_POSE_BATCH_MAX_MOVED];
    if ((int)threadIdx.x < c) M[threadIdx.x] = M_d[threadIdx.x];
    __syncthreads();
    const long long e = (long long)blockIdx.x * SCATTER_THREADS + threadIdx.x;
    if (e >= (long long)n * c) return;
    const int u = (int)(e / c), a = (int)(e - (long long)u * c);
    const long long ij = ecc_pose_scatter::position(u, a, M, n);
    if (ij == ecc_pose_scatter::HOLE) return;
    for (int col = 0; col < T; ++col) base_cols[(long long)col * base_stride + ij] = vals[(long long)col * vals_stride + e];
}

}  // namespace

// c changed views (1 .. ECC_POSE_BATCH_MAX_MOVED, M_d: device, strictly ascending, in [0, n)), their grid's T columns in vals (n c
// entries each, vals_stride apart), the kept T columns of n (n - 1) / 2 values in base_cols (base_stride apart).
extern "C" hipError_t ecc_launch_form_base_scatter(const float* vals, long long vals_stride, int n, int c, const int32_t* M_d, int T,
                                                   float* base_cols, long long base_stride, hipStream_t stream)
{
    if (n < 2 || c < 1 || c > ECC_POSE_BATCH_MAX_MOVED || c > n || T < 1 || vals_stride < (long long)n * c ||
        base_stride < (long long)n * (n - 1) / 2 || !vals || !M_d || !base_cols)
        return hipErrorInvalidValue;
    const long long entries = (long long)n * c;
    hipLaunchKernelGGL(form_base_scatter_kernel, dim3((unsigned)((entries + SCATTER_THREADS - 1) / SCATTER_THREADS)), dim3(SCATTER_THREADS), 0,
                       stream, vals, vals_stride, n, c, M_d, T, base_cols, base_stride);
    return hipGetLastError();
}
