// line_weights_kernel.hip -- the two kernels around the Radon kernel that turn a flagged-pixel image into line weights, gfx950
// (host side: ecc_line_weights.hip).
//
//   dilate_max_kernel   D(y, x) = max of the flagged image over the (2 dilate_px + 1)^2 square, edges clamped; image stack to image
//                       stack, never in place;
//   clip_min_kernel     W(ix, iy) = min over the (2 guard_bins + 1)^2 bins of clip(1 - L / zero_at_px, 0, 1), edges clamped; reads the
//                       elements of a slab stack of lengths L (private layout, ecc_layout.h) and writes the destination slabs
//                       COMPLETELY: elements, the replicated border rows and columns, zeros in the pitch padding.  Never in place.
//
// Both are ecc_extremum_tile.h's three phases -- load with halo, row pass, column pass -- over one 16 x 64 tile per 256-thread
// workgroup with a barrier between the phases.  The clip is applied as the tile is loaded, so the clipped weights exist in LDS only.
// Along the fast axis consecutive lanes read consecutive LDS words in every phase (no bank conflicts, no row padding); the windows
// are plain loops of 2 R + 1 LDS reads: at the caps that is 66 reads per output, against a Radon kernel that spends 0.5 ms per image.
// Plain loads and stores, no atomics, no scratch; LDS is static, sized for the caps (ecc_extremum::lds_*_floats).
#include <hip/hip_runtime.h>

#include "ecc_extremum_tile.h"
#include "ecc_layout.h"

namespace {

using namespace ecc_extremum;

template <class Op, int R_MAX, int BORDER, class Load, class Store>
__device__ __forceinline__ void run_tile(const Tile& t, Load load, Store store)
{
    __shared__ float in[lds_in_floats(R_MAX, BORDER)];
    __shared__ float tmp[lds_tmp_floats(R_MAX, BORDER)];
    const int tid = (int)threadIdx.x;
    load_tile(t, tid, THREADS, in, load);
    __syncthreads();
    row_pass<Op>(t, tid, THREADS, in, tmp);
    __syncthreads();
    col_pass<Op>(t, tid, THREADS, tmp, store);
}

__global__ __launch_bounds__(THREADS) void dilate_max_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t stride,
                                                             int n_u, int n_v, int radius)
{
    Tile t;
    t.rows = make_axis(n_v, 0, 0, radius, (int)blockIdx.y, TILE_ROWS);
    t.cols = make_axis(n_u, 0, 0, radius, (int)blockIdx.x, TILE_COLS);
    const float* s = src + (int64_t)blockIdx.z * stride;
    float* d = dst + (int64_t)blockIdx.z * stride;
    run_tile<Max, DILATE_MAX, 0>(
        t, [=](int r, int c) { return s[(size_t)r * n_u + c]; }, [=](int r, int c, float v) { d[(size_t)r * n_u + c] = v; });
}

__global__ __launch_bounds__(THREADS) void clip_min_kernel(const float* __restrict__ lengths, int64_t lengths_stride,
                                                           float* __restrict__ dst, int64_t dst_stride, int n_alpha, int n_t, int pitch,
                                                           int radius, float zero_at_px)
{
    Tile t;
    t.rows = make_axis(n_alpha, 1, 0, radius, (int)blockIdx.y, TILE_ROWS);
    t.cols = make_axis(n_t, 1, pitch - 1, radius, (int)blockIdx.x, TILE_COLS);
    const float* s = lengths + (int64_t)blockIdx.z * lengths_stride;
    float* d = dst + (int64_t)blockIdx.z * dst_stride;
    run_tile<Min, GUARD_MAX, 1>(
        t, [=](int r, int c) { return clip_weight(s[(size_t)(r + 1) * pitch + (c + 1)], zero_at_px); },
        [=](int r, int c, float v) { d[(size_t)(r + 1) * pitch + (c + 1)] = v; });
}

}  // namespace

// src, dst: n_img images of n_v x n_u floats, `stride` floats apart; 1 <= radius <= DILATE_MAX; dst must not overlap src.
extern "C" hipError_t ecc_launch_dilate_max(const float* src, float* dst, int64_t stride, int n_img, int n_u, int n_v, int radius,
                                            hipStream_t stream)
{
    const dim3 grid(Axis::tiles(n_u, 0, 0, TILE_COLS), Axis::tiles(n_v, 0, 0, TILE_ROWS), n_img);
    hipLaunchKernelGGL(dilate_max_kernel, grid, dim3(THREADS), 0, stream, src, dst, stride, n_u, n_v, radius);
    return hipGetLastError();
}

// lengths, dst: n_img slabs in the private layout; 0 <= radius <= GUARD_MAX; dst must not overlap lengths.  Of `lengths` only the
// elements are read; every float of the n_img destination slabs is written.
extern "C" hipError_t ecc_launch_clip_min(const float* lengths, int64_t lengths_stride, float* dst, int64_t dst_stride, int n_img,
                                          int n_alpha, int n_t, int pitch, int radius, float zero_at_px, hipStream_t stream)
{
    const dim3 grid(Axis::tiles(n_t, 1, pitch - 1, TILE_COLS), Axis::tiles(n_alpha, 1, 0, TILE_ROWS), n_img);
    hipLaunchKernelGGL(clip_min_kernel, grid, dim3(THREADS), 0, stream, lengths, lengths_stride, dst, dst_stride, n_alpha, n_t, pitch,
                       radius, zero_at_px);
    return hipGetLastError();
}
