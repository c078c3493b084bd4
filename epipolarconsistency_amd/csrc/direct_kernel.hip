// direct_kernel.hip -- MetricDirect: epipolar consistency straight from the projection images.
//
// The reference evaluates one pair at a time from the host (ref: LibEpipolarConsistency/EpipolarConsistencyDirect.cpp:
// 67-219,247-259): per pair it builds the kappa grid and the 2 x n_lines epipolar lines on the host in float64,
// uploads them, launches kernel_computeLineIntegrals twice (EpipolarConsistencyDirect.cu:31-125; 32-thread blocks,
// texture fetches, a device-wide sync after each), reads both signals back and sums on the host.  Here a batch of
// pairs is four stream-ordered launches with nothing crossing PCIe but the final scalar:
//   direct_view_kernel   thread per view: source position and the row-QR factors of P (float64)
//   direct_pair_kernel   thread per pair: baseline, the two reference planes, kappa range/step, line count
//   direct_lines_kernel  thread per (pair, image, kappa): the line in float64 -> float, then the reference's
//                        fp32 line integral (0.4-px steps, two parallel lines half a pixel apart) with the exact
//                        bilinear rule on the image in global memory; neighbouring threads are neighbouring lines
//                        of the pencil, so their taps share cache lines
//   direct_reduce_kernel wave per pair: sum (v0-v1)^2 dkappa in float64 (fixed order), cost image entry
// setFanBeamConsistency (RectifiedFBCC.h, ...Direct.cpp:133-196): the pair kernel also builds the two rectifying
// homographies, and each line thread derives its LinePerspectivity weighting in float64 before a weighted plain
// line integral -- the reference does that per line on the host.
// Arithmetic follows oracle/ecc_oracle.c (eccor_direct_pair): line integrals are bit-identical for identical
// lines; the lines themselves differ from the oracle's only through the float64 sin/cos of the two libms.
// The record, the lines and the line integrals themselves are ecc_direct_lines.h, shared with direct_list_kernel.hip.
#include <hip/hip_runtime.h>
#include <math.h>

#include "ecc_host_geometry.h"
#include "ecc_layout.h"
#include "ecc_sampling.h"
#ifdef ECC_DIRECT_STATS  // scripts/direct_stats.py: slabs, steps through the tile / through global memory (radon_kernel.hip's scheme)
__device__ unsigned long long g_direct_stats[8];
#define ECC_SLAB_STAT(i, v) atomicAdd(&g_direct_stats[i], (unsigned long long)(v))
#endif
#include "ecc_direct_lines.h"

namespace {

__global__ __launch_bounds__(64) void direct_view_kernel(const double* __restrict__ Ps, int n, EccDirectView* __restrict__ views,
                                                         int n_u, int n_v)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    double P[12];
    for (int k = 0; k < 12; ++k) P[k] = Ps[12 * (size_t)v + k];
    EccDirectView out;
    ecc_host::camera_center(P, out.C);
    ecc_host::RowQR f;
    ecc_host::row_qr(P, &f);
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 4; ++k) out.Q[4 * i + k] = f.Q[i][k];
        for (int j = 0; j < 3; ++j) out.L[3 * i + j] = f.L[i][j];
    }
    out.radius = ecc_host::object_radius(P, n_u, n_v);
    for (int k = 0; k < 12; ++k) out.P[k] = P[k];
    views[v] = out;
}

__global__ __launch_bounds__(256) void direct_pair_kernel(EccDirectParams p)
{
    const long long local = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (local >= p.count) return;
    int i, j;
    if (p.idx2) {
        i = p.idx2[2 * local];
        j = p.idx2[2 * local + 1];
    } else {
        ecc_get_ij_device(p.first + local, p.n_views, i, j);
    }
    direct_pair_record(p, local, i, j);
}

// The two line-integral kernels: a pair's two sides are views r.i and r.j, matrix and image alike (the list forms, where they
// are not: direct_list_kernel.hip).
__global__ __launch_bounds__(256) void direct_lines_gather_kernel(EccDirectParams p)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const long long pair = blockIdx.y;
    const int which = blockIdx.z;
    const EccDirectPair& r = p.pairs[pair];
    if (k >= r.n_lines) return;
    const EccDirectView& V = p.views[which ? r.j : r.i];
    float lf0, lf1, lf2, kf;
    direct_line_of(p, r, V, k, lf0, lf1, lf2, kf);
    const bool use_T = p.imagesT && fabsf(lf1) > fabsf(lf0);
    const float* img = (use_T ? p.imagesT : p.images) + (int64_t)(which ? r.j : r.i) * p.image_stride;
    const int si = use_T ? p.n_v : 1, sj = use_T ? 1 : p.n_u;
    const ecc_slab::LineRun ln = direct_line_run(lf0, lf1, lf2, p.n_u, p.n_v);
    float v = 0.f;
    if (ln.active) {
        if (p.use_fbcc) {
            DirectFbccSum acc;
            const float lf[3] = {lf0, lf1, lf2};
            ecc_host::fbcc_line_info(V.P, V.C, which ? r.H1 : r.H0, r.dvec, r.Eplane, lf, &acc.fbcc);
            for (float t = ln.t; t <= ln.t_max; t += 0.4f)
                acc.add(ecc_tex_global_strided(img, p.n_u, p.n_v, si, sj, ln.o0 + t * ln.d0, ln.o1 + t * ln.d1), 0.f, t);
            v = acc.sum;
        } else {
            DirectDerivSums acc;
            const float h0 = 0.5f * lf0, h1 = 0.5f * lf1;
            for (float t = ln.t; t <= ln.t_max; t += 0.4f) {
                const float x = ln.o0 + t * ln.d0, y = ln.o1 + t * ln.d1;
                acc.add(ecc_tex_global_strided(img, p.n_u, p.n_v, si, sj, x + h0, y + h1),
                        ecc_tex_global_strided(img, p.n_u, p.n_v, si, sj, x - h0, y - h1), t);
            }
            v = acc.sump - acc.summ;
        }
    }
    p.samples[((size_t)pair * 2 + which) * p.n_max + k] = v;
    if (p.debug_lines && pair == 0) {
        float* dl = p.debug_lines + 6 * (size_t)k + 3 * which;
        dl[0] = lf0;
        dl[1] = lf1;
        dl[2] = lf2;
        if (which == 0) p.debug_kappas[k] = kf;
    }
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void direct_lines_kernel(EccDirectParams p)
{
    __shared__ ecc_slab::Shared sh;
    __shared__ float s_first_line[2];
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const long long pair = blockIdx.y;
    const int which = blockIdx.z;  // 0: first view of the pair, 1: second
    const EccDirectPair& r = p.pairs[pair];
    if ((int)(blockIdx.x * blockDim.x) >= r.n_lines) return;  // uniform: nothing below this line returns early
    const bool live = k < r.n_lines;
    const EccDirectView& V = p.views[which ? r.j : r.i];
    float lf0 = 0.f, lf1 = 1.f, lf2 = 0.f, kf = 0.f;
    if (live) direct_line_of(p, r, V, k, lf0, lf1, lf2, kf);
    ecc_slab::LineRun ln = direct_line_run(lf0, lf1, lf2, p.n_u, p.n_v);
    ln.active = ln.active && live;
    ecc_host::FbccInfo info;
    if (p.use_fbcc && live) {
        const float lf[3] = {lf0, lf1, lf2};
        ecc_host::fbcc_line_info(V.P, V.C, which ? r.H1 : r.H0, r.dvec, r.Eplane, lf, &info);
    }
    // The workgroup's tile orientation, walking direction and window slope come from its first line (uniform): the
    // tile's fast axis is the image axis the line NORMAL is closer to (as in the Radon kernel); lines with y-normals
    // stage from the transposed copy of the images.
    if (threadIdx.x == 0) {
        s_first_line[0] = lf0;
        s_first_line[1] = lf1;
    }
    __syncthreads();
    const float n0 = ecc_slab::uni(s_first_line[0]), n1 = ecc_slab::uni(s_first_line[1]);
    const float* img = p.images + (int64_t)(which ? r.j : r.i) * p.image_stride;
    const float* imgT = p.imagesT ? p.imagesT + (int64_t)(which ? r.j : r.i) * p.image_stride : nullptr;
    const bool transp = imgT && fabsf(n1) > fabsf(n0);
    // direction (d0, d1) = (l1, -l0); plain tile: s = y, ds = -l0, df = l1; transposed: s = x, ds = l1, df = -l0
    const float ds0 = transp ? n1 : -n0, df0 = transp ? -n0 : n1;
    const float sigma = ds0 >= 0.f ? 1.f : -1.f;
    const float beta0 = df0 / (fabsf(ds0) > 1e-6f ? ds0 : 1e-6f);
    float v;
    if (transp) v = direct_lines_body<true>(p, sh, img, imgT, ln, 0.5f * lf0, 0.5f * lf1, sigma, beta0, p.use_fbcc ? &info : nullptr);
    else v = direct_lines_body<false>(p, sh, img, imgT, ln, 0.5f * lf0, 0.5f * lf1, sigma, beta0, p.use_fbcc ? &info : nullptr);
    if (!live) return;
    if (!ln.active) v = 0.f;
    p.samples[((size_t)pair * 2 + which) * p.n_max + k] = v;
    if (p.debug_lines && pair == 0) {
        float* dl = p.debug_lines + 6 * (size_t)k + 3 * which;
        dl[0] = lf0;
        dl[1] = lf1;
        dl[2] = lf2;
        if (which == 0) p.debug_kappas[k] = kf;
    }
}

// ref: EpipolarConsistencyDirect.cpp:205-208 (metric += (v0-v1)*(v0-v1)*dkappa, float difference and square)
__global__ __launch_bounds__(256) void direct_reduce_kernel(EccDirectParams p)
{
    const int lane = threadIdx.x & 63;
    const long long pair = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= p.count) return;
    const EccDirectPair& r = p.pairs[pair];
    const float* v0 = p.samples + (size_t)pair * 2 * p.n_max;
    const float* v1 = v0 + p.n_max;
    double acc = 0.0;
    for (int k = lane; k < r.n_lines; k += 64) {
        const float d = v0[k] - v1[k];
        acc += (double)(d * d) * r.dkappa;
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    if (lane == 0) {
        p.pair_metric[pair] = acc;
        if (p.cost) p.cost[(size_t)r.i + (size_t)r.j * p.n_views] = (float)acc;  // ref: :255 cost_image.pixel(i,j)
        if (p.pair_lines) p.pair_lines[pair] = r.n_lines;
    }
}

// Sum of `count` float64 pair metrics in a fixed order, added to *total (ref: :247-259, cost += ecc).
__global__ __launch_bounds__(1024) void direct_sum_kernel(const double* __restrict__ vals, long long count,
                                                          double* __restrict__ total)
{
    const double tot = direct_block_sum(vals, count);
    if (threadIdx.x == 0) *total += tot;
}

// Transposed copies of the images (u becomes the slow axis), tiled through LDS.
__global__ void direct_transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int W, int H, int64_t stride)
{
    __shared__ float tl[32][33];
    const float* s = src + (int64_t)blockIdx.z * stride;
    float* d = dst + (int64_t)blockIdx.z * stride;
    const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 32;
    for (int r = threadIdx.y; r < 32; r += blockDim.y) {
        const int x = x0 + threadIdx.x, y = y0 + r;
        tl[r][threadIdx.x] = (x < W && y < H) ? s[(size_t)y * W + x] : 0.f;
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 32; r += blockDim.y) {
        const int x = x0 + r, y = y0 + threadIdx.x;
        if (x < W && y < H) d[(size_t)x * H + y] = tl[threadIdx.x][r];
    }
}

}  // namespace

extern "C" hipError_t ecc_launch_direct_transpose(const float* src, float* dst, int n, int W, int H, hipStream_t stream)
{
    dim3 grid((W + 31) / 32, (H + 31) / 32, n), block(32, 8);
    hipLaunchKernelGGL(direct_transpose_kernel, grid, block, 0, stream, src, dst, W, H, (int64_t)W * H);
    return hipGetLastError();
}

extern "C" hipError_t ecc_launch_direct_views(const double* Ps_d, int n, EccDirectView* views, int n_u, int n_v,
                                              hipStream_t stream)
{
    hipLaunchKernelGGL(direct_view_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, Ps_d, n, views, n_u, n_v);
    return hipGetLastError();
}

// The float64 value of every pair of a batch from its line integrals (p->pairs, p->samples -> p->pair_metric).
extern "C" hipError_t ecc_launch_direct_reduce(const EccDirectParams* p, hipStream_t stream)
{
    hipLaunchKernelGGL(direct_reduce_kernel, dim3((unsigned)((p->count + 3) / 4)), dim3(256), 0, stream, *p);
    return hipGetLastError();
}

// One batch: p->count pairs starting at p->first (get_ij order); p->count <= 65535.
extern "C" hipError_t ecc_launch_direct_batch(const EccDirectParams* p, double* total, hipStream_t stream)
{
    if (p->count <= 0) return hipSuccess;
    hipLaunchKernelGGL(direct_pair_kernel, dim3((unsigned)((p->count + 255) / 256)), dim3(256), 0, stream, *p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    dim3 grid((p->n_max + 255) / 256, (unsigned)p->count, 2);
    if (p->n_u < DIRECT_SLAB_MIN_SIZE || p->n_v < DIRECT_SLAB_MIN_SIZE)
        hipLaunchKernelGGL(direct_lines_gather_kernel, grid, dim3(256), 0, stream, *p);
    else
        hipLaunchKernelGGL(direct_lines_kernel, grid, dim3(256), 0, stream, *p);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = ecc_launch_direct_reduce(p, stream);
    if (e != hipSuccess) return e;
    if (total) {
        hipLaunchKernelGGL(direct_sum_kernel, dim3(1), dim3(1024), 0, stream, p->pair_metric, p->count, total);
        e = hipGetLastError();
    }
    return e;
}

#ifdef ECC_DIRECT_STATS
extern "C" __attribute__((visibility("default"))) void ecc_debug_direct_stats(unsigned long long* out, int reset)
{
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_direct_stats), sizeof(unsigned long long) * 8);
    if (reset) {
        const unsigned long long z[8] = {0};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_direct_stats), z, sizeof(z));
    }
}
#endif
