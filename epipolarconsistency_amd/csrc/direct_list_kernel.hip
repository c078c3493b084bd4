// direct_list_kernel.hip -- MetricDirect over index lists: the reference's tuples (P0, P1, I0, I1), where the matrices and the
// images of a pair are separate indices (ref: Metric::evaluate(indices, out), EpipolarConsistency.h; Gui/SingleImageMotion.h
// builds (input_index, i, input_index, i) for every other view i).  The kernels of direct_kernel.hip take a pair's two views as
// matrix and image alike; these take the view record from the matrix index and the pixels from the image index.  Record, lines
// and line integrals are the device functions of ecc_direct_lines.h, the ones direct_kernel.hip's kernels call: a list entry has
// the bits of the single-pair call on the same matrices and images (tests/test_gpu_direct_lists.py).
//   direct_list_pair_kernel          thread per entry: the record of matrices (P0, P1)
//   direct_list_lines[_gather]_kernel  thread per (entry, side, kappa): the line from the matrix's view record, the integral
//                                    through image I0 / I1
//   direct_segment_sum_kernel        workgroup per segment: its float64 sum in direct_sum_kernel's order
// The float64 value per entry is direct_reduce_kernel's (direct_kernel.hip), unchanged.
#include <hip/hip_runtime.h>
#include <math.h>

#include "ecc_direct_lines.h"

extern "C" hipError_t ecc_launch_direct_reduce(const EccDirectParams* p, hipStream_t stream);  // direct_kernel.hip

namespace {

__global__ __launch_bounds__(256) void direct_list_pair_kernel(EccDirectListParams q)
{
    const long long local = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (local >= q.b.count) return;
    direct_pair_record(q.b, local, q.idx4[4 * local], q.idx4[4 * local + 1]);
}

// direct_lines_gather_kernel with the view record from the matrix index and the pixels from the image index (no debug outputs)
__global__ __launch_bounds__(256) void direct_list_lines_gather_kernel(EccDirectListParams q)
{
    const EccDirectParams& p = q.b;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const long long pair = blockIdx.y;
    const int which = blockIdx.z;
    const EccDirectPair& r = p.pairs[pair];
    if (k >= r.n_lines) return;
    const EccDirectView& V = p.views[which ? r.j : r.i];
    const int image = q.idx4[4 * pair + 2 + which];
    float lf0, lf1, lf2, kf;
    direct_line_of(p, r, V, k, lf0, lf1, lf2, kf);
    const bool use_T = p.imagesT && fabsf(lf1) > fabsf(lf0);
    const float* img = (use_T ? p.imagesT : p.images) + (int64_t)image * p.image_stride;
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
}

// direct_lines_kernel likewise: the same tile orientation rule, walk and store
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void direct_list_lines_kernel(EccDirectListParams q)
{
    __shared__ ecc_slab::Shared sh;
    __shared__ float s_first_line[2];
    const EccDirectParams& p = q.b;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const long long pair = blockIdx.y;
    const int which = blockIdx.z;  // 0: the side of (P0, I0), 1: of (P1, I1)
    const EccDirectPair& r = p.pairs[pair];
    if ((int)(blockIdx.x * blockDim.x) >= r.n_lines) return;  // uniform: nothing below this line returns early
    const bool live = k < r.n_lines;
    const EccDirectView& V = p.views[which ? r.j : r.i];
    const int image = q.idx4[4 * pair + 2 + which];
    float lf0 = 0.f, lf1 = 1.f, lf2 = 0.f, kf = 0.f;
    if (live) direct_line_of(p, r, V, k, lf0, lf1, lf2, kf);
    ecc_slab::LineRun ln = direct_line_run(lf0, lf1, lf2, p.n_u, p.n_v);
    ln.active = ln.active && live;
    ecc_host::FbccInfo info;
    if (p.use_fbcc && live) {
        const float lf[3] = {lf0, lf1, lf2};
        ecc_host::fbcc_line_info(V.P, V.C, which ? r.H1 : r.H0, r.dvec, r.Eplane, lf, &info);
    }
    // tile orientation, walking direction and window slope from the workgroup's first line (uniform), as direct_lines_kernel
    if (threadIdx.x == 0) {
        s_first_line[0] = lf0;
        s_first_line[1] = lf1;
    }
    __syncthreads();
    const float n0 = ecc_slab::uni(s_first_line[0]), n1 = ecc_slab::uni(s_first_line[1]);
    const float* img = p.images + (int64_t)image * p.image_stride;
    const float* imgT = p.imagesT ? p.imagesT + (int64_t)image * p.image_stride : nullptr;
    const bool transp = imgT && fabsf(n1) > fabsf(n0);
    const float ds0 = transp ? n1 : -n0, df0 = transp ? -n0 : n1;
    const float sigma = ds0 >= 0.f ? 1.f : -1.f;
    const float beta0 = df0 / (fabsf(ds0) > 1e-6f ? ds0 : 1e-6f);
    float v;
    if (transp) v = direct_lines_body<true>(p, sh, img, imgT, ln, 0.5f * lf0, 0.5f * lf1, sigma, beta0, p.use_fbcc ? &info : nullptr);
    else v = direct_lines_body<false>(p, sh, img, imgT, ln, 0.5f * lf0, 0.5f * lf1, sigma, beta0, p.use_fbcc ? &info : nullptr);
    if (!live) return;
    if (!ln.active) v = 0.f;
    p.samples[((size_t)pair * 2 + which) * p.n_max + k] = v;
}

// sums[s] = the values [offsets[s], offsets[s + 1]) added as direct_sum_kernel adds a batch (an empty segment: 0.0)
__global__ __launch_bounds__(DIRECT_SUM_THREADS) void direct_segment_sum_kernel(const double* __restrict__ vals,
                                                                                const int64_t* __restrict__ offsets,
                                                                                double* __restrict__ sums)
{
    const int64_t first = offsets[blockIdx.x];
    const double tot = direct_block_sum(vals + first, offsets[blockIdx.x + 1] - first);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

}  // namespace

// One batch of a list: q->b.count <= 65535 entries; their float64 values go to q->b.pair_metric.
extern "C" hipError_t ecc_launch_direct_list_batch(const EccDirectListParams* q, hipStream_t stream)
{
    const EccDirectParams* p = &q->b;
    if (p->count <= 0) return hipSuccess;
    hipLaunchKernelGGL(direct_list_pair_kernel, dim3((unsigned)((p->count + 255) / 256)), dim3(256), 0, stream, *q);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    dim3 grid((p->n_max + 255) / 256, (unsigned)p->count, 2);
    if (p->n_u < DIRECT_SLAB_MIN_SIZE || p->n_v < DIRECT_SLAB_MIN_SIZE)
        hipLaunchKernelGGL(direct_list_lines_gather_kernel, grid, dim3(256), 0, stream, *q);
    else
        hipLaunchKernelGGL(direct_list_lines_kernel, grid, dim3(256), 0, stream, *q);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return ecc_launch_direct_reduce(p, stream);
}

extern "C" hipError_t ecc_launch_direct_segment_sums(const double* vals, const int64_t* offsets, int n_segments, double* sums,
                                                     hipStream_t stream)
{
    if (n_segments <= 0) return hipSuccess;
    hipLaunchKernelGGL(direct_segment_sum_kernel, dim3((unsigned)n_segments), dim3(DIRECT_SUM_THREADS), 0, stream, vals, offsets, sums);
    return hipGetLastError();
}
