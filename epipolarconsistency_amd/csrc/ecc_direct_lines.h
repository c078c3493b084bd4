// ecc_direct_lines.h -- MetricDirect's device pieces, stated once: the pair record, the line of a plane angle, the line's
// run through the image, the two accumulators, the band of a workgroup's lines, the walk of a workgroup's lines through the
// LDS tile and the float64 block sum.  direct_kernel.hip (all pairs in get_ij order, one pair) and direct_list_kernel.hip (index
// lists, where the matrix and the image of a pair's side are separate indices) build their kernels from them, so a line has one
// arithmetic.
// Include after ECC_SLAB_STAT is defined where statistics are wanted (direct_kernel.hip).
#ifndef ECC_DIRECT_LINES_H
#define ECC_DIRECT_LINES_H

#include <hip/hip_runtime.h>
#include <math.h>

#include "ecc_host_geometry.h"
#include "ecc_layout.h"
#include "ecc_sampling.h"
#include "ecc_slab_tile.h"

namespace {

// ref: EpipolarConsistencyDirect.cpp:84-117 + estimateAngularRange (EpipolarConsistency.cpp:49-59): the record of pair
// `local` of the batch from the view records of its two matrices; (i, j) are rows of p.views
__device__ __forceinline__ void direct_pair_record(const EccDirectParams& p, long long local, int i, int j)
{
    const EccDirectView& V0 = p.views[i];
    const EccDirectView& V1 = p.views[j];
    EccDirectPair r;
    r.i = i;
    r.j = j;
    double B[6];
    ecc_host::join_points(V0.C, V1.C, B);
    double radius = p.object_radius_mm;
    if (radius <= 0) radius = V0.radius > V1.radius ? V0.radius : V1.radius;  // ref: :88-90
    const double Pi = 3.14159265358979323846264338327950288419716939937510582;
    const double mom = sqrt(B[3] * B[3] + B[1] * B[1] + B[0] * B[0]);
    const double dir = sqrt(B[2] * B[2] + B[4] * B[4] + B[5] * B[5]);
    const double baseline_dist = mom / dir;
    // The range comes from the host where it is given: the device's asin may differ from the host's in the last bit, which
    // moves the grid's middle angle between 0 and 1e-16 and, for a detector with an integer diagonal, the line count by one.
    double k_first, k_second;
    if (p.k_second) {
        k_second = p.k_second[local];
        k_first = -k_second;
    } else if (baseline_dist <= radius) {
        k_first = -0.5 * Pi;
        k_second = 0.5 * Pi;
    } else {
        const double km = fabs(asin(radius / baseline_dist));
        k_first = -km;
        k_second = km;
    }
    double dkappa = p.dkappa;
    if (dkappa <= 0) {
        const double diag = sqrt((double)(p.n_u * p.n_u + p.n_v * p.n_v));
        dkappa = 0.5 * (k_second - k_first) / diag;
    }
    const double nl = (k_second - k_first) / dkappa;
    int n_lines = nl < 2147483000.0 ? (int)nl : 2147483000;
    if (!(nl >= 0)) n_lines = 0;            // NaN geometry (coincident source positions)
    if (p.user_kappas) n_lines = p.n_user_kappas;  // ref: :105-106: a non-empty `kappas` is taken as the grid
    if (n_lines > p.n_max) n_lines = p.n_max;  // cannot happen for the host's bound; keeps the stores in range
    r.k_first = k_first;
    r.dkappa = dkappa;
    r.n_lines = n_lines;
    const double origin3[4] = {0, 0, 0, 1};
    ecc_host::join_line_point(B, origin3, r.E0);
    ecc_host::join_line_point(B, r.E0, r.E90);
    const double n0 = sqrt(r.E0[0] * r.E0[0] + r.E0[1] * r.E0[1] + r.E0[2] * r.E0[2]);
    const double n90 = sqrt(r.E90[0] * r.E90[0] + r.E90[1] * r.E90[1] + r.E90[2] * r.E90[2]);
    for (int k = 0; k < 4; ++k) {
        r.E0[k] /= n0;
        r.E90[k] /= n90;
    }
    r.pad = 0;
    for (int k = 0; k < 9; ++k) r.H0[k] = r.H1[k] = 0;
    r.dvec[0] = -B[2]; r.dvec[1] = -B[4]; r.dvec[2] = -B[5];
    r.Eplane[0] = r.Eplane[1] = r.Eplane[2] = r.Eplane[3] = 0;
    if (p.use_fbcc) {
        // virtual detector plane spanned by the baseline direction and its moment, rectifying homographies
        // (ref: EpipolarConsistencyDirect.cpp:133-151)
        const double U[3] = {r.dvec[0] / dir, r.dvec[1] / dir, r.dvec[2] / dir};
        const double Vv[3] = {B[3] / mom, -B[1] / mom, B[0] / mom};
        ecc_host::cross3(U, Vv, r.Eplane);
        r.Eplane[3] = 0;
        ecc_host::RowQR f;
        for (int which = 0; which < 2; ++which) {
            const EccDirectView& W = which ? V1 : V0;
            for (int a = 0; a < 3; ++a) {
                for (int q = 0; q < 4; ++q) f.Q[a][q] = W.Q[4 * a + q];
                for (int b = 0; b < 3; ++b) f.L[a][b] = W.L[3 * a + b];
            }
            ecc_host::fbcc_homography(f, W.C, U, Vv, r.Eplane, which ? r.H1 : r.H0);
        }
    }
    p.pairs[local] = r;
}

// ---- line integrals (ref: EpipolarConsistencyDirect.cu:31-125, kernel_computeLineIntegrals) ---------------------
// One thread per epipolar line, stepping 0.4 px along the clipped line and accumulating bilinear samples sequentially
// in fp32 in the reference's order: the derivative form takes two samples half a pixel to either side of the line
// (sump, summ), the fan-beam form one weighted sample.  A workgroup is 256 ADJACENT lines of one pair's pencil in one
// image: they are nearly parallel (the epipole of a C-arm scan is far outside the image) and sweep a narrow band --
// exactly the Radon kernel's situation, so the band is walked slab by slab through the LDS tile of texel pairs of
// ecc_slab_tile.h instead of gathering from global memory (round 2: 64 lanes = 64 cache lines per load even with the
// transposed image copy).  Same arithmetic per sample (ecc_sampling.h), bit-identical results.
// The reference's launcher hands n_u over for both image sizes (:137); the evident intent (n_u, n_v) is implemented,
// identical for square images (oracle/ecc_oracle.c does the same).

// ref: EpipolarConsistencyDirect.cu:44-76 (line -> origin, direction, clipped parameter range)
__device__ __forceinline__ ecc_slab::LineRun direct_line_run(float l0, float l1, float l2, int n_u, int n_v)
{
    float o0 = -l2 * l0, o1 = -l2 * l1;
    const float d0 = l1, d1 = -l0;
    float ts[4] = {(1 - o0) / d0, (n_u - 1 - o0) / d0, (1 - o1) / d1, (n_v - 1 - o1) / d1};
    if ((double)(d0 * d0) < 1e-12) ts[0] = -(ts[1] = 1e10f);
    if ((double)(d1 * d1) < 1e-12) ts[2] = -(ts[3] = 1e10f);
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int i = 0; i < 3; i++)
            if (ts[i] > ts[i + 1]) {
                const float tmp = ts[i];
                ts[i] = ts[i + 1];
                ts[i + 1] = tmp;
            }
    const float t_min = ts[1], t_max = ts[2];
    const float u = o0 + t_min * d0, v = o1 + t_min * d1;
    const bool inside = (u <= n_u && v <= n_v && u >= 0 && v >= 0);  // else the reference returns 0 (:78-82)
    o0 += .5f;
    o1 += .5f;
    // a degenerate line (NaN) fails every loop condition; t_max - t_min <= the image diagonal otherwise
    return ecc_slab::LineRun{o0, o1, d0, d1, t_min, t_max, inside};
}

struct DirectDerivSums {  // ref: EpipolarConsistencyDirect.cu:103-113
    float sump = 0.f, summ = 0.f;
    __device__ __forceinline__ void add(float vA, float vB, float)
    {
        sump += vA * 0.4f;
        summ += vB * 0.4f;
    }
};
struct DirectFbccSum {  // ref: EpipolarConsistencyDirect.cu:87-101 (the fbcc_d branch): rectified by weighting, no derivative
    float sum = 0.f;
    ecc_host::FbccInfo fbcc;
    __device__ __forceinline__ void add(float vA, float, float t)
    {
        const float u_prime = fbcc.transform(t) - fbcc.t_prime_ak;
        const float fbcc_weight = fbcc.derivative(t) / sqrtf(u_prime * u_prime + fbcc.d_l_kappa_C_sq);
        sum += 0.4f * vA * fbcc_weight;
    }
};

// The band of a workgroup's lines from four workgroup-wide extremes: the smallest / largest fast coordinate of any line
// (both samples) at two reference slow coordinates.  Every line is linear in s, so between the references the band lies
// within the interpolated extremes -- whatever the lines are (no pencil assumption); tight when they do not cross
// inside the image.
struct LinearBand {
    float f0lo, f0hi, f1lo, f1hi, s0, inv_ds01, beta;
    __device__ __forceinline__ void operator()(float sa, float sb, float& gmin, float& gmax) const
    {
        const float la = (sa - s0) * inv_ds01, lb = (sb - s0) * inv_ds01;
        const float loa = f0lo + (f1lo - f0lo) * la - beta * sa, lob = f0lo + (f1lo - f0lo) * lb - beta * sb;
        const float hia = f0hi + (f1hi - f0hi) * la - beta * sa, hib = f0hi + (f1hi - f0hi) * lb - beta * sb;
        gmin = fminf(loa, lob);
        gmax = fmaxf(hia, hib);
    }
};

template <bool TRANSP>
__device__ __forceinline__ float direct_lines_body(const EccDirectParams& p, ecc_slab::Shared& sh, const float* img,
                                                   const float* imgT, ecc_slab::LineRun& ln, float lh0, float lh1, float sigma,
                                                   float beta0, const ecc_host::FbccInfo* fbcc)
{
    using namespace ecc_slab;
    const int W = p.n_u, H = p.n_v;
    const int Ns = TRANSP ? W : H;
    const float of = TRANSP ? ln.o1 : ln.o0, os = TRANSP ? ln.o0 : ln.o1;
    const float df = TRANSP ? ln.d1 : ln.d0, ds = TRANSP ? ln.d0 : ln.d1;
    const float hf = TRANSP ? lh1 : lh0, hs = TRANSP ? lh0 : lh1;  // the derivative pair's offset from the line
    BandFrame bf;
    bf.sigma = sigma;
    set_beta(bf, beta0);
    bf.marg = uni(.75f);
    const bool runs_with = ln.active && ds * sigma > .3f;  // (the walker's own rule)
    LinearBand band;
    band.s0 = -2.f;
    band.inv_ds01 = 1.f / ((float)Ns + 4.f);
    band.beta = bf.beta;
    {
        const float m = runs_with ? df / ds : 0.f;
        const float s1 = (float)Ns + 2.f;
        // the line itself at the two reference coordinates, widened by the derivative pair's offsets
        const float c = of - os * m;  // f = c + m s
        const float w = fbcc ? 0.f : fabsf(hf) + fabsf(hs * m);
        float lo0 = runs_with ? c + m * band.s0 - w : FLT_MAX, hi0 = runs_with ? c + m * band.s0 + w : -FLT_MAX;
        float lo1 = runs_with ? c + m * s1 - w : FLT_MAX, hi1 = runs_with ? c + m * s1 + w : -FLT_MAX;
        block_min_max(sh, lo0, hi0);
        block_min_max(sh, lo1, hi1);
        band.f0lo = lo0; band.f0hi = hi0; band.f1lo = lo1; band.f1hi = hi1;
    }
    const float* src = TRANSP ? imgT : img;
    if (fbcc) {
        DirectFbccSum acc;
        acc.fbcc = *fbcc;
        walk<TRANSP, false, false, false>(sh, img, W, H, src, bf, band, ln, 0.f, 0.f, 0.f, 0.f, 0.4f, acc);
        return acc.sum;
    }
    DirectDerivSums acc;
    walk<TRANSP, true, true, false>(sh, img, W, H, src, bf, band, ln, lh0, lh1, -lh0, -lh1, 0.4f, acc);
    return acc.sump - acc.summ;
}

// ref: EpipolarConsistencyDirect.cpp:113-117 (kappa grid, float) and :49-63 (the line of plane kappa), normalised
__device__ __forceinline__ void direct_line_of(const EccDirectParams& p, const EccDirectPair& r, const EccDirectView& V, int k,
                                               float& lf0, float& lf1, float& lf2, float& kf)
{
    kf = p.user_kappas ? p.user_kappas[k] : (float)(r.k_first + r.dkappa * k);
    const double kappa = kf, c = cos(kappa), s = sin(kappa);
    double E[4], l[3];
    for (int q = 0; q < 4; ++q) E[q] = c * r.E0[q] + s * r.E90[q];
    ecc_host::RowQR f;
    for (int a = 0; a < 3; ++a) {
        for (int q = 0; q < 4; ++q) f.Q[a][q] = V.Q[4 * a + q];
        for (int b = 0; b < 3; ++b) f.L[a][b] = V.L[3 * a + b];
    }
    ecc_host::plane_to_line(f, E, l);
    const double nn = sqrt(l[0] * l[0] + l[1] * l[1]);
    lf0 = (float)(l[0] / nn);
    lf1 = (float)(l[1] / nn);
    lf2 = (float)(l[2] / nn);
}

// Small images (either side below DIRECT_SLAB_MIN_SIZE pixels): 256 adjacent lines of a pencil are a third of such an
// image wide, the slabs of their band get short and wide, and the whole image is cache-resident anyway -- one thread per
// line gathering from global memory (round 1-2's kernel) is faster there (256^2: 0.33 against 0.52 ms per 28-pair
// evaluation; 512^2: 1.77 against 0.91).  The lanes of a wave are adjacent lines at the same step: for near-horizontal
// lines they differ in v, so those read the transposed copy.  Same arithmetic, same bits as the slab kernel.
constexpr int DIRECT_SLAB_MIN_SIZE = 384;

// The float64 sum of `count` values by one workgroup of DIRECT_SUM_THREADS in a fixed order: strided partials per thread, the
// shuffle tree per wave, then the wave partials in index order.  A fixed function of the values; thread 0 holds the result.
constexpr int DIRECT_SUM_THREADS = 1024;
__device__ __forceinline__ double direct_block_sum(const double* __restrict__ vals, long long count)
{
    __shared__ double s[DIRECT_SUM_THREADS / 64];
    double acc = 0.0;
    for (long long k = threadIdx.x; k < count; k += DIRECT_SUM_THREADS) acc += vals[k];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
    __syncthreads();
    double tot = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < DIRECT_SUM_THREADS / 64; w++) tot += s[w];
    return tot;
}

}  // namespace

#endif
