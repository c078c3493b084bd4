// view_hessian_kernel.hip -- the per-view quadratic form as a matrix: three moment blocks per pair, and their assembly (gfx950).
//
// A metric over K * n Radon intermediates, channel-major, and K * n coefficients a[c * n + i] as in view_coeff_kernel.hip: for the
// pair i < j with the signed samples v0_c, v1_c of channel c in view i and in view j, and w = K0[6] dkappa,
//   P00[c][d] = w sum_s v0_c v0_d,   P11[c][d] = w sum_s v1_c v1_d,   P01[c][d] = -w sum_s v0_c v1_d      (s: the pair's +- samples)
// so that the pair's value at (a_i, a_j) is a_i^T P00 a_i + a_j^T P11 a_j + 2 a_i^T P01 a_j.  The form is wanted near its minimum,
// where it is a small difference of large moments, so nothing is rounded in float32 behind the samples: a sample is converted to
// binary64 once, every product of two samples is exact in binary64 (24 + 24 bits), and an entry is acc = fma(x, y, acc) for the +
// and then the - sample of a kappa step, per lane in float64 in pairs_coeff_kernel's trip order, reduced by the same wave tree,
// multiplied by w = (double)K0[6] * (double)dkappa by lane 0 and stored as float64.
// pairs_moments_kernel<DERIV, NC> runs on form_loop_poly and form_loop_exact of ecc_pair_forms.h; its choice of loop
// (moment_accumulate: no pair weight inside the loops), the kernel body and the reference kernels stay here.  MomentForm's trip gathers
// NC footprints at each of the four taps (the float32 sample values of pairs_coeff_kernel), converts them to binary64 and adds the T2
// exact products.  The polynomial loops see unsigned samples u with the fold signs s0, s1 of the two views: P00 and P11 need no sign
// (s^2 = 1), and -v0 v1 = -s0 s1 u0 u1 = rel_sign u0 u1 with the frame's rel_sign, applied to the lane's sums of u0 u1 when the
// loop ends (poly_end) -- an exact negation, which commutes with every rounding after it.  The exact and the reference loop see signed samples
// and accumulate fma(-v0, v1, acc).  T2 = NC (NC + 1) + NC^2 columns: P00's upper triangle in the Gram form's entry order, P11's
// upper triangle, P01 row-major.
// assemble_view_hessian_kernel writes H (index k = c * n + i) from the columns: off-diagonal blocks and their transposed twins as
// P01 / N, diagonal blocks as sums over a view's n - 1 pairs in sum_view_terms_kernel's order (sum_kernel.hip).  No atomics.
#include <hip/hip_runtime.h>
#include <float.h>

#include "ecc_layout.h"
#include "ecc_pair_forms.h"
#include "ecc_sum_order.h"

namespace {

constexpr int tri_entries(int nc) { return nc * (nc + 1) / 2; }
constexpr int moment_entries(int nc) { return 2 * tri_entries(nc) + nc * nc; }

// acc[t] = fma(x, y, acc[t]) for the + and then the - sample of every entry, in the order of the columns.  SIGNED: the samples
// carry their signs, and P01 accumulates -v0 v1 (the negated factor is exact).
template <int NC, bool SIGNED>
__device__ __forceinline__ void moment_add(double (&acc)[moment_entries(NC)], const double (&x0p)[NC], const double (&x0m)[NC],
                                           const double (&x1p)[NC], const double (&x1m)[NC])
{
    int t = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int d = c; d < NC; ++d, ++t) acc[t] = fma(x0m[c], x0m[d], fma(x0p[c], x0p[d], acc[t]));
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int d = c; d < NC; ++d, ++t) acc[t] = fma(x1m[c], x1m[d], fma(x1p[c], x1p[d], acc[t]));
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int d = 0; d < NC; ++d, ++t)
            acc[t] = SIGNED ? fma(-x0m[c], x1m[d], fma(-x0p[c], x1p[d], acc[t])) : fma(x0m[c], x1m[d], fma(x0p[c], x1p[d], acc[t]));
}

// the trips of the polynomial and the exact loops (form_loop_poly, form_loop_exact, ecc_pair_forms.h): NC gathers at each of the four
// taps, every sample converted to binary64 once, the T2 exact products
template <int NC>
struct MomentForm : ChannelForm<EccViewMomentParams> {
    double (&acc)[moment_entries(NC)];

    __device__ __forceinline__ MomentForm(const EccViewMomentParams& g, double (&acc)[moment_entries(NC)]) : ChannelForm(g), acc(acc) {}

    // unsigned samples: P01 accumulates u0 u1, signed when the loop ends
    __device__ __forceinline__ void poly_trip(const SlabView sv0, const SlabView sv1, const SampleTap t0p, const SampleTap t1p,
                                              const SampleTap t0m, const SampleTap t1m, float, float)
    {
        double x0p[NC], x1p[NC], x0m[NC], x1m[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const GlobalBytes o0 = sv0.origin + chan * c, o1 = sv1.origin + chan * c;
            x0p[c] = (double)sample_tap_value(o0, t0p);
            x1p[c] = (double)sample_tap_value(o1, t1p);
            x0m[c] = (double)sample_tap_value(o0, t0m);
            x1m[c] = (double)sample_tap_value(o1, t1m);
        }
        moment_add<NC, false>(acc, x0p, x0m, x1p, x1m);
    }

    // -v0 v1 = -s0 s1 u0 u1 = rel_sign u0 u1: rel_sign = -1 negates the lane's P01 sums (exact; wave-uniform)
    __device__ __forceinline__ void poly_end(float rel_sign)
    {
        if (rel_sign < 0.f) {
#pragma unroll
            for (int t = 2 * tri_entries(NC); t < moment_entries(NC); ++t) acc[t] = -acc[t];
        }
    }

    template <bool DERIV, int PITCH4>
    __device__ __forceinline__ void exact_trip(const SlabView sv0, const SlabView sv1, const LineTap t0p, const LineTap t1p, const LineTap t0m,
                                               const LineTap t1m, float, float)
    {
        const unsigned o0p = line_tap_offset(t0p, sv0), o1p = line_tap_offset(t1p, sv1);
        const unsigned o0m = line_tap_offset(t0m, sv0), o1m = line_tap_offset(t1m, sv1);
        double x0p[NC], x1p[NC], x0m[NC], x1m[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const GlobalBytes o0 = sv0.origin + chan * c, o1 = sv1.origin + chan * c;
            x0p[c] = (double)line_tap_finish<DERIV>(line_footprint(o0, o0p), t0p);
            x1p[c] = (double)line_tap_finish<DERIV>(line_footprint(o1, o1p), t1p);
            x0m[c] = (double)line_tap_finish<DERIV>(line_footprint(o0, o0m), t0m);
            x1m[c] = (double)line_tap_finish<DERIV>(line_footprint(o1, o1m), t1m);
        }
        moment_add<NC, true>(acc, x0p, x0m, x1p, x1m);
    }
};

// form_accumulate (ecc_pair_forms.h) without the pair weight: the same choice of loop for the same record, made by the same helpers.
// (Kept here: on form_accumulate the four plain-data kernels change their instruction streams, see CHANGELOG.)
template <bool DERIV, int NC>
__device__ __forceinline__ void moment_accumulate(const EccPairParams& p, const EccViewMomentParams& g, const EccPairRecord* __restrict__ rec,
                                                  int iD0, int iD1, int lane, double (&acc)[moment_entries(NC)])
{
    const unsigned pitch4 = (unsigned)p.pitch * 8u;
    const SlabView sv0 = {(GlobalBytes)p.dtrs[iD0], pitch4};
    const SlabView sv1 = {(GlobalBytes)p.dtrs[iD1], pitch4};
    MomentForm<NC> form(g, acc);
    const float n_alpha_f = (float)p.n_alpha, n_t_f = (float)p.n_t;
    const float pitch4_f = (float)pitch4;
    const float kappa_max = uniformf(rec->K1[7]);

    const bool reduce = kappa_max > 0.785398163397448f;  // wave-uniform
    const int poly_raw = __builtin_amdgcn_readfirstlane(rec->poly_ok);
    const int poly_ok = poly_raw & ~1;
    const bool in_range = (poly_raw & 1) != 0;
    int k_first = lane;
    if (poly_ok) {
        const float kappa_fit = ecc_kappa_fit(kappa_max), dkappa = uniformf(rec->K1[6]);  // (no weight in the loops: lane 0 applies it)
        poly_loop_dispatch(p.wide_offsets != 0, pitch4, poly_ok, in_range, [&](auto P4, auto DEG, auto NOCL) {
            k_first = form_loop_poly<DERIV, decltype(P4)::value, decltype(DEG)::value, decltype(NOCL)::value>(
                form, lane, p.k_limit, rec, dkappa, kappa_fit, 0.f, sv0, sv1, n_alpha_f, n_t_f, pitch4_f);
        });
        if (!(kappa_fit < kappa_max)) return;  // wave-uniform: the polynomials covered the whole range (the normal case)
        asm volatile("" : "+s"(rec));  // what follows is read from the record afterwards (as in pair_accumulate)
    }
    float K0[8], K1[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        K0[i] = uniformf(rec->K0[i]);
        K1[i] = uniformf(rec->K1[i]);
    }
    const float dist_scale = n_t_f / p.range_t, dist_bias = fmaf(0.5f, n_t_f, 0.5f);
    exact_loop_dispatch(p, reduce, pitch4, sv0, sv1, iD0, iD1, [&](auto REDUCE, auto P4, const SlabView v0, const SlabView v1) {
        form_loop_exact<DERIV, decltype(REDUCE)::value, decltype(P4)::value>(form, k_first, p.k_limit, K0, K1, v0, v1, n_alpha_f, n_t_f,
                                                                           dist_scale, dist_bias, pitch4_f);
    });
}

// the pair's weight in binary64 from its two float32 factors (exact: 24 + 24 bits)
__device__ __forceinline__ double pair_weight(const EccPairRecord* __restrict__ rec)
{
    return (double)uniformf(rec->K0[6]) * (double)uniformf(rec->K1[6]);
}

// One wave per pair, on pairs_kernel's workgroup -> pairs mapping (main_pair_of_wave, ecc_pairs_device.h).
// Registers: the 4 NC gathers of a kappa step as in pairs_coeff_kernel, the 4 NC samples as float64 and
// 2 T2 accumulator registers; tests/test_view_hessian_abi.py pins the plan and what was built.
template <bool DERIV, int NC>
__global__ __launch_bounds__(PK_MAIN_THREADS) void pairs_moments_kernel(EccPairParams p, EccViewMomentParams g)
{
    constexpr int T2 = moment_entries(NC);
    const int lane = threadIdx.x & 63;
    long long local;
    if (!main_pair_of_wave(p.count, local)) return;
    local = uniform_index(local);
    const EccPairRecord* __restrict__ rec = p.records + local;
    const int iD0 = __builtin_amdgcn_readfirstlane(rec->iD0), iD1 = __builtin_amdgcn_readfirstlane(rec->iD1);
    double acc[T2];
#pragma unroll
    for (int t = 0; t < T2; ++t) acc[t] = 0.0;
    moment_accumulate<DERIV, NC>(p, g, rec, iD0, iD1, lane, acc);
#pragma unroll
    for (int t = 0; t < T2; ++t) ecc_sum::wave_sum(acc[t]);
    if (lane == 0) {
        const double w = pair_weight(rec);
#pragma unroll
        for (int t = 0; t < T2; ++t) g.values[(long long)t * g.col_stride + local] = acc[t] * w;
    }
}

// ---- ECC_SAMPLING_REFERENCE -------------------------------------------------------------------------
// reference_loop<false> (ecc_pairs_device.h) for NC channels: the moment products on the signed samples.
template <int NC>
__device__ __forceinline__ void moment_reference_loop(const EccPairParams& p, const float (&K0)[8], const float (&K1)[8],
                                                      const GlobalFloats (&d0)[NC], const GlobalFloats (&d1)[NC], int first_k, int stride,
                                                      double (&acc)[moment_entries(NC)])
{
    const float dkappa = K1[6], kappa_max = K1[7];
    const bool deriv = p.is_derivative != 0;
    for (int k = first_k; k < p.k_limit; k += stride) {
        const float kappa = dkappa * 0.5f + dkappa * k;  // ref: ...RadonIntermediate.cu:259
        if (kappa >= kappa_max) break;
        double sk, ck;
        sincos((double)kappa, &sk, &ck);
        float x0 = (float)ck;
        const float x1 = (float)sk;
        const PlainTap t0p = plain_line_tap(K0, x0, x1, p.range_t), t1p = plain_line_tap(K1, x0, x1, p.range_t);
        x0 *= -1;  // ref: ...RadonIntermediate.cu:106
        const PlainTap t0m = plain_line_tap(K0, x0, x1, p.range_t), t1m = plain_line_tap(K1, x0, x1, p.range_t);
        double x0p[NC], x1p[NC], x0m[NC], x1m[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            x0p[c] = (double)plain_tap_value(t0p, d0[c], p.pitch, p.n_alpha, p.n_t, deriv);
            x1p[c] = (double)plain_tap_value(t1p, d1[c], p.pitch, p.n_alpha, p.n_t, deriv);
            x0m[c] = (double)plain_tap_value(t0m, d0[c], p.pitch, p.n_alpha, p.n_t, deriv);
            x1m[c] = (double)plain_tap_value(t1m, d1[c], p.pitch, p.n_alpha, p.n_t, deriv);
        }
        moment_add<NC, true>(acc, x0p, x0m, x1p, x1m);
    }
}

// pairs_reference_kernel<false, SPLIT> for NC channels with the moment products: SPLIT = 1 one wave per pair, SPLIT = 4 the
// workgroup's four waves on one pair with the wave sums added in wave order (the grouping the metric's mode fixes).
template <int NC, int SPLIT>
__global__ __launch_bounds__(PK_THREADS) void pairs_moments_reference_kernel(EccPairParams p, EccViewMomentParams g)
{
    static_assert(SPLIT == 1 || SPLIT == PK_THREADS / 64, "one pair per wave or per workgroup");
    constexpr int T2 = moment_entries(NC);
    __shared__ double part[T2][PK_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long local = SPLIT == 1 ? (long long)blockIdx.x * 4 + wave : (long long)blockIdx.x;
    if (local >= p.count) return;  // SPLIT > 1: uniform over the workgroup
    local = uniform_index(local);
    const EccPairRecord* __restrict__ rec = p.records + local;
    float K0[8], K1[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        K0[i] = uniformf(rec->K0[i]);
        K1[i] = uniformf(rec->K1[i]);
    }
    const int iD0 = __builtin_amdgcn_readfirstlane(rec->iD0), iD1 = __builtin_amdgcn_readfirstlane(rec->iD1);
    GlobalFloats d0[NC], d1[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        d0[c] = (GlobalFloats)p.slabs[(long long)c * p.n_views + iD0];
        d1[c] = (GlobalFloats)p.slabs[(long long)c * p.n_views + iD1];
    }
    double acc[T2];
#pragma unroll
    for (int t = 0; t < T2; ++t) acc[t] = 0.0;
    moment_reference_loop<NC>(p, K0, K1, d0, d1, SPLIT == 1 ? lane : (int)threadIdx.x, 64 * SPLIT, acc);
#pragma unroll
    for (int t = 0; t < T2; ++t) ecc_sum::wave_sum(acc[t]);
    if (SPLIT > 1) {  // wave sums -> wave 0, added in wave order (add_wave_partials)
        if (lane == 0) {
#pragma unroll
            for (int t = 0; t < T2; ++t) part[t][wave] = acc[t];
        }
        __syncthreads();
        if (wave != 0) return;
#pragma unroll
        for (int t = 0; t < T2; ++t) {
            double sum = part[t][0];
#pragma unroll
            for (int w = 1; w < PK_THREADS / 64; ++w) sum += part[t][w];
            acc[t] = sum;
        }
    }
    if (lane == 0) {
        const double w = (double)K0[6] * (double)K1[6];
#pragma unroll
        for (int t = 0; t < T2; ++t) g.values[(long long)t * g.col_stride + local] = acc[t] * w;
    }
}

template <int NC>
hipError_t launch_moments_nc(const EccPairParams& p, const EccViewMomentParams& g, hipStream_t stream)
{
    return launch_pair_form(p, g, stream, pairs_moments_reference_kernel<NC, 4>, pairs_moments_reference_kernel<NC, 1>,
                            pairs_moments_kernel<true, NC>, pairs_moments_kernel<false, NC>);
}

// H from the columns.  Workgroup (view v, entry e) of n_views x (K (K + 1) / 2 + K^2):
//   e < K (K + 1) / 2, the entry (c <= d) of v's diagonal block: the n - 1 terms of the pairs that contain v -- P00 of the pair
//     (v, w) where v is the smaller index, P11 of the pair (w, v) where it is the larger -- added in sum_view_terms_kernel's order
//     (partners ascending, thread t its terms t, t + THREADS, ... in float64 to 0.0, the wave tree, the wave sums in wave order),
//     divided by N and written to H[(c,v),(d,v)] and H[(d,v),(c,v)];
//   else the entry (c, d) of P01: for every partner w > v, P01 / N to H[(c,v),(d,w)] and to its twin H[(d,w),(c,v)].
// Every entry of H is written exactly once, by one thread: no atomics, the same bits on every run, H == H^T bit for bit.
__global__ __launch_bounds__(ecc_sum::THREADS) void assemble_view_hessian_kernel(const double* __restrict__ values, long long col_stride,
                                                                                 int n_views, int n_channels, double* __restrict__ H)
{
    __shared__ double s[ecc_sum::WAVES];
    const int v = blockIdx.x, K = n_channels, tri = K * (K + 1) / 2;
    const long long n = n_views, dim = n * K;
    const double N = (double)(n * (n - 1) / 2);
    int e = blockIdx.y;  // (uniform over the workgroup, and so is the branch below)
    if (e < tri) {
        int c = 0;
        while (e >= K - c) e -= K - c, ++c;
        const int d = c + e;
        const double* __restrict__ p00 = values + (long long)blockIdx.y * col_stride;
        const double* __restrict__ p11 = values + (long long)(tri + blockIdx.y) * col_stride;
        double acc = 0.0;
        for (int u = threadIdx.x; u < n_views - 1; u += ecc_sum::THREADS) {
            const int w = u < v ? u : u + 1;
            const long long lo = w < v ? w : v, hi = w < v ? v : w;
            const long long pair = lo * n - lo * (lo + 1) / 2 + (hi - lo - 1);  // get_ij order (ecc_layout.h)
            acc += w < v ? p11[pair] : p00[pair];
        }
        ecc_sum::stage_wave_sums(acc, s);
        if (threadIdx.x == 0) {
            const double h = ecc_sum::waves_in_order(s) / N;
            H[(c * n + v) * dim + (d * n + v)] = h;
            if (d != c) H[(d * n + v) * dim + (c * n + v)] = h;
        }
    } else {
        e -= tri;
        const int c = e / K, d = e % K;
        const double* __restrict__ p01 = values + (long long)(2 * tri + e) * col_stride;
        const long long first = (long long)v * n - (long long)v * (v + 1) / 2;  // the pair (v, v + 1)
        for (long long w = v + 1 + threadIdx.x; w < n; w += ecc_sum::THREADS) {
            const double h = p01[first + (w - v - 1)] / N;
            H[(c * n + v) * dim + (d * n + w)] = h;
            H[(d * n + w) * dim + (c * n + v)] = h;
        }
    }
}

}  // namespace

// The T2 = K (K + 1) + K^2 float64 entries of every pair of the all-pairs launch p (records of ecc_launch_k01 for the same
// parameters, earlier on the same stream; first = 0, no index list, no slots) into g->values.  n_channels in [1, ECC_GRAM_CHANNELS_MAX].
extern "C" hipError_t ecc_launch_pairs_moments(const EccPairParams* p, const EccViewMomentParams* g, int n_channels, hipStream_t stream)
{
    if (p->count <= 0) return hipSuccess;
    if (p->use_corr || p->indices || p->record_slots || p->skip_enabled || !g->values || g->col_stride < p->count || (g->col_stride & 3))
        return hipErrorInvalidValue;
    switch (n_channels) {
    case 1: return launch_moments_nc<1>(*p, *g, stream);
    case 2: return launch_moments_nc<2>(*p, *g, stream);
    case 3: return launch_moments_nc<3>(*p, *g, stream);
    case 4: return launch_moments_nc<4>(*p, *g, stream);
    default: return hipErrorInvalidValue;
    }
}

// H_d: (n_views * n_channels)^2 doubles, every one written.  values_d: the T2 columns of ecc_launch_pairs_moments for all
// n_views (n_views - 1) / 2 pairs.
extern "C" hipError_t ecc_launch_assemble_view_hessian(const double* values_d, long long col_stride, int n_views, int n_channels, double* H_d,
                                                       hipStream_t stream)
{
    if (n_views < 2 || n_channels < 1 || n_channels > ECC_GRAM_CHANNELS_MAX || !values_d || !H_d ||
        col_stride < (long long)n_views * (n_views - 1) / 2)
        return hipErrorInvalidValue;
    const int entries = n_channels * (n_channels + 1) / 2 + n_channels * n_channels;
    hipLaunchKernelGGL(assemble_view_hessian_kernel, dim3((unsigned)n_views, (unsigned)entries), dim3(ecc_sum::THREADS), 0, stream, values_d,
                       col_stride, n_views, n_channels, H_d);
    return hipGetLastError();
}
