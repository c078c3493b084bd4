// view_coeff_kernel.hip -- the metric of per-view channel coefficients and its gradient terms (gfx950).
//
// A metric over K * n Radon intermediates, channel-major (channel c of view i is dtr c * n + i), and K * n coefficients
// a[c * n + i]: the corrected intermediate of view i is sum_c a_c,i D_c,i, so for the pair i < j every redundant sample is
//   delta = sum_c a_c,i v0_c - sum_c a_c,j v1_c        (v0_c, v1_c: the signed samples of channel c in view i and in view j)
// at the sample positions, fold signs, kappa range and weights of pairs_kernel's evaluation, and per pair
//   value = sum_kappa (delta+^2 + delta-^2) K0[6] dkappa,
//   h0[c] = sum_kappa (delta+ v0+_c + delta- v0-_c) K0[6] dkappa = 1/2 d value / d a_c,i,
//   h1[c] = -sum_kappa (delta+ v1+_c + delta- v1-_c) K0[6] dkappa = 1/2 d value / d a_c,j.
// pairs_coeff_kernel<DERIV, NC> is pairs_gram_kernel (gram_kernel.hip) with other products behind the same 4 NC gathers: one wave per
// pair, the record and the pair's 2 NC coefficients in scalar registers, the same dispatch over the record's degree and the slab
// size, per-lane float64 sums in the same trip order, the same wave tree.  A side's combined sample is formed in channel order,
// s = a_0 v_0, then s = fmaf(a_c, v_c, s); the two differences and the value term are pairs_kernel's expressions:
//   polynomial loops   fmaf(dp, dp, dm * dm) * w06_dkappa       (unsigned samples; the folds' relative sign in the differences)
//   exact loop         ((dp * dp + dm * dm) * K0[6]) * dkappa   (signed samples)
//   reference loop     the same expression on sample_line_plain's samples
// so with one channel and every coefficient 1.0 (1.0f * v is v) the value column has the bits of pairs_kernel.  The gradient terms
// are the same expressions with the second factor exchanged for a sample.  Sign of h1: with unsigned samples u and fold signs s0, s1
// the true difference is s0 (u0 - s0 s1 u1) = s0 dp, and its derivative by a_c,j is -s1 u1_c; the product is -s0 s1 dp u1_c =
// rel_sign dp u1_c -- the relative sign the differences already carry, folded into the wave-uniform weight (an exact negation).
// The 1 + 2 NC columns -- value, h0[0 .. NC), h1[0 .. NC) -- are stored like the Gram form's; the value column is summed by
// sum_gram_kernel, the gradient columns per (view, channel) by sum_view_terms_kernel (sum_kernel.hip).
#include <hip/hip_runtime.h>
#include <float.h>

#include "ecc_layout.h"
#include "ecc_pairs_device.h"

namespace {

constexpr int coeff_entries(int nc) { return 1 + 2 * nc; }

// s = a[0] v[0], then fmaf(a[c], v[c], s) in channel order
template <int NC>
__device__ __forceinline__ float combine_channels(const float (&a)[NC], const float (&v)[NC])
{
    float s = a[0] * v[0];
#pragma unroll
    for (int c = 1; c < NC; ++c) s = fmaf(a[c], v[c], s);
    return s;
}

// the pair's coefficients: a0[c] = a[c * n + iD0], a1[c] = a[c * n + iD1] (wave-uniform: scalar loads)
template <int NC>
__device__ __forceinline__ void pair_coefficients(const float* __restrict__ coeffs, int n_views, int iD0, int iD1, float (&a0)[NC],
                                                  float (&a1)[NC])
{
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        a0[c] = uniformf(coeffs[(long long)c * n_views + iD0]);
        a1[c] = uniformf(coeffs[(long long)c * n_views + iD1]);
    }
}

// gram_loop_poly (gram_kernel.hip) with the coefficient products: returns the lane's first sample index past the fit's range.
// chan: bytes from a view's copy to the same view's copy of the next channel (wave-uniform).
template <bool DERIV, int NC, int PITCH4, int DEG, bool NOCLAMP>
__device__ __forceinline__ int coeff_loop_poly(int lane, int k_limit, const EccPairRecord* __restrict__ rec, float dkappa,
                                               float kappa_fit, float w06, const SlabView sv0, const SlabView sv1, long long chan,
                                               float n_alpha_f, float n_t_f, float pitch4_f, const float (&a0)[NC], const float (&a1)[NC],
                                               double (&acc)[coeff_entries(NC)])
{
    float ca[2][ECC_POLY_DEG + 3], cd[2][ECC_POLY_DEG + 2];
    unsigned fold[2];
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        fold[v] = (unsigned)__builtin_amdgcn_readfirstlane((int)rec->fold[v]);
#pragma unroll
        for (int k = 0; k <= ECC_POLY_DEG + 1; ++k) {
            if (k > DEG && k <= ECC_POLY_DEG) continue;
            ca[v][k] = uniformf(rec->ca[v][k]);
            cd[v][k] = uniformf(rec->cd[v][k]);
        }
        ca[v][ECC_POLY_DEG + 2] = uniformf(rec->ca[v][ECC_POLY_DEG + 2]);
    }
    const float xs = uniformf(rec->x_scale);
    const float xa_max = n_alpha_f + 0.5f;
    const float rel_sign = (DERIV && ((fold[0] ^ fold[1]) & 0x80000000u)) ? 1.0f : -1.0f;  // see kappa_loop_poly
    const float w06_dkappa = w06 * dkappa;
    const float w1 = rel_sign * w06_dkappa;  // view j's terms: the weight with the relative sign (header comment)
    float kf = (float)lane;
    int k = lane;
    for (; k < k_limit; k += 64, kf += 64.f) {
        const float kappa = dkappa * 0.5f + dkappa * kf;  // ref: ...RadonIntermediate.cu:259 (same fp32 ops)
        if (kappa >= kappa_fit) break;
        const float x = kappa * xs, z = x * x;
        float xa0p, xa0m, yd0p, yd0m, xa1p, xa1m, yd1p, yd1m;
        poly_pm<DEG>(ca[0], ca[0][ECC_POLY_DEG + 1], ca[0][ECC_POLY_DEG + 2], false, x, z, xa0p, xa0m);
        poly_pm<DEG>(cd[0], cd[0][ECC_POLY_DEG + 1], 0.f, true, x, z, yd0p, yd0m);
        poly_pm<DEG>(ca[1], ca[1][ECC_POLY_DEG + 1], ca[1][ECC_POLY_DEG + 2], false, x, z, xa1p, xa1m);
        poly_pm<DEG>(cd[1], cd[1][ECC_POLY_DEG + 1], 0.f, true, x, z, yd1p, yd1m);
        const SampleTap t0p = sample_tap<PITCH4, NOCLAMP>(xa0p, yd0p, sv0, n_t_f, pitch4_f, xa_max);
        const SampleTap t1p = sample_tap<PITCH4, NOCLAMP>(xa1p, yd1p, sv1, n_t_f, pitch4_f, xa_max);
        const SampleTap t0m = sample_tap<PITCH4, NOCLAMP>(xa0m, yd0m, sv0, n_t_f, pitch4_f, xa_max);
        const SampleTap t1m = sample_tap<PITCH4, NOCLAMP>(xa1m, yd1m, sv1, n_t_f, pitch4_f, xa_max);
        float v0p[NC], v1p[NC], v0m[NC], v1m[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const GlobalBytes o0 = sv0.origin + chan * c, o1 = sv1.origin + chan * c;
            v0p[c] = sample_tap_value(o0, t0p);
            v1p[c] = sample_tap_value(o1, t1p);
            v0m[c] = sample_tap_value(o0, t0m);
            v1m[c] = sample_tap_value(o1, t1m);
        }
        const float dp = fmaf(combine_channels<NC>(a1, v1p), rel_sign, combine_channels<NC>(a0, v0p));
        const float dm = fmaf(combine_channels<NC>(a1, v1m), rel_sign, combine_channels<NC>(a0, v0m));
        acc[0] += (double)(fmaf(dp, dp, dm * dm) * w06_dkappa);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            acc[1 + c] += (double)(fmaf(dp, v0p[c], dm * v0m[c]) * w06_dkappa);
            acc[1 + NC + c] += (double)(fmaf(dp, v1p[c], dm * v1m[c]) * w1);
        }
    }
    return k;
}

// gram_loop_exact (gram_kernel.hip) with the coefficient products: kappa_step's expressions on the signed samples.
template <bool DERIV, int NC, bool REDUCE, int PITCH4>
__device__ __forceinline__ void coeff_loop_exact(int k_first, int k_limit, const float (&K0)[8], const float (&K1)[8], const SlabView sv0,
                                                 const SlabView sv1, long long chan, float n_alpha_f, float n_t_f, float dist_scale,
                                                 float dist_bias, float pitch4_f, const float (&a0)[NC], const float (&a1)[NC],
                                                 double (&acc)[coeff_entries(NC)])
{
    const float dkappa = K1[6], kappa_max = K1[7];
    for (int k = k_first; k < k_limit; k += 64) {
        const float kappa = dkappa * 0.5f + dkappa * k;  // ref: ...RadonIntermediate.cu:259 (same fp32 ops)
        if (kappa >= kappa_max) return;
        float sn, cs;
        sincos_quadrant<REDUCE>(kappa, sn, cs);
        const float a00 = K0[0] * cs, a01 = K0[1] * cs, a02 = K0[2] * cs;
        const float b00 = K0[3] * sn, b01 = K0[4] * sn, b02 = K0[5] * sn;
        const float a10 = K1[0] * cs, a11 = K1[1] * cs, a12 = K1[2] * cs;
        const float b10 = K1[3] * sn, b11 = K1[4] * sn, b12 = K1[5] * sn;
        const LineTap t0p = sample_line_prep<PITCH4>(b00 + a00, b01 + a01, b02 + a02, sv0, n_alpha_f, n_t_f, dist_scale, dist_bias, pitch4_f);
        const LineTap t1p = sample_line_prep<PITCH4>(b10 + a10, b11 + a11, b12 + a12, sv1, n_alpha_f, n_t_f, dist_scale, dist_bias, pitch4_f);
        const LineTap t0m = sample_line_prep<PITCH4>(b00 - a00, b01 - a01, b02 - a02, sv0, n_alpha_f, n_t_f, dist_scale, dist_bias, pitch4_f);
        const LineTap t1m = sample_line_prep<PITCH4>(b10 - a10, b11 - a11, b12 - a12, sv1, n_alpha_f, n_t_f, dist_scale, dist_bias, pitch4_f);
        // the taps' byte offsets inside a copy (the prepared pointer minus the origin it was formed from: folded away)
        const unsigned o0p = (unsigned)((GlobalBytes)t0p.ptr - sv0.origin), o1p = (unsigned)((GlobalBytes)t1p.ptr - sv1.origin);
        const unsigned o0m = (unsigned)((GlobalBytes)t0m.ptr - sv0.origin), o1m = (unsigned)((GlobalBytes)t1m.ptr - sv1.origin);
        float v0p[NC], v1p[NC], v0m[NC], v1m[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const GlobalBytes o0 = sv0.origin + chan * c, o1 = sv1.origin + chan * c;
            const auto tap = [](GlobalBytes origin, unsigned off, const LineTap t) {
                const ecc_v4f_a4 q4 = *(GlobalF4)(origin + off);
                const F4 q = {q4.x, q4.y, q4.z, q4.w};
                return line_tap_finish<DERIV>(q, t);
            };
            v0p[c] = tap(o0, o0p, t0p);
            v1p[c] = tap(o1, o1p, t1p);
            v0m[c] = tap(o0, o0m, t0m);
            v1m[c] = tap(o1, o1m, t1m);
        }
        const float dp = combine_channels<NC>(a0, v0p) - combine_channels<NC>(a1, v1p);
        const float dm = combine_channels<NC>(a0, v0m) - combine_channels<NC>(a1, v1m);
        acc[0] += (double)(((dp * dp + dm * dm) * K0[6]) * dkappa);  // ref: ...RadonIntermediate.cu:112,269
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            acc[1 + c] += (double)(((dp * v0p[c] + dm * v0m[c]) * K0[6]) * dkappa);
            acc[1 + NC + c] -= (double)(((dp * v1p[c] + dm * v1m[c]) * K0[6]) * dkappa);  // the minus of v0 - v1
        }
    }
}

// gram_accumulate (gram_kernel.hip): the same choice of loop for the same record, made by the same helpers.
template <bool DERIV, int NC>
__device__ __forceinline__ void coeff_accumulate(const EccPairParams& p, const EccViewCoeffParams& g, const EccPairRecord* __restrict__ rec,
                                                 int iD0, int iD1, int lane, const float (&a0)[NC], const float (&a1)[NC],
                                                 double (&acc)[coeff_entries(NC)])
{
    const unsigned pitch4 = (unsigned)p.pitch * 8u;
    const SlabView sv0 = {(GlobalBytes)p.dtrs[iD0], pitch4};
    const SlabView sv1 = {(GlobalBytes)p.dtrs[iD1], pitch4};
    const long long chan = g.paired_channel_bytes;
    const float n_alpha_f = (float)p.n_alpha, n_t_f = (float)p.n_t;
    const float pitch4_f = (float)pitch4;
    const float kappa_max = uniformf(rec->K1[7]);

    const bool reduce = kappa_max > 0.785398163397448f;  // wave-uniform
    const int poly_raw = __builtin_amdgcn_readfirstlane(rec->poly_ok);
    const int poly_ok = poly_raw & ~1;
    const bool in_range = (poly_raw & 1) != 0;
    int k_first = lane;
    if (poly_ok) {
        const float kappa_fit = ecc_kappa_fit(kappa_max), dkappa = uniformf(rec->K1[6]), w06 = uniformf(rec->K0[6]);
        poly_loop_dispatch(p.wide_offsets != 0, pitch4, poly_ok, in_range, [&](auto P4, auto DEG, auto NOCL) {
            k_first = coeff_loop_poly<DERIV, NC, decltype(P4)::value, decltype(DEG)::value, decltype(NOCL)::value>(
                lane, p.k_limit, rec, dkappa, kappa_fit, w06, sv0, sv1, chan, n_alpha_f, n_t_f, pitch4_f, a0, a1, acc);
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
        const long long chan_here = decltype(P4)::value == ECC_QUAD_LAYOUT ? g.quad_channel_bytes : chan;
        coeff_loop_exact<DERIV, NC, decltype(REDUCE)::value, decltype(P4)::value>(k_first, p.k_limit, K0, K1, v0, v1, chan_here, n_alpha_f, n_t_f,
                                                                                dist_scale, dist_bias, pitch4_f, a0, a1, acc);
    });
}

// One wave per pair, on pairs_kernel's workgroup -> pairs mapping (main_pair_of_wave, ecc_pairs_device.h).
// Registers: the 4 NC gathers of a kappa step as in pairs_gram_kernel, all 4 NC samples kept for the gradient
// products, 2 (1 + 2 NC) accumulator registers; tests/test_view_coefficients_abi.py pins the plan and what was built.
template <bool DERIV, int NC>
__global__ __launch_bounds__(PK_MAIN_THREADS) void pairs_coeff_kernel(EccPairParams p, EccViewCoeffParams g)
{
    constexpr int T = coeff_entries(NC);
    const int lane = threadIdx.x & 63;
    long long local;
    if (!main_pair_of_wave(p.count, local)) return;
    local = uniform_index(local);
    const EccPairRecord* __restrict__ rec = p.records + local;
    const int iD0 = __builtin_amdgcn_readfirstlane(rec->iD0), iD1 = __builtin_amdgcn_readfirstlane(rec->iD1);
    float a0[NC], a1[NC];
    pair_coefficients<NC>(g.coeffs, p.n_views, iD0, iD1, a0, a1);
    double acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = 0.0;
    coeff_accumulate<DERIV, NC>(p, g, rec, iD0, iD1, lane, a0, a1, acc);
#pragma unroll
    for (int t = 0; t < T; ++t) ecc_sum::wave_sum(acc[t]);
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < T; ++t) g.values[(long long)t * g.col_stride + local] = (float)acc[t];  // pair_value<false>
    }
}

// ---- ECC_SAMPLING_REFERENCE -------------------------------------------------------------------------
// gram_reference_loop (gram_kernel.hip) with the coefficient products: reference_loop's expressions on the signed samples.
template <int NC>
__device__ __forceinline__ void coeff_reference_loop(const EccPairParams& p, const float (&K0)[8], const float (&K1)[8],
                                                     const GlobalFloats (&d0)[NC], const GlobalFloats (&d1)[NC], const float (&a0)[NC],
                                                     const float (&a1)[NC], int first_k, int stride, double (&acc)[coeff_entries(NC)])
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
        float v0p[NC], v1p[NC], v0m[NC], v1m[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            v0p[c] = plain_tap_value(t0p, d0[c], p.pitch, p.n_alpha, p.n_t, deriv);
            v1p[c] = plain_tap_value(t1p, d1[c], p.pitch, p.n_alpha, p.n_t, deriv);
            v0m[c] = plain_tap_value(t0m, d0[c], p.pitch, p.n_alpha, p.n_t, deriv);
            v1m[c] = plain_tap_value(t1m, d1[c], p.pitch, p.n_alpha, p.n_t, deriv);
        }
        const float dp = combine_channels<NC>(a0, v0p) - combine_channels<NC>(a1, v1p);
        const float dm = combine_channels<NC>(a0, v0m) - combine_channels<NC>(a1, v1m);
        const float consistency = (dp * dp + dm * dm) * K0[6];  // ref: ...RadonIntermediate.cu:112
        acc[0] += (double)(consistency * dkappa);               // ref: ...RadonIntermediate.cu:269
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            acc[1 + c] += (double)(((dp * v0p[c] + dm * v0m[c]) * K0[6]) * dkappa);
            acc[1 + NC + c] -= (double)(((dp * v1p[c] + dm * v1m[c]) * K0[6]) * dkappa);  // the minus of v0 - v1
        }
    }
}

// pairs_gram_reference_kernel (gram_kernel.hip) with the coefficient products: SPLIT = 1 one wave per pair, SPLIT = 4 the
// workgroup's four waves on one pair with the wave sums added in wave order (the grouping the metric's mode fixes).
template <int NC, int SPLIT>
__global__ __launch_bounds__(PK_THREADS) void pairs_coeff_reference_kernel(EccPairParams p, EccViewCoeffParams g)
{
    static_assert(SPLIT == 1 || SPLIT == PK_THREADS / 64, "one pair per wave or per workgroup");
    constexpr int T = coeff_entries(NC);
    __shared__ double part[T][PK_THREADS / 64];
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
    float a0[NC], a1[NC];
    pair_coefficients<NC>(g.coeffs, p.n_views, iD0, iD1, a0, a1);
    double acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = 0.0;
    coeff_reference_loop<NC>(p, K0, K1, d0, d1, a0, a1, SPLIT == 1 ? lane : (int)threadIdx.x, 64 * SPLIT, acc);
#pragma unroll
    for (int t = 0; t < T; ++t) ecc_sum::wave_sum(acc[t]);
    if (SPLIT > 1) {  // wave sums -> wave 0, added in wave order (add_wave_partials)
        if (lane == 0) {
#pragma unroll
            for (int t = 0; t < T; ++t) part[t][wave] = acc[t];
        }
        __syncthreads();
        if (wave != 0) return;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            double sum = part[t][0];
#pragma unroll
            for (int w = 1; w < PK_THREADS / 64; ++w) sum += part[t][w];
            acc[t] = sum;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < T; ++t) g.values[(long long)t * g.col_stride + local] = (float)acc[t];
    }
}

template <int NC>
hipError_t launch_coeff_nc(const EccPairParams& p, const EccViewCoeffParams& g, hipStream_t stream)
{
    if (p.reference_arithmetic) {
        if (p.reference_split > 1)
            hipLaunchKernelGGL((pairs_coeff_reference_kernel<NC, 4>), dim3((unsigned)p.count), dim3(PK_THREADS), 0, stream, p, g);
        else
            hipLaunchKernelGGL((pairs_coeff_reference_kernel<NC, 1>), dim3((unsigned)((p.count + 3) / 4)), dim3(PK_THREADS), 0, stream, p, g);
        return hipGetLastError();
    }
    const dim3 grid = main_pairs_grid(p.count), block(PK_MAIN_THREADS);
    if (p.is_derivative) hipLaunchKernelGGL((pairs_coeff_kernel<true, NC>), grid, block, 0, stream, p, g);
    else hipLaunchKernelGGL((pairs_coeff_kernel<false, NC>), grid, block, 0, stream, p, g);
    return hipGetLastError();
}

}  // namespace

// The 1 + 2 K entries of every pair of the all-pairs launch p (records of ecc_launch_k01 for the same parameters, earlier on the
// same stream; first = 0, no index list, no slots) into g->values.  n_channels in [1, ECC_GRAM_CHANNELS_MAX]; g->coeffs: K * n_views
// floats on the device.
extern "C" hipError_t ecc_launch_pairs_coeff(const EccPairParams* p, const EccViewCoeffParams* g, int n_channels, hipStream_t stream)
{
    if (p->count <= 0) return hipSuccess;
    if (p->use_corr || p->indices || p->record_slots || p->skip_enabled || !g->values || !g->coeffs || g->col_stride < p->count ||
        (g->col_stride & 3))
        return hipErrorInvalidValue;
    switch (n_channels) {
    case 1: return launch_coeff_nc<1>(*p, *g, stream);
    case 2: return launch_coeff_nc<2>(*p, *g, stream);
    case 3: return launch_coeff_nc<3>(*p, *g, stream);
    case 4: return launch_coeff_nc<4>(*p, *g, stream);
    default: return hipErrorInvalidValue;
    }
}
