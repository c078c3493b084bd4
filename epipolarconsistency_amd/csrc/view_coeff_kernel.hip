// view_coeff_kernel.hip -- the metric of per-view channel coefficients and its gradient terms (gfx950).
//
// A metric over K * n Radon intermediates, channel-major (channel c of view i is dtr c * n + i), and K * n coefficients
// a[c * n + i]: the corrected intermediate of view i is sum_c a_c,i D_c,i, so for the pair i < j every redundant sample is
//   delta = sum_c a_c,i v0_c - sum_c a_c,j v1_c        (v0_c, v1_c: the signed samples of channel c in view i and in view j)
// at the sample positions, fold signs, kappa range and weights of pairs_kernel's evaluation, and per pair
//   value = sum_kappa (delta+^2 + delta-^2) K0[6] dkappa,
//   h0[c] = sum_kappa (delta+ v0+_c + delta- v0-_c) K0[6] dkappa = 1/2 d value / d a_c,i,
//   h1[c] = -sum_kappa (delta+ v1+_c + delta- v1-_c) K0[6] dkappa = 1/2 d value / d a_c,j.
// pairs_coeff_kernel<DERIV, NC> runs on the frames of ecc_pair_forms.h: form_accumulate, form_loop_poly,
// form_loop_exact.  CoeffForm's trip gathers NC footprints at each of the four taps and keeps all 4 NC samples, combines each side with
// the pair's 2 NC coefficients (scalar registers), and adds the value and the 2 NC gradient products to per-lane float64 sums in trip
// order; the kernel body and the reference kernels stay here.  A side's combined sample is formed in channel order,
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
#include "ecc_pair_forms.h"

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

// the trips of the polynomial and the exact loops (form_loop_poly, form_loop_exact, ecc_pair_forms.h): NC gathers at each of the four
// taps, every sample kept, the two combined differences, the 1 + 2 NC products
template <int NC>
struct CoeffForm : ChannelForm<EccViewCoeffParams> {
    const float (&a0)[NC];
    const float (&a1)[NC];
    double (&acc)[coeff_entries(NC)];
    float w1;  // view j's terms in a polynomial loop: the weight with the relative sign (header comment)

    __device__ __forceinline__ CoeffForm(const EccViewCoeffParams& g, const float (&a0)[NC], const float (&a1)[NC], double (&acc)[coeff_entries(NC)])
        : ChannelForm(g), a0(a0), a1(a1), acc(acc)
    {
    }

    __device__ __forceinline__ void poly_begin(const SlabView sv0, const SlabView sv1, float rel_sign, float w06_dkappa)
    {
        w1 = rel_sign * w06_dkappa;
        ChannelForm::poly_begin(sv0, sv1, rel_sign, w06_dkappa);
    }

    __device__ __forceinline__ void poly_trip(const SlabView sv0, const SlabView sv1, const SampleTap t0p, const SampleTap t1p,
                                              const SampleTap t0m, const SampleTap t1m, float rel_sign, float w06_dkappa)
    {
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

    template <bool DERIV, int PITCH4>
    __device__ __forceinline__ void exact_trip(const SlabView sv0, const SlabView sv1, const LineTap t0p, const LineTap t1p, const LineTap t0m,
                                               const LineTap t1m, float w06, float dkappa)
    {
        const unsigned o0p = line_tap_offset(t0p, sv0), o1p = line_tap_offset(t1p, sv1);
        const unsigned o0m = line_tap_offset(t0m, sv0), o1m = line_tap_offset(t1m, sv1);
        float v0p[NC], v1p[NC], v0m[NC], v1m[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const GlobalBytes o0 = sv0.origin + chan * c, o1 = sv1.origin + chan * c;
            v0p[c] = line_tap_finish<DERIV>(line_footprint(o0, o0p), t0p);
            v1p[c] = line_tap_finish<DERIV>(line_footprint(o1, o1p), t1p);
            v0m[c] = line_tap_finish<DERIV>(line_footprint(o0, o0m), t0m);
            v1m[c] = line_tap_finish<DERIV>(line_footprint(o1, o1m), t1m);
        }
        const float dp = combine_channels<NC>(a0, v0p) - combine_channels<NC>(a1, v1p);
        const float dm = combine_channels<NC>(a0, v0m) - combine_channels<NC>(a1, v1m);
        acc[0] += (double)(((dp * dp + dm * dm) * w06) * dkappa);  // ref: ...RadonIntermediate.cu:112,269
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            acc[1 + c] += (double)(((dp * v0p[c] + dm * v0m[c]) * w06) * dkappa);
            acc[1 + NC + c] -= (double)(((dp * v1p[c] + dm * v1m[c]) * w06) * dkappa);  // the minus of v0 - v1
        }
    }
};

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
    form_accumulate_local<DERIV, true, CoeffForm<NC>>(p, rec, iD0, iD1, lane, g, a0, a1, acc);
#pragma unroll
    for (int t = 0; t < T; ++t) ecc_sum::wave_sum(acc[t]);
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < T; ++t) g.values[(long long)t * g.col_stride + local] = (float)acc[t];  // pair_value<false>
    }
}

// ---- ECC_SAMPLING_REFERENCE -------------------------------------------------------------------------
// reference_loop<false> (ecc_pairs_device.h) for NC channels and their coefficients: its expressions on the signed samples.
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

// pairs_reference_kernel<false, SPLIT> for NC channels and their coefficients: SPLIT = 1 one wave per pair, SPLIT = 4 the
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
    return launch_pair_form(p, g, stream, pairs_coeff_reference_kernel<NC, 4>, pairs_coeff_reference_kernel<NC, 1>, pairs_coeff_kernel<true, NC>,
                            pairs_coeff_kernel<false, NC>);
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
