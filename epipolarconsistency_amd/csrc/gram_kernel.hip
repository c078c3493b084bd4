// gram_kernel.hip -- the metric as a quadratic form of channel coefficients (gfx950).
//
// A metric over K * n Radon intermediates, channel-major (channel c of view i is dtr c * n + i).  Line integrals, the derivative
// across t, the ramp filter and bilinear sampling are linear, so for corrected images sum_c a_c I_c,i every redundant sample is
// linear in a and the metric is a^T G a with, per pair,
//   g[c][d] = sum_kappa (delta_c+ delta_d+ + delta_c- delta_d-) K0[6] dkappa,   delta_c = sample of channel c in view i - in view j,
// at the sample positions, fold signs, kappa range and weights of pairs_kernel's evaluation (they depend on the matrices only).
// pairs_gram_kernel<DERIV, NC> is pairs_kernel with the position arithmetic of a kappa step done ONCE and NC gathers per sample
// position behind it: one wave per pair, the record in scalar registers, the same dispatch over the record's degree and the slab
// size (pair_accumulate, ecc_pairs_device.h), the same per-lane float64 sums in the same trip order, the same wave tree.  The
// diagonal entry (c, c) of a pair therefore has the bits pairs_kernel gives on channel c's intermediates alone:
//   polynomial loops   fmaf(p_c, p_d, m_c * m_d) * w06_dkappa      (kappa_loop_poly; its two-steps-per-trip form adds the same
//                                                                    terms in the same order, so one step per trip is enough here)
//   exact loop         ((p_c * p_d + m_c * m_d) * K0[6]) * dkappa  (kappa_step)
//   reference loop     the same expression on sample_line_plain's samples (reference_loop)
// Only c <= d is computed.  The T = NC (NC + 1) / 2 columns are then summed by sum_gram_kernel (sum_kernel.hip) in the order of
// ecc_sum_order.h.
#include <hip/hip_runtime.h>
#include <float.h>

#include "ecc_layout.h"
#include "ecc_pairs_device.h"

namespace {

constexpr int gram_entries(int nc) { return nc * (nc + 1) / 2; }

// acc[t] += term(c, d) for c <= d in the order of the columns
template <int NC, class Term>
__device__ __forceinline__ void gram_add(double (&acc)[gram_entries(NC)], const Term& term)
{
    int t = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int d = c; d < NC; ++d) acc[t++] += (double)term(c, d);
}

// kappa_loop_poly<DERIV, false, PITCH4, DEG, 1, NOCLAMP> for NC channels: returns the lane's first sample index past the fit's range.
// chan: bytes from a view's copy to the same view's copy of the next channel (wave-uniform).
template <bool DERIV, int NC, int PITCH4, int DEG, bool NOCLAMP>
__device__ __forceinline__ int gram_loop_poly(int lane, int k_limit, const EccPairRecord* __restrict__ rec, float dkappa,
                                              float kappa_fit, float w06, const SlabView sv0, const SlabView sv1, long long chan,
                                              float n_alpha_f, float n_t_f, float pitch4_f, double (&acc)[gram_entries(NC)])
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
    // the folds are the geometry's, the same for every channel: the relative sign serves all of them (see kappa_loop_poly), and the
    // sign the two differences of a side share cancels in every product delta_c delta_d as it does in the square
    const float rel_sign = (DERIV && ((fold[0] ^ fold[1]) & 0x80000000u)) ? 1.0f : -1.0f;
    const float w06_dkappa = w06 * dkappa;
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
        float vp[NC], vm[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const GlobalBytes o0 = sv0.origin + chan * c, o1 = sv1.origin + chan * c;
            const float v0p = sample_tap_value(o0, t0p), v1p = sample_tap_value(o1, t1p);
            const float v0m = sample_tap_value(o0, t0m), v1m = sample_tap_value(o1, t1m);
            vp[c] = fmaf(v1p, rel_sign, v0p);
            vm[c] = fmaf(v1m, rel_sign, v0m);
        }
        gram_add<NC>(acc, [&](int c, int d) { return fmaf(vp[c], vp[d], vm[c] * vm[d]) * w06_dkappa; });
    }
    return k;
}

// kappa_loop<DERIV, false, REDUCE, PITCH4> / kappa_step for NC channels.
template <bool DERIV, int NC, bool REDUCE, int PITCH4>
__device__ __forceinline__ void gram_loop_exact(int k_first, int k_limit, const float (&K0)[8], const float (&K1)[8], const SlabView sv0,
                                                const SlabView sv1, long long chan, float n_alpha_f, float n_t_f, float dist_scale,
                                                float dist_bias, float pitch4_f, double (&acc)[gram_entries(NC)])
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
        float vp[NC], vm[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const GlobalBytes o0 = sv0.origin + chan * c, o1 = sv1.origin + chan * c;
            const auto tap = [](GlobalBytes origin, unsigned off, const LineTap t) {
                const ecc_v4f_a4 q4 = *(GlobalF4)(origin + off);
                const F4 q = {q4.x, q4.y, q4.z, q4.w};
                return line_tap_finish<DERIV>(q, t);
            };
            const float v0p = tap(o0, o0p, t0p), v1p = tap(o1, o1p, t1p), v0m = tap(o0, o0m, t0m), v1m = tap(o1, o1m, t1m);
            vp[c] = v0p - v1p;
            vm[c] = v0m - v1m;
        }
        // ref: ...RadonIntermediate.cu:112,269 with the second factor exchanged
        gram_add<NC>(acc, [&](int c, int d) { return ((vp[c] * vp[d] + vm[c] * vm[d]) * K0[6]) * dkappa; });
    }
}

// pair_accumulate<DERIV, false> (ecc_pairs_device.h) for NC channels: the same choice of loop for the same record, made by the same
// helpers (poly_loop_dispatch, exact_loop_dispatch).
template <bool DERIV, int NC>
__device__ __forceinline__ void gram_accumulate(const EccPairParams& p, const EccGramParams& g, const EccPairRecord* __restrict__ rec,
                                                int iD0, int iD1, int lane, double (&acc)[gram_entries(NC)])
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
            k_first = gram_loop_poly<DERIV, NC, decltype(P4)::value, decltype(DEG)::value, decltype(NOCL)::value>(
                lane, p.k_limit, rec, dkappa, kappa_fit, w06, sv0, sv1, chan, n_alpha_f, n_t_f, pitch4_f, acc);
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
        gram_loop_exact<DERIV, NC, decltype(REDUCE)::value, decltype(P4)::value>(k_first, p.k_limit, K0, K1, v0, v1, chan_here, n_alpha_f, n_t_f,
                                                                               dist_scale, dist_bias, pitch4_f, acc);
    });
}

// One wave per pair, on pairs_kernel's workgroup -> pairs mapping (main_pair_of_wave, ecc_pairs_device.h).
// Registers: a kappa step has 4 NC gathers of 16 bytes in flight and the loop carries 2 T accumulator
// registers, so the kernel does not run at pairs_kernel's seven waves per SIMD; tests/test_gram_abi.py pins what was planned.
// (Measured and dropped: a scheduling barrier behind every channel, or every second one, of a step -- 4 or 8 gathers in flight
// instead of 4 NC, 67 / 88 / 117 or 78 / 99 / 124 vector registers instead of 78 / 110 / 147, i.e. up to two waves per SIMD
// more: 0.661 / 1.112 / 1.719 and 0.652 / 1.095 / 1.738 ms per call against 0.655 / 1.083 / 1.771 for K = 2 / 3 / 4, A/B on one
// box.  Occupancy traded for gathers in flight changes nothing: the launch waits for the memory path, as pairs_kernel does.
// A cap with amdgpu_num_vgpr spills at every value below the compiler's own choice.)
template <bool DERIV, int NC>
__global__ __launch_bounds__(PK_MAIN_THREADS) void pairs_gram_kernel(EccPairParams p, EccGramParams g)
{
    constexpr int T = gram_entries(NC);
    const int lane = threadIdx.x & 63;
    long long local;
    if (!main_pair_of_wave(p.count, local)) return;
    local = uniform_index(local);
    const EccPairRecord* __restrict__ rec = p.records + local;
    const int iD0 = __builtin_amdgcn_readfirstlane(rec->iD0), iD1 = __builtin_amdgcn_readfirstlane(rec->iD1);
    double acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = 0.0;
    gram_accumulate<DERIV, NC>(p, g, rec, iD0, iD1, lane, acc);
#pragma unroll
    for (int t = 0; t < T; ++t) ecc_sum::wave_sum(acc[t]);
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < T; ++t) g.values[(long long)t * g.col_stride + local] = (float)acc[t];  // pair_value<false>
    }
}

// ---- ECC_SAMPLING_REFERENCE -------------------------------------------------------------------------
// reference_loop<false> for NC channels: the samples first_k, first_k + stride, ... of one pair.
template <int NC>
__device__ __forceinline__ void gram_reference_loop(const EccPairParams& p, const float (&K0)[8], const float (&K1)[8],
                                                    const GlobalFloats (&d0)[NC], const GlobalFloats (&d1)[NC], int first_k, int stride,
                                                    double (&acc)[gram_entries(NC)])
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
        float vp[NC], vm[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float v0p = plain_tap_value(t0p, d0[c], p.pitch, p.n_alpha, p.n_t, deriv);
            const float v1p = plain_tap_value(t1p, d1[c], p.pitch, p.n_alpha, p.n_t, deriv);
            const float v0m = plain_tap_value(t0m, d0[c], p.pitch, p.n_alpha, p.n_t, deriv);
            const float v1m = plain_tap_value(t1m, d1[c], p.pitch, p.n_alpha, p.n_t, deriv);
            vp[c] = v0p - v1p;
            vm[c] = v0m - v1m;
        }
        gram_add<NC>(acc, [&](int c, int d) {
            const float consistency = (vp[c] * vp[d] + vm[c] * vm[d]) * K0[6];  // ref: ...RadonIntermediate.cu:112
            return consistency * dkappa;                                       // ref: ...RadonIntermediate.cu:269
        });
    }
}

// pairs_reference_kernel<false, SPLIT> for NC channels: SPLIT = 1 one wave per pair, SPLIT = 4 the workgroup's four waves on one
// pair with the wave sums added in wave order -- the grouping of the float64 sums that the metric's mode fixes (fill_pair_params).
// The dtrs' own slabs are separate allocations: every channel's slab comes from the table.
template <int NC, int SPLIT>
__global__ __launch_bounds__(PK_THREADS) void pairs_gram_reference_kernel(EccPairParams p, EccGramParams g)
{
    static_assert(SPLIT == 1 || SPLIT == PK_THREADS / 64, "one pair per wave or per workgroup");
    constexpr int T = gram_entries(NC);
    __shared__ double part[T][PK_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long local = SPLIT == 1 ? (long long)blockIdx.x * 4 + wave : (long long)blockIdx.x;
    if (local >= p.count) return;  // SPLIT > 1: uniform over the workgroup
    // the preamble of pairs_reference_kernel (kept apart: sharing changes pairs_kernel's code, see CHANGELOG)
    local = ((long long)__builtin_amdgcn_readfirstlane((int)(local >> 32)) << 32) |
            (unsigned)__builtin_amdgcn_readfirstlane((int)local);
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
    double acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = 0.0;
    gram_reference_loop<NC>(p, K0, K1, d0, d1, SPLIT == 1 ? lane : (int)threadIdx.x, 64 * SPLIT, acc);
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
hipError_t launch_gram_nc(const EccPairParams& p, const EccGramParams& g, hipStream_t stream)
{
    if (p.reference_arithmetic) {
        if (p.reference_split > 1)
            hipLaunchKernelGGL((pairs_gram_reference_kernel<NC, 4>), dim3((unsigned)p.count), dim3(PK_THREADS), 0, stream, p, g);
        else
            hipLaunchKernelGGL((pairs_gram_reference_kernel<NC, 1>), dim3((unsigned)((p.count + 3) / 4)), dim3(PK_THREADS), 0, stream, p, g);
        return hipGetLastError();
    }
    const dim3 grid = main_pairs_grid(p.count), block(PK_MAIN_THREADS);
    if (p.is_derivative) hipLaunchKernelGGL((pairs_gram_kernel<true, NC>), grid, block, 0, stream, p, g);
    else hipLaunchKernelGGL((pairs_gram_kernel<false, NC>), grid, block, 0, stream, p, g);
    return hipGetLastError();
}

}  // namespace

// The T = K (K + 1) / 2 entries of every pair of the all-pairs launch p (records of ecc_launch_k01 for the same parameters,
// earlier on the same stream; first = 0, no index list, no slots) into g->values.  n_channels in [2, ECC_GRAM_CHANNELS_MAX].
extern "C" hipError_t ecc_launch_pairs_gram(const EccPairParams* p, const EccGramParams* g, int n_channels, hipStream_t stream)
{
    if (p->count <= 0) return hipSuccess;
    if (p->use_corr || p->indices || p->record_slots || p->skip_enabled || !g->values || g->col_stride < p->count || (g->col_stride & 3))
        return hipErrorInvalidValue;
    switch (n_channels) {
    case 2: return launch_gram_nc<2>(*p, *g, stream);
    case 3: return launch_gram_nc<3>(*p, *g, stream);
    case 4: return launch_gram_nc<4>(*p, *g, stream);
    default: return hipErrorInvalidValue;
    }
}
