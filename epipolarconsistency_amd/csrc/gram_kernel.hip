// gram_kernel.hip -- the metric as a quadratic form of channel coefficients (gfx950).
//
// A metric over K * n Radon intermediates, channel-major (channel c of view i is dtr c * n + i).  Line integrals, the derivative
// across t, the ramp filter and bilinear sampling are linear, so for corrected images sum_c a_c I_c,i every redundant sample is
// linear in a and the metric is a^T G a with, per pair,
//   g[c][d] = sum_kappa (delta_c+ delta_d+ + delta_c- delta_d-) K0[6] dkappa,   delta_c = sample of channel c in view i - in view j,
// at the sample positions, fold signs, kappa range and weights of pairs_kernel's evaluation (they depend on the matrices only).
// pairs_gram_kernel<DERIV, NC> runs on the frames of ecc_pair_forms.h: form_accumulate (the choice of loop for the
// record), form_loop_poly and form_loop_exact (the position arithmetic of a kappa step, done ONCE).  GramForm's trip gathers NC
// footprints at each of the four taps, forms the two differences delta_c+-, and adds the T products to per-lane float64 sums in trip
// order; the kernel body and the reference kernels (loop, four-wave hand-over) stay here.  The diagonal entry (c, c) of a pair has the
// bits pairs_kernel gives on channel c's intermediates alone:
//   polynomial loops   fmaf(p_c, p_d, m_c * m_d) * w06_dkappa      (kappa_loop_poly; its two-steps-per-trip form adds the same
//                                                                    terms in the same order, so one step per trip is enough here)
//   exact loop         ((p_c * p_d + m_c * m_d) * K0[6]) * dkappa  (kappa_step)
//   reference loop     the same expression on sample_line_plain's samples (reference_loop)
// Only c <= d is computed.  The T = NC (NC + 1) / 2 columns are then summed by sum_gram_kernel (sum_kernel.hip) in the order of
// ecc_sum_order.h.
#include <hip/hip_runtime.h>
#include <float.h>

#include "ecc_layout.h"
#include "ecc_pair_forms.h"

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

// the trips of the polynomial and the exact loops (form_loop_poly, form_loop_exact, ecc_pair_forms.h): NC gathers at each of the four
// taps, the two differences of every channel, the T products
template <int NC>
struct GramForm : ChannelForm<EccGramParams> {
    double (&acc)[gram_entries(NC)];

    __device__ __forceinline__ GramForm(const EccGramParams& g, double (&acc)[gram_entries(NC)]) : ChannelForm(g), acc(acc) {}

    // the sign the two differences of a side share cancels in every product delta_c delta_d as it does in the square
    __device__ __forceinline__ void poly_trip(const SlabView sv0, const SlabView sv1, const SampleTap t0p, const SampleTap t1p,
                                              const SampleTap t0m, const SampleTap t1m, float rel_sign, float w06_dkappa)
    {
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

    template <bool DERIV, int PITCH4>
    __device__ __forceinline__ void exact_trip(const SlabView sv0, const SlabView sv1, const LineTap t0p, const LineTap t1p, const LineTap t0m,
                                               const LineTap t1m, float w06, float dkappa)
    {
        const unsigned o0p = line_tap_offset(t0p, sv0), o1p = line_tap_offset(t1p, sv1);
        const unsigned o0m = line_tap_offset(t0m, sv0), o1m = line_tap_offset(t1m, sv1);
        float vp[NC], vm[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const GlobalBytes o0 = sv0.origin + chan * c, o1 = sv1.origin + chan * c;
            const float v0p = line_tap_finish<DERIV>(line_footprint(o0, o0p), t0p), v1p = line_tap_finish<DERIV>(line_footprint(o1, o1p), t1p);
            const float v0m = line_tap_finish<DERIV>(line_footprint(o0, o0m), t0m), v1m = line_tap_finish<DERIV>(line_footprint(o1, o1m), t1m);
            vp[c] = v0p - v1p;
            vm[c] = v0m - v1m;
        }
        // ref: ...RadonIntermediate.cu:112,269 with the second factor exchanged
        gram_add<NC>(acc, [&](int c, int d) { return ((vp[c] * vp[d] + vm[c] * vm[d]) * w06) * dkappa; });
    }
};

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
    form_accumulate_local<DERIV, true, GramForm<NC>>(p, rec, iD0, iD1, lane, g, acc);
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
    return launch_pair_form(p, g, stream, pairs_gram_reference_kernel<NC, 4>, pairs_gram_reference_kernel<NC, 1>, pairs_gram_kernel<true, NC>,
                            pairs_gram_kernel<false, NC>);
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
