// weighted_kernel.hip -- the metric with per-line weights in Radon space (gfx950).
//
// A metric over 2 n Radon intermediates, channel-major as for the Gram form (ecc_layout.h): dtr i is the data of view i, dtr
// n + i the LINE WEIGHTS W_i of view i on the same bin grid (normally made with FILTER_NONE, values meant to lie in [0, 1]; any
// finite float is taken as it is).  For the pair i < j every +-kappa sample has the positions, kappa range and sampling mode of
// pairs_kernel's evaluation, d = the difference of the two signed data samples as pairs_kernel forms it, and
//   mu = W_i(sample) * W_j(sample)        one float32 multiply of two bilinear samples taken at the same taps as the data.
// The fold sign is NEVER applied to a weight sample: a weight is a property of the line, the same for both orientations of it
// (line_tap_finish<false>, plain_tap_value(.., false), the unsigned sample_tap_value without rel_sign).  Per kappa step the value
// term is pairs_kernel's expression with mu multiplied into the first factor only:
//   polynomial loops             fmaf(mu_p * dp, dp, (mu_m * dm) * dm) * w06_dkappa
//   exact and reference loops    (((mu_p * dp) * dp + (mu_m * dm) * dm) * K0[6]) * dkappa
// so with mu == 1.0f (1.0f * d is d) these are pairs_kernel's bits.  Beside the value each lane adds (double)(mu_p + mu_m) and 2.0
// per trip: the weight mass and the sample count.  Per pair
//   c = the float32 value, as pairs_kernel stores it,
//   u = (float)(mass / count), the COVERAGE in [0, 1] for weights in [0, 1]: one float64 division of the two wave sums; a pair whose
//       loops ran no trip (count == 0) has c = 0 and u = 1.0f,
// stored as two columns like the Gram form's entries and summed by sum_gram_kernel (ecc_weighted.hip divides the sums).
// pairs_weighted_kernel<DERIV> is pairs_coeff_kernel<DERIV, 2> (view_coeff_kernel.hip) with other and fewer products behind the same 8
// gathers: one wave per pair, the record in scalar registers, the same dispatch over the record's degree and the slab size, per-lane
// float64 sums in the same trip order, the same wave tree.  Plain vector loads and stores only: no atomics, no inline assembly of
// its own.
// Index lists and pose deltas launch these kernels over their own records (ecc_weighted_poses.hip).
// Not here (include/ecc_hip.h): full-matrices pose batches, transform, range, group and RCCL forms; weights under the correlation
// cost; a 1 / (sigma0^2 + sigma1^2) variance form.  A per-sample robust loss is robust_kernel.hip (not combined with these weights).
#include <hip/hip_runtime.h>
#include <float.h>

#include "ecc_layout.h"
#include "ecc_pairs_device.h"

namespace {

// the three per-lane sums: the value, the weight mass, the sample count
struct WeightedSums {
    double value, mass, count;
};

// coeff_loop_poly (view_coeff_kernel.hip) with the weighted products: returns the lane's first sample index past the fit's range.
// chan: bytes from a view's data copy to the same view's weight copy (wave-uniform).
template <bool DERIV, int PITCH4, int DEG, bool NOCLAMP>
__device__ __forceinline__ int weighted_loop_poly(int lane, int k_limit, const EccPairRecord* __restrict__ rec, float dkappa,
                                                  float kappa_fit, float w06, const SlabView sv0, const SlabView sv1, long long chan,
                                                  float n_alpha_f, float n_t_f, float pitch4_f, WeightedSums& acc)
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
    const float rel_sign = (DERIV && ((fold[0] ^ fold[1]) & 0x80000000u)) ? 1.0f : -1.0f;  // see kappa_loop_poly: the data only
    const float w06_dkappa = w06 * dkappa;
    const GlobalBytes w0 = sv0.origin + chan, w1 = sv1.origin + chan;
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
        const float v0p = sample_tap_value(sv0.origin, t0p), v1p = sample_tap_value(sv1.origin, t1p);
        const float v0m = sample_tap_value(sv0.origin, t0m), v1m = sample_tap_value(sv1.origin, t1m);
        const float mu_p = sample_tap_value(w0, t0p) * sample_tap_value(w1, t1p);  // unsigned, whatever the folds
        const float mu_m = sample_tap_value(w0, t0m) * sample_tap_value(w1, t1m);
        const float dp = fmaf(v1p, rel_sign, v0p), dm = fmaf(v1m, rel_sign, v0m);
        acc.value += (double)(fmaf(mu_p * dp, dp, (mu_m * dm) * dm) * w06_dkappa);
        acc.mass += (double)(mu_p + mu_m);
        acc.count += 2.0;
    }
    return k;
}

// coeff_loop_exact (view_coeff_kernel.hip) with the weighted products: kappa_step's expressions on the signed data samples, the
// weights without the fold's sign.
template <bool DERIV, bool REDUCE, int PITCH4>
__device__ __forceinline__ void weighted_loop_exact(int k_first, int k_limit, const float (&K0)[8], const float (&K1)[8], const SlabView sv0,
                                                    const SlabView sv1, long long chan, float n_alpha_f, float n_t_f, float dist_scale,
                                                    float dist_bias, float pitch4_f, WeightedSums& acc)
{
    const float dkappa = K1[6], kappa_max = K1[7];
    const GlobalBytes w0 = sv0.origin + chan, w1 = sv1.origin + chan;
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
        const auto footprint = [](GlobalBytes origin, unsigned off) {
            const ecc_v4f_a4 q4 = *(GlobalF4)(origin + off);
            const F4 q = {q4.x, q4.y, q4.z, q4.w};
            return q;
        };
        const float v0p = line_tap_finish<DERIV>(footprint(sv0.origin, o0p), t0p), v1p = line_tap_finish<DERIV>(footprint(sv1.origin, o1p), t1p);
        const float v0m = line_tap_finish<DERIV>(footprint(sv0.origin, o0m), t0m), v1m = line_tap_finish<DERIV>(footprint(sv1.origin, o1m), t1m);
        const float mu_p = line_tap_finish<false>(footprint(w0, o0p), t0p) * line_tap_finish<false>(footprint(w1, o1p), t1p);
        const float mu_m = line_tap_finish<false>(footprint(w0, o0m), t0m) * line_tap_finish<false>(footprint(w1, o1m), t1m);
        const float dp = v0p - v1p, dm = v0m - v1m;
        acc.value += (double)((((mu_p * dp) * dp + (mu_m * dm) * dm) * K0[6]) * dkappa);  // ref: ...RadonIntermediate.cu:112,269,254
        acc.mass += (double)(mu_p + mu_m);
        acc.count += 2.0;
    }
}

// coeff_accumulate (view_coeff_kernel.hip): the same choice of loop for the same record, made by the same helpers.
template <bool DERIV>
__device__ __forceinline__ void weighted_accumulate(const EccPairParams& p, const EccWeightedParams& g, const EccPairRecord* __restrict__ rec,
                                                    int iD0, int iD1, int lane, WeightedSums& acc)
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
            k_first = weighted_loop_poly<DERIV, decltype(P4)::value, decltype(DEG)::value, decltype(NOCL)::value>(
                lane, p.k_limit, rec, dkappa, kappa_fit, w06, sv0, sv1, chan, n_alpha_f, n_t_f, pitch4_f, acc);
        });
        if (!(kappa_fit < kappa_max)) return;  // wave-uniform: the polynomials covered the whole range (the normal case)
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
        weighted_loop_exact<DERIV, decltype(REDUCE)::value, decltype(P4)::value>(k_first, p.k_limit, K0, K1, v0, v1, chan_here, n_alpha_f, n_t_f,
                                                                                dist_scale, dist_bias, pitch4_f, acc);
    });
}

// The pair's two entries from the wave's sums (lane 0): c into column 0, u into column 1.
__device__ __forceinline__ void store_weighted(const EccWeightedParams& g, long long local, const WeightedSums& acc)
{
    g.values[local] = (float)acc.value;  // pair_value<false>; no trip: 0
    g.values[g.col_stride + local] = acc.count > 0.0 ? (float)(acc.mass / acc.count) : 1.0f;
}

// One wave per pair, on pairs_kernel's workgroup -> pairs mapping (main_pair_of_wave, ecc_pairs_device.h).
// Registers: the 8 gathers of a kappa step as in pairs_coeff_kernel<DERIV, 2>, 6 accumulator registers against its
// 10 and no coefficient registers; tests/test_weighted_abi.py pins the plan and what was built.
template <bool DERIV>
__global__ __launch_bounds__(PK_MAIN_THREADS) void pairs_weighted_kernel(EccPairParams p, EccWeightedParams g)
{
    const int lane = threadIdx.x & 63;
    long long local;
    if (!main_pair_of_wave(p.count, local)) return;
    local = uniform_index(local);
    const EccPairRecord* __restrict__ rec = p.records + local;
    const int iD0 = __builtin_amdgcn_readfirstlane(rec->iD0), iD1 = __builtin_amdgcn_readfirstlane(rec->iD1);
    WeightedSums acc = {0.0, 0.0, 0.0};
    weighted_accumulate<DERIV>(p, g, rec, iD0, iD1, lane, acc);
    ecc_sum::wave_sum(acc.value);
    ecc_sum::wave_sum(acc.mass);
    ecc_sum::wave_sum(acc.count);
    if (lane == 0) store_weighted(g, local, acc);
}

// ---- ECC_SAMPLING_REFERENCE -------------------------------------------------------------------------
// coeff_reference_loop (view_coeff_kernel.hip) with the weighted products: reference_loop's expressions on the signed data samples.
__device__ __forceinline__ void weighted_reference_loop(const EccPairParams& p, const float (&K0)[8], const float (&K1)[8], GlobalFloats d0,
                                                        GlobalFloats d1, GlobalFloats w0, GlobalFloats w1, int first_k, int stride,
                                                        WeightedSums& acc)
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
        const float v0p = plain_tap_value(t0p, d0, p.pitch, p.n_alpha, p.n_t, deriv), v1p = plain_tap_value(t1p, d1, p.pitch, p.n_alpha, p.n_t, deriv);
        const float v0m = plain_tap_value(t0m, d0, p.pitch, p.n_alpha, p.n_t, deriv), v1m = plain_tap_value(t1m, d1, p.pitch, p.n_alpha, p.n_t, deriv);
        const float mu_p = plain_tap_value(t0p, w0, p.pitch, p.n_alpha, p.n_t, false) * plain_tap_value(t1p, w1, p.pitch, p.n_alpha, p.n_t, false);
        const float mu_m = plain_tap_value(t0m, w0, p.pitch, p.n_alpha, p.n_t, false) * plain_tap_value(t1m, w1, p.pitch, p.n_alpha, p.n_t, false);
        const float dp = v0p - v1p, dm = v0m - v1m;
        const float consistency = ((mu_p * dp) * dp + (mu_m * dm) * dm) * K0[6];  // ref: ...RadonIntermediate.cu:112,254
        acc.value += (double)(consistency * dkappa);                             // ref: ...RadonIntermediate.cu:269
        acc.mass += (double)(mu_p + mu_m);
        acc.count += 2.0;
    }
}

// pairs_coeff_reference_kernel (view_coeff_kernel.hip) with the weighted products: SPLIT = 1 one wave per pair, SPLIT = 4 the
// workgroup's four waves on one pair with the wave sums added in wave order (the grouping the metric's mode fixes).
template <int SPLIT>
__global__ __launch_bounds__(PK_THREADS) void pairs_weighted_reference_kernel(EccPairParams p, EccWeightedParams g)
{
    static_assert(SPLIT == 1 || SPLIT == PK_THREADS / 64, "one pair per wave or per workgroup");
    __shared__ double part[3][PK_THREADS / 64];
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
    const GlobalFloats d0 = (GlobalFloats)p.slabs[iD0], d1 = (GlobalFloats)p.slabs[iD1];
    const GlobalFloats w0 = (GlobalFloats)p.slabs[(long long)p.n_views + iD0], w1 = (GlobalFloats)p.slabs[(long long)p.n_views + iD1];
    WeightedSums acc = {0.0, 0.0, 0.0};
    weighted_reference_loop(p, K0, K1, d0, d1, w0, w1, SPLIT == 1 ? lane : (int)threadIdx.x, 64 * SPLIT, acc);
    ecc_sum::wave_sum(acc.value);
    ecc_sum::wave_sum(acc.mass);
    ecc_sum::wave_sum(acc.count);
    if (SPLIT > 1) {  // wave sums -> wave 0, added in wave order (add_wave_partials)
        if (lane == 0) {
            part[0][wave] = acc.value;
            part[1][wave] = acc.mass;
            part[2][wave] = acc.count;
        }
        __syncthreads();
        if (wave != 0) return;
        double sum[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            sum[t] = part[t][0];
#pragma unroll
            for (int w = 1; w < PK_THREADS / 64; ++w) sum[t] += part[t][w];
        }
        acc.value = sum[0];
        acc.mass = sum[1];
        acc.count = sum[2];
    }
    if (lane == 0) store_weighted(g, local, acc);
}

}  // namespace

// The two entries {c, u} of every pair of the launch p (records of ecc_launch_k01 for the same parameters, earlier on the same
// stream; first = 0, no slots) into g->values; the metric's dtrs are the data of the n_views views, then their line weights.
// p->indices may be set (an index list, a pose batch's grid): the kernels do not read it, the record carries both Radon-intermediate
// indices, which must lie in [0, n_views) -- the weights of a sample come from dtr n_views + that index.
extern "C" hipError_t ecc_launch_pairs_weighted(const EccPairParams* p, const EccWeightedParams* g, hipStream_t stream)
{
    if (p->count <= 0) return hipSuccess;
    if (p->use_corr || p->record_slots || p->skip_enabled || !g->values || g->col_stride < p->count || (g->col_stride & 3))
        return hipErrorInvalidValue;
    if (p->reference_arithmetic) {
        if (p->reference_split > 1)
            hipLaunchKernelGGL((pairs_weighted_reference_kernel<4>), dim3((unsigned)p->count), dim3(PK_THREADS), 0, stream, *p, *g);
        else
            hipLaunchKernelGGL((pairs_weighted_reference_kernel<1>), dim3((unsigned)((p->count + 3) / 4)), dim3(PK_THREADS), 0, stream, *p, *g);
        return hipGetLastError();
    }
    const dim3 grid = main_pairs_grid(p->count), block(PK_MAIN_THREADS);
    if (p->is_derivative) hipLaunchKernelGGL((pairs_weighted_kernel<true>), grid, block, 0, stream, *p, *g);
    else hipLaunchKernelGGL((pairs_weighted_kernel<false>), grid, block, 0, stream, *p, *g);
    return hipGetLastError();
}
