// robust_kernel.hip -- the metric under a per-sample robust loss (gfx950).
//
// A metric over one Radon intermediate per view, as pairs_kernel takes it.  For the pair i < j every +-kappa sample has the
// positions, kappa range and sampling mode of pairs_kernel's evaluation and d = the difference of the two signed data samples as
// pairs_kernel forms it.  Every loss here is rho(d) = w(d) d^2 with the IRLS weight w in (0, 1], one float32 operation per line,
// nothing contracted but the fmaf, the division the IEEE one:
//   a = fabsf(d)      t = fminf(1.0f, delta / a)                   (a == 0: +inf -> 1)
//   HUBER             w = t * (2.0f - t)                           rho = d^2 inside delta, 2 delta |d| - delta^2 outside
//   TRUNCATED         w = t * t                                    rho = min(d^2, delta^2)
//   GEMAN_MCCLURE     s = a * inv_delta; w = 1.0f / fmaf(s, s, 1.0f)    rho = d^2 delta^2 / (delta^2 + d^2)
// Per kappa step the value term is pairs_weighted_kernel's expression (weighted_kernel.hip) with w where it has mu:
//   polynomial loops             fmaf(w_p * dp, dp, (w_m * dm) * dm) * w06_dkappa
//   exact and reference loops    (((w_p * dp) * dp + (w_m * dm) * dm) * K0[6]) * dkappa
// so with w == 1.0f (delta = +inf, or any delta no |d| exceeds) these are pairs_kernel's bits.  Beside the value each lane adds
// (double)(w_p + w_m), the weight mass, (double)(dp * dp) + (double)(dm * dm), the raw squares (products in float32), and 2.0, the
// sample count.  Per pair
//   c = the float32 value, as pairs_kernel stores it,
//   u = (float)(mass / count), the INLIER MASS in (0, 1],
//   r = (float)(raw / count), the mean squared raw residual: no loss and no delta in it (ecc_host_robust_scale takes delta from it),
// a pair whose loops ran no trip (count == 0) has {0, 1, 0}; three columns, c and u summed by sum_gram_kernel (ecc_robust.hip).
// pairs_robust_kernel<DERIV> is pairs_weighted_kernel<DERIV> without the channel offset and its four weight gathers: one wave per
// pair, the record in scalar registers, the same dispatch over the record's degree and the slab size, the four positions of a kappa
// step computed once, 4 gathers, per-lane float64 sums in the same trip order, the same wave tree.  loss and delta are launch-uniform
// kernel arguments and the loss a uniform select (a scalar branch around one division), not a template parameter: three times the
// instantiations of every loop for the same registers.  Plain vector loads and stores only: no atomics, no inline
// assembly of its own.
// Not here (include/ecc_hip.h): pose-delta, transform, range, group and RCCL forms; the loss combined with line weights; the loss
// under the correlation cost; Tukey's biweight.
#include <hip/hip_runtime.h>
#include <float.h>

#include "ecc_layout.h"
#include "ecc_pairs_device.h"

namespace {

// the four per-lane sums: the value, the weight mass, the raw squares, the sample count
struct RobustSums {
    double value, mass, raw, count;
};

// the launch-uniform part of the loss
struct RobustLoss {
    int loss;
    float delta, inv_delta;
};

// w(d): the IRLS weight of a residual (see the head of this file; `loss` is wave-uniform, the branch a scalar one)
__device__ __forceinline__ float robust_weight(const RobustLoss& L, float d)
{
    const float a = fabsf(d);
    if (L.loss == ECC_ROBUST_GEMAN_MCCLURE) {
        const float s = a * L.inv_delta;
        return 1.0f / fmaf(s, s, 1.0f);
    }
    const float t = fminf(1.0f, L.delta / a);
    return L.loss == ECC_ROBUST_HUBER ? t * (2.0f - t) : t * t;
}

// the sums of a trip beside its value
__device__ __forceinline__ void robust_add(RobustSums& acc, float w_p, float w_m, float dp, float dm)
{
    acc.mass += (double)(w_p + w_m);
    acc.raw += (double)(dp * dp) + (double)(dm * dm);
    acc.count += 2.0;
}

// weighted_loop_poly (weighted_kernel.hip) with w(d) for mu: returns the lane's first sample index past the fit's range.
template <bool DERIV, int PITCH4, int DEG, bool NOCLAMP>
__device__ __forceinline__ int robust_loop_poly(int lane, int k_limit, const EccPairRecord* __restrict__ rec, float dkappa, float kappa_fit,
                                                float w06, const SlabView sv0, const SlabView sv1, float n_alpha_f, float n_t_f,
                                                float pitch4_f, const RobustLoss L, RobustSums& acc)
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
        const float dp = fmaf(v1p, rel_sign, v0p), dm = fmaf(v1m, rel_sign, v0m);
        const float w_p = robust_weight(L, dp), w_m = robust_weight(L, dm);
        acc.value += (double)(fmaf(w_p * dp, dp, (w_m * dm) * dm) * w06_dkappa);
        robust_add(acc, w_p, w_m, dp, dm);
    }
    return k;
}

// weighted_loop_exact (weighted_kernel.hip) with w(d) for mu: kappa_step's expressions on the signed data samples.
template <bool DERIV, bool REDUCE, int PITCH4>
__device__ __forceinline__ void robust_loop_exact(int k_first, int k_limit, const float (&K0)[8], const float (&K1)[8], const SlabView sv0,
                                                  const SlabView sv1, float n_alpha_f, float n_t_f, float dist_scale, float dist_bias,
                                                  float pitch4_f, const RobustLoss L, RobustSums& acc)
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
        const auto footprint = [](const LineTap& t) {
            const ecc_v4f_a4 q4 = *(GlobalF4)t.ptr;
            const F4 q = {q4.x, q4.y, q4.z, q4.w};
            return q;
        };
        const float v0p = line_tap_finish<DERIV>(footprint(t0p), t0p), v1p = line_tap_finish<DERIV>(footprint(t1p), t1p);
        const float v0m = line_tap_finish<DERIV>(footprint(t0m), t0m), v1m = line_tap_finish<DERIV>(footprint(t1m), t1m);
        const float dp = v0p - v1p, dm = v0m - v1m;
        const float w_p = robust_weight(L, dp), w_m = robust_weight(L, dm);
        acc.value += (double)((((w_p * dp) * dp + (w_m * dm) * dm) * K0[6]) * dkappa);  // ref: ...RadonIntermediate.cu:112,269,254
        robust_add(acc, w_p, w_m, dp, dm);
    }
}

// weighted_accumulate (weighted_kernel.hip): the same choice of loop for the same record, made by the same helpers.
template <bool DERIV>
__device__ __forceinline__ void robust_accumulate(const EccPairParams& p, const RobustLoss L, const EccPairRecord* __restrict__ rec, int iD0,
                                                  int iD1, int lane, RobustSums& acc)
{
    const unsigned pitch4 = (unsigned)p.pitch * 8u;
    const SlabView sv0 = {(GlobalBytes)p.dtrs[iD0], pitch4};
    const SlabView sv1 = {(GlobalBytes)p.dtrs[iD1], pitch4};
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
            k_first = robust_loop_poly<DERIV, decltype(P4)::value, decltype(DEG)::value, decltype(NOCL)::value>(
                lane, p.k_limit, rec, dkappa, kappa_fit, w06, sv0, sv1, n_alpha_f, n_t_f, pitch4_f, L, acc);
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
        robust_loop_exact<DERIV, decltype(REDUCE)::value, decltype(P4)::value>(k_first, p.k_limit, K0, K1, v0, v1, n_alpha_f, n_t_f, dist_scale,
                                                                              dist_bias, pitch4_f, L, acc);
    });
}

// The pair's three entries from the wave's sums (lane 0): c into column 0, u into column 1, r into column 2.
__device__ __forceinline__ void store_robust(const EccRobustParams& g, long long local, const RobustSums& acc)
{
    const bool any = acc.count > 0.0;
    g.values[local] = (float)acc.value;  // pair_value<false>; no trip: 0
    g.values[g.col_stride + local] = any ? (float)(acc.mass / acc.count) : 1.0f;
    g.values[2 * g.col_stride + local] = any ? (float)(acc.raw / acc.count) : 0.0f;
}

__device__ __forceinline__ RobustLoss uniform_loss(const EccRobustParams& g)
{
    const RobustLoss L = {__builtin_amdgcn_readfirstlane(g.loss), uniformf(g.delta), uniformf(g.inv_delta)};
    return L;
}

// One wave per pair, on pairs_kernel's workgroup -> pairs mapping (main_pair_of_wave, ecc_pairs_device.h).
// Registers: the 4 gathers of a kappa step as in pairs_kernel, 8 accumulator registers; tests/test_robust_abi.py pins
// the plan and what was built.
template <bool DERIV>
__global__ __launch_bounds__(PK_MAIN_THREADS) void pairs_robust_kernel(EccPairParams p, EccRobustParams g)
{
    const int lane = threadIdx.x & 63;
    long long local;
    if (!main_pair_of_wave(p.count, local)) return;
    local = uniform_index(local);
    const EccPairRecord* __restrict__ rec = p.records + local;
    const int iD0 = __builtin_amdgcn_readfirstlane(rec->iD0), iD1 = __builtin_amdgcn_readfirstlane(rec->iD1);
    RobustSums acc = {0.0, 0.0, 0.0, 0.0};
    robust_accumulate<DERIV>(p, uniform_loss(g), rec, iD0, iD1, lane, acc);
    ecc_sum::wave_sum(acc.value);
    ecc_sum::wave_sum(acc.mass);
    ecc_sum::wave_sum(acc.raw);
    ecc_sum::wave_sum(acc.count);
    if (lane == 0) store_robust(g, local, acc);
}

// ---- ECC_SAMPLING_REFERENCE -------------------------------------------------------------------------
// weighted_reference_loop (weighted_kernel.hip) with w(d) for mu: reference_loop's expressions on the signed data samples.
__device__ __forceinline__ void robust_reference_loop(const EccPairParams& p, const float (&K0)[8], const float (&K1)[8], GlobalFloats d0,
                                                      GlobalFloats d1, int first_k, int stride, const RobustLoss L, RobustSums& acc)
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
        const float dp = v0p - v1p, dm = v0m - v1m;
        const float w_p = robust_weight(L, dp), w_m = robust_weight(L, dm);
        const float consistency = ((w_p * dp) * dp + (w_m * dm) * dm) * K0[6];  // ref: ...RadonIntermediate.cu:112,254
        acc.value += (double)(consistency * dkappa);                           // ref: ...RadonIntermediate.cu:269
        robust_add(acc, w_p, w_m, dp, dm);
    }
}

// pairs_weighted_reference_kernel (weighted_kernel.hip) with w(d) for mu: SPLIT = 1 one wave per pair, SPLIT = 4 the workgroup's
// four waves on one pair with the wave sums added in wave order (the grouping the metric's mode fixes).
template <int SPLIT>
__global__ __launch_bounds__(PK_THREADS) void pairs_robust_reference_kernel(EccPairParams p, EccRobustParams g)
{
    static_assert(SPLIT == 1 || SPLIT == PK_THREADS / 64, "one pair per wave or per workgroup");
    __shared__ double part[SPLIT > 1 ? 4 : 1][SPLIT > 1 ? PK_THREADS / 64 : 1];
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
    RobustSums acc = {0.0, 0.0, 0.0, 0.0};
    robust_reference_loop(p, K0, K1, d0, d1, SPLIT == 1 ? lane : (int)threadIdx.x, 64 * SPLIT, uniform_loss(g), acc);
    ecc_sum::wave_sum(acc.value);
    ecc_sum::wave_sum(acc.mass);
    ecc_sum::wave_sum(acc.raw);
    ecc_sum::wave_sum(acc.count);
    if (SPLIT > 1) {  // wave sums -> wave 0, added in wave order (add_wave_partials)
        if (lane == 0) {
            part[0][wave] = acc.value;
            part[1][wave] = acc.mass;
            part[2][wave] = acc.raw;
            part[3][wave] = acc.count;
        }
        __syncthreads();
        if (wave != 0) return;
        double sum[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            sum[t] = part[t][0];
#pragma unroll
            for (int w = 1; w < PK_THREADS / 64; ++w) sum[t] += part[t][w];
        }
        acc.value = sum[0];
        acc.mass = sum[1];
        acc.raw = sum[2];
        acc.count = sum[3];
    }
    if (lane == 0) store_robust(g, local, acc);
}

}  // namespace

// The three entries {c, u, r} of every pair of the launch p (records of ecc_launch_k01 for the same parameters, earlier on the same
// stream; first = 0, no slots) into g->values.  p->indices may be set (an index list): the kernels do not read it, the record carries
// both Radon-intermediate indices.
extern "C" hipError_t ecc_launch_pairs_robust(const EccPairParams* p, const EccRobustParams* g, hipStream_t stream)
{
    if (p->count <= 0) return hipSuccess;
    if (p->use_corr || p->record_slots || p->skip_enabled || !g->values || g->col_stride < p->count || (g->col_stride & 3) ||
        g->loss < ECC_ROBUST_HUBER || g->loss > ECC_ROBUST_GEMAN_MCCLURE || !(g->delta > 0.f))
        return hipErrorInvalidValue;
    if (p->reference_arithmetic) {
        if (p->reference_split > 1)
            hipLaunchKernelGGL((pairs_robust_reference_kernel<4>), dim3((unsigned)p->count), dim3(PK_THREADS), 0, stream, *p, *g);
        else
            hipLaunchKernelGGL((pairs_robust_reference_kernel<1>), dim3((unsigned)((p->count + 3) / 4)), dim3(PK_THREADS), 0, stream, *p, *g);
        return hipGetLastError();
    }
    const dim3 grid = main_pairs_grid(p->count), block(PK_MAIN_THREADS);
    if (p->is_derivative) hipLaunchKernelGGL((pairs_robust_kernel<true>), grid, block, 0, stream, *p, *g);
    else hipLaunchKernelGGL((pairs_robust_kernel<false>), grid, block, 0, stream, *p, *g);
    return hipGetLastError();
}
