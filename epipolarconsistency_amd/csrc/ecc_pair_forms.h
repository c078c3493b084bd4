// ecc_pair_forms.h -- the loop skeleton shared by the pair-form kernels (gram_kernel.hip, view_coeff_kernel.hip,
// view_hessian_kernel.hip, weighted_kernel.hip, variance_kernel.hip, and through ecc_loss_forms.h robust_kernel.hip,
// weighted_robust_kernel.hip, variance_robust_kernel.hip and the three map kernels), stated once.
//
// A FORM of the pair metric is pairs_kernel's evaluation of one pair per wave -- the record in scalar registers, the dispatch over
// the record's degree and the slab size, the four sample positions of a kappa step, per-lane float64 sums in trip order, the wave
// tree -- with its own gathers and products behind the four positions.  The frames below own everything up to the four taps of a
// kappa step; a form is a small struct in its kernel file that owns what is gathered there and what is added (the forms under a
// robust loss, which an evaluation kernel and its map kernel share, are templates in ecc_loss_forms.h).  Its members:
//   poly_begin(sv0, sv1, rel_sign, w06_dkappa)                before a polynomial loop: what the form derives from the loop's uniforms
//   poly_trip(sv0, sv1, t0p, t1p, t0m, t1m, rel_sign, w06_dkappa)    one kappa step of a polynomial loop: SampleTaps, UNSIGNED samples
//   poly_end(rel_sign)                                        after a polynomial loop
//   exact_begin<PITCH4>(sv0, sv1)                             before an exact loop (PITCH4 == ECC_QUAD_LAYOUT: the row-quad copies)
//   exact_trip<DERIV, PITCH4>(sv0, sv1, t0p, t1p, t0m, t1m, w06, dkappa)    one step of an exact loop: LineTaps, signed samples
//   begin(p, iD0, iD1), reference_begin(p, iD0, iD1)          form_main_sums / form_reference_sums only: once per pair
//   reference_trip(p, deriv, t0p, t1p, t0m, t1m, w06, dkappa) form_reference_loop only: one step, PlainTaps
// (PairFormDefaults has the empty ones.)  The lane's sums live in the kernel, double acc[T], one per stored column; the form holds a
// reference.  The kernels themselves (names, template parameters, launch bounds), how lane 0 turns sums into columns, and the
// extern "C" launch functions with their argument checks stay in the form's file.
// What a trip may assume: everything it is handed but the taps is wave-uniform (sv0, sv1, rel_sign, w06_dkappa, w06, dkappa live in
// scalar registers), and so is every member the begin hooks set; a trip runs inside a divergent loop, the lanes past the range have
// left it; rel_sign is +1.0f or -1.0f (-1.0f for plain data), applied to data samples only.
// The ORDER OF STATEMENTS in the frames is the order the forms' kernels were built with, and the compiler's output follows it:
// w06_dkappa after rel_sign, the begin hook after both and before the lane's k, the record's exact-loop part read after the polynomial
// branch, `deriv` before the reference loop.  So does where the form object lives (form_accumulate_local).  Every kernel keeps the
// instruction stream it had with the skeleton written out in its file; which pieces each form takes from here, and which it keeps,
// is in the CHANGELOG ("the pair forms' loop skeleton once").
#ifndef ECC_PAIR_FORMS_H
#define ECC_PAIR_FORMS_H

#include <utility>
#include "ecc_pairs_device.h"

namespace {

// the hooks most forms leave empty
struct PairFormDefaults {
    __device__ __forceinline__ void begin(const EccPairParams&, int, int) {}
    __device__ __forceinline__ void poly_begin(const SlabView, const SlabView, float, float) {}
    __device__ __forceinline__ void poly_end(float) {}
    template <int PITCH4>
    __device__ __forceinline__ void exact_begin(const SlabView, const SlabView)
    {
    }
};

// ---- the exact loops' taps in a channel-major metric ---------------------------------------------------
// A tap's byte offset inside a copy (the prepared pointer minus the origin it was formed from: folded away), and the footprint at that
// offset of another channel's copy.
__device__ __forceinline__ unsigned line_tap_offset(const LineTap t, const SlabView sv)
{
    return (unsigned)((GlobalBytes)t.ptr - sv.origin);
}

__device__ __forceinline__ F4 line_footprint(GlobalBytes origin, unsigned off)
{
    const ecc_v4f_a4 q4 = *(GlobalF4)(origin + off);
    const F4 q = {q4.x, q4.y, q4.z, q4.w};
    return q;
}

// bytes from a view's copy to the same view's copy of the next channel, in the copies the loop for PITCH4 samples (wave-uniform)
template <int PITCH4, class G>
__device__ __forceinline__ long long channel_bytes(const G& g)
{
    return PITCH4 == ECC_QUAD_LAYOUT ? g.quad_channel_bytes : g.paired_channel_bytes;
}

// the wave tree over every sum, one call per sum
template <int T, size_t... I>
__device__ __forceinline__ void form_wave_sums(double (&acc)[T], std::index_sequence<I...>)
{
    (ecc_sum::wave_sum(acc[I]), ...);
}

// What the channel forms (K intermediates per view, channel-major) share: the launch's channel parameters and, per loop, the bytes
// from one channel's copy to the next (read before the loop, as the kernels were built).
template <class G>
struct ChannelForm : PairFormDefaults {
    const G& g;
    long long chan;

    __device__ __forceinline__ explicit ChannelForm(const G& g) : g(g) {}
    __device__ __forceinline__ void poly_begin(const SlabView, const SlabView, float, float) { chan = g.paired_channel_bytes; }
    template <int PITCH4>
    __device__ __forceinline__ void exact_begin(const SlabView, const SlabView)
    {
        chan = channel_bytes<PITCH4>(g);
    }
};

// ---- 1. the polynomial loop ------------------------------------------------------------------------------
// kappa_loop_poly<DERIV, false, PITCH4, DEG, 1, NOCLAMP> (its two-steps-per-trip form adds the same terms in the same order, so one
// step per trip is enough) up to the four taps: returns the lane's first sample index past the fit's range.
template <bool DERIV, int PITCH4, int DEG, bool NOCLAMP, class Form>
__device__ __forceinline__ int form_loop_poly(Form& form, int lane, int k_limit, const EccPairRecord* __restrict__ rec, float dkappa,
                                              float kappa_fit, float w06, const SlabView sv0, const SlabView sv1, float n_alpha_f,
                                              float n_t_f, float pitch4_f)
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
    // the folds are the geometry's, the same for every channel: the relative sign serves all of them (see kappa_loop_poly), applied
    // to data samples only
    const float rel_sign = (DERIV && ((fold[0] ^ fold[1]) & 0x80000000u)) ? 1.0f : -1.0f;  // (written out: the select the kernels have)
    const float w06_dkappa = w06 * dkappa;
    form.poly_begin(sv0, sv1, rel_sign, w06_dkappa);
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
        form.poly_trip(sv0, sv1, t0p, t1p, t0m, t1m, rel_sign, w06_dkappa);
    }
    form.poly_end(rel_sign);
    return k;
}

// ---- 2. the exact loop -------------------------------------------------------------------------------------
// kappa_loop<DERIV, false, REDUCE, PITCH4> / kappa_step up to the four taps.
template <bool DERIV, bool REDUCE, int PITCH4, class Form>
__device__ __forceinline__ void form_loop_exact(Form& form, int k_first, int k_limit, const float (&K0)[8], const float (&K1)[8],
                                                const SlabView sv0, const SlabView sv1, float n_alpha_f, float n_t_f, float dist_scale,
                                                float dist_bias, float pitch4_f)
{
    const float dkappa = K1[6], kappa_max = K1[7];
    form.template exact_begin<PITCH4>(sv0, sv1);
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
        form.template exact_trip<DERIV, PITCH4>(sv0, sv1, t0p, t1p, t0m, t1m, K0[6], dkappa);
    }
}

// ---- 3. the choice of loop ---------------------------------------------------------------------------------
// pair_accumulate<DERIV, false> (ecc_pairs_device.h) for a form: the same choice of loop for the same record, made by the same
// helpers (poly_loop_dispatch, exact_loop_dispatch).  FENCE: the form's kernels were built with pair_accumulate's fence on the record
// pointer behind the polynomial branch (gram, coefficients), or without it (weighted, robust).
template <bool DERIV, bool FENCE, class Form>
__device__ __forceinline__ void form_accumulate(const EccPairParams& p, const EccPairRecord* __restrict__ rec, int iD0, int iD1, int lane,
                                                Form& form)
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
            k_first = form_loop_poly<DERIV, decltype(P4)::value, decltype(DEG)::value, decltype(NOCL)::value>(
                form, lane, p.k_limit, rec, dkappa, kappa_fit, w06, sv0, sv1, n_alpha_f, n_t_f, pitch4_f);
        });
        if (!(kappa_fit < kappa_max)) return;  // wave-uniform: the polynomials covered the whole range (the normal case)
        if constexpr (FENCE) asm volatile("" : "+s"(rec));  // what follows is read from the record afterwards (as in pair_accumulate)
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

// The same with the form object made here, from `args`, inside the inlined callee: where the channel forms' kernels were built with it.
// (The forms with named sums keep theirs in the kernel's own scope; the compiler's loop structure follows that difference, CHANGELOG.)
template <bool DERIV, bool FENCE, class Form, class... Args>
__device__ __forceinline__ void form_accumulate_local(const EccPairParams& p, const EccPairRecord* __restrict__ rec, int iD0, int iD1,
                                                      int lane, Args&&... args)
{
    Form form(args...);
    form_accumulate<DERIV, FENCE>(p, rec, iD0, iD1, lane, form);
}

// ---- 4. the main kernel's body -----------------------------------------------------------------------------
// One wave per pair, on pairs_kernel's workgroup -> pairs mapping (main_pair_of_wave): the wave's sums of pair `local` into acc (the
// array the form adds to).  True in the lane that stores them.  Used by the forms with named sums (weighted, robust); the channel forms'
// kernels keep their bodies, whose loops over the sums the compiler schedules differently (CHANGELOG).
template <bool DERIV, class Form, int T>
__device__ __forceinline__ bool form_main_sums(const EccPairParams& p, Form& form, double (&acc)[T], long long& local)
{
    const int lane = threadIdx.x & 63;
    if (!main_pair_of_wave(p.count, local)) return false;
    local = uniform_index(local);
    const EccPairRecord* __restrict__ rec = p.records + local;
    const int iD0 = __builtin_amdgcn_readfirstlane(rec->iD0), iD1 = __builtin_amdgcn_readfirstlane(rec->iD1);
    form.begin(p, iD0, iD1);
    form_accumulate<DERIV, false>(p, rec, iD0, iD1, lane, form);
    form_wave_sums(acc, std::make_index_sequence<T>{});
    return lane == 0;
}

// ---- ECC_SAMPLING_REFERENCE ----------------------------------------------------------------------------
// 5. reference_loop<false> up to the four taps: the samples first_k, first_k + stride, ... of one pair.
template <class Form>
__device__ __forceinline__ void form_reference_loop(Form& form, const EccPairParams& p, const float (&K0)[8], const float (&K1)[8],
                                                    int first_k, int stride)
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
        form.reference_trip(p, deriv, t0p, t1p, t0m, t1m, K0[6], dkappa);
    }
}

// 6. pairs_reference_kernel<false, SPLIT> for a form: SPLIT = 1 one wave per pair, SPLIT = 4 the workgroup's four waves on one pair
// with the wave sums added in wave order -- the grouping of the float64 sums that the metric's mode fixes (fill_pair_params).  The
// sums of pair `local` into acc; true in the lane that stores them.  (The preamble of pairs_reference_kernel itself is kept apart:
// sharing it changes pairs_kernel.hip's code, see CHANGELOG.)
template <int SPLIT, class Form, int T>
__device__ __forceinline__ bool form_reference_sums(const EccPairParams& p, Form& form, double (&acc)[T], long long& local)
{
    static_assert(SPLIT == 1 || SPLIT == PK_THREADS / 64, "one pair per wave or per workgroup");
    __shared__ double part[T][PK_THREADS / 64];  // (SPLIT = 1: never touched, no LDS allocated)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    local = SPLIT == 1 ? (long long)blockIdx.x * 4 + wave : (long long)blockIdx.x;
    if (local >= p.count) return false;  // SPLIT > 1: uniform over the workgroup
    local = uniform_index(local);
    const EccPairRecord* __restrict__ rec = p.records + local;
    float K0[8], K1[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        K0[i] = uniformf(rec->K0[i]);
        K1[i] = uniformf(rec->K1[i]);
    }
    const int iD0 = __builtin_amdgcn_readfirstlane(rec->iD0), iD1 = __builtin_amdgcn_readfirstlane(rec->iD1);
    form.reference_begin(p, iD0, iD1);
    form_reference_loop(form, p, K0, K1, SPLIT == 1 ? lane : (int)threadIdx.x, 64 * SPLIT);
    form_wave_sums(acc, std::make_index_sequence<T>{});
    if (SPLIT > 1) {  // wave sums -> wave 0, added in wave order (add_wave_partials)
        if (lane == 0) {
#pragma unroll
            for (int t = 0; t < T; ++t) part[t][wave] = acc[t];
        }
        __syncthreads();
        if (wave != 0) return false;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            double sum = part[t][0];
#pragma unroll
            for (int w = 1; w < PK_THREADS / 64; ++w) sum += part[t][w];
            acc[t] = sum;
        }
    }
    return lane == 0;
}

// ---- 7. the host's choice of kernel ------------------------------------------------------------------------
// The reference kernel for four waves or for one wave per pair, else the main kernel for derivative or plain data.  lds_bytes: the
// dynamic LDS of a workgroup, for the forms that size theirs by the launch (residual_histogram_kernel.hip).
template <class G>
hipError_t launch_pair_form(const EccPairParams& p, const G& g, hipStream_t stream, void (*ref4)(EccPairParams, G),
                            void (*ref1)(EccPairParams, G), void (*main_deriv)(EccPairParams, G), void (*main_plain)(EccPairParams, G),
                            size_t lds_bytes = 0)
{
    if (p.reference_arithmetic) {
        if (p.reference_split > 1) hipLaunchKernelGGL(ref4, dim3((unsigned)p.count), dim3(PK_THREADS), lds_bytes, stream, p, g);
        else hipLaunchKernelGGL(ref1, dim3((unsigned)((p.count + 3) / 4)), dim3(PK_THREADS), lds_bytes, stream, p, g);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(p.is_derivative ? main_deriv : main_plain, main_pairs_grid(p.count), dim3(PK_MAIN_THREADS), lds_bytes, stream, p, g);
    return hipGetLastError();
}

}  // namespace

#endif
