// weighted_robust_kernel.hip -- the metric with per-line weights AND a per-sample robust loss (gfx950).
//
// A metric over 2 n Radon intermediates as weighted_kernel.hip takes it: dtr i is the data of view i, dtr n + i the LINE WEIGHTS W_i
// of view i on the same bin grid.  The weights say which lines somebody flagged (a collimator blade, a table edge); the loss takes
// care of what nobody flagged (an instrument, a defect that appears mid-scan).  For the pair i < j every +-kappa sample has the
// positions, kappa range and sampling mode of pairs_kernel's evaluation, d = the difference of the two signed data samples as
// pairs_kernel forms it, and
//   mu = W_i(sample) * W_j(sample)     as in weighted_kernel.hip: unsigned taps of the weight copies, one float32 multiply
//   w  = robust_weight(L, d)           as in robust_kernel.hip (ecc_robust_weight.h), of the RAW residual d: a line weight says how
//                                      far a line is trusted, it does not rescale its residual
//   f  = mu * w                        one float32 multiply
// Per kappa step the value term is pairs_kernel's expression with f multiplied into the first factor only:
//   polynomial loops             fmaf(f_p * dp, dp, (f_m * dm) * dm) * w06_dkappa
//   exact and reference loops    (((f_p * dp) * dp + (f_m * dm) * dm) * K0[6]) * dkappa
// Beside the value each lane adds (double)(mu_p + mu_m), the weight mass, (double)(f_p + f_m), the mass the loss keeps,
// (double)(mu_p * (dp * dp)) + (double)(mu_m * (dm * dm)), the weighted raw squares (products in float32), and 2.0, the sample
// count.  Per pair, four columns
//   c = the float32 value, as pairs_kernel stores it,
//   u = (float)(mass / count), the COVERAGE of weighted_kernel.hip,
//   k = (float)(kept / count), the weight mass the loss keeps: k <= u for weights >= 0, k / u is the inlier mass among the trusted lines,
//   r = (float)(raw / count), the weighted mean squared raw residual: no loss and no delta in it (ecc_host_weighted_robust_scale
//       takes delta from r / u),
// a pair whose loops ran no trip (count == 0) has {0, 1, 1, 0}.  The order {c, u, k, r}: sum_weighted_poses_kernel sums columns 0 and
// 1 of any column-form buffer, so a later pose-delta form calls it on the buffer and on the buffer + 2 columns.
// By construction: every w == 1.0f (delta = +inf) gives f == mu, so c and u have pairs_weighted_kernel's bits and k has u's; every
// mu == 1.0f gives f == w, so {c, k, r} have pairs_robust_kernel's {c, u, r} bits and u is 1.0f; both give pairs_kernel's bits.
// Both kernels run wholly on the frames of ecc_pair_forms.h: form_main_sums and form_reference_sums with every piece
// below them.  WeightedRobustForm's trip is WeightedForm's 8 gathers followed by RobustForm's weights; five per-lane float64 sums in
// trip order.  loss and delta are launch-uniform kernel arguments and the loss a uniform select, not a template parameter.  Plain
// vector loads and stores only: no atomics, no inline assembly.
// Not here (include/ecc_hip.h): the pose-delta and transform batches of this form (they need no kernel beyond this one); range, group
// and RCCL forms; the correlation cost; Tukey's biweight; a variance form.
#include <hip/hip_runtime.h>
#include <float.h>

#include "ecc_layout.h"
#include "ecc_pair_forms.h"
#include "ecc_robust_weight.h"

namespace {

// the five per-lane sums: the value, the weight mass, the mass the loss keeps, the weighted raw squares, the sample count
enum { VALUE, MASS, KEPT, RAW, COUNT, WEIGHTED_ROBUST_SUMS };

// the trips of the three loop kinds (ecc_pair_forms.h): the 4 data gathers and, at the same taps of the weight copies, 4 more; the
// residuals of the + and the - sample, their loss weights, the sums
struct WeightedRobustForm : PairFormDefaults {
    const EccWeightedRobustParams& g;
    double (&acc)[WEIGHTED_ROBUST_SUMS];
    RobustLoss L;                   // the launch-uniform loss, in scalar registers
    GlobalBytes w0, w1;             // the weight copies of the loop's two views (wave-uniform)
    GlobalFloats d0, d1, rw0, rw1;  // the reference loop's slabs: data and weights

    __device__ __forceinline__ WeightedRobustForm(const EccWeightedRobustParams& g, double (&acc)[WEIGHTED_ROBUST_SUMS]) : g(g), acc(acc) {}

    __device__ __forceinline__ void begin(const EccPairParams&, int, int)
    {
        L = {__builtin_amdgcn_readfirstlane(g.loss), uniformf(g.delta), uniformf(g.inv_delta)};
    }

    // the sums of a trip beside its value
    __device__ __forceinline__ void add(float value, float mu_p, float mu_m, float f_p, float f_m, float dp, float dm)
    {
        acc[VALUE] += (double)value;
        acc[MASS] += (double)(mu_p + mu_m);
        acc[KEPT] += (double)(f_p + f_m);
        acc[RAW] += (double)(mu_p * (dp * dp)) + (double)(mu_m * (dm * dm));
        acc[COUNT] += 2.0;
    }

    __device__ __forceinline__ void poly_begin(const SlabView sv0, const SlabView sv1, float, float)
    {
        w0 = sv0.origin + g.paired_channel_bytes, w1 = sv1.origin + g.paired_channel_bytes;
    }

    __device__ __forceinline__ void poly_trip(const SlabView sv0, const SlabView sv1, const SampleTap t0p, const SampleTap t1p,
                                              const SampleTap t0m, const SampleTap t1m, float rel_sign, float w06_dkappa)
    {
        const float v0p = sample_tap_value(sv0.origin, t0p), v1p = sample_tap_value(sv1.origin, t1p);
        const float v0m = sample_tap_value(sv0.origin, t0m), v1m = sample_tap_value(sv1.origin, t1m);
        const float mu_p = sample_tap_value(w0, t0p) * sample_tap_value(w1, t1p);  // unsigned, whatever the folds
        const float mu_m = sample_tap_value(w0, t0m) * sample_tap_value(w1, t1m);
        const float dp = fmaf(v1p, rel_sign, v0p), dm = fmaf(v1m, rel_sign, v0m);
        const float f_p = mu_p * robust_weight(L, dp), f_m = mu_m * robust_weight(L, dm);
        add(fmaf(f_p * dp, dp, (f_m * dm) * dm) * w06_dkappa, mu_p, mu_m, f_p, f_m, dp, dm);
    }

    template <int PITCH4>
    __device__ __forceinline__ void exact_begin(const SlabView sv0, const SlabView sv1)
    {
        w0 = sv0.origin + channel_bytes<PITCH4>(g), w1 = sv1.origin + channel_bytes<PITCH4>(g);
    }

    template <bool DERIV, int PITCH4>
    __device__ __forceinline__ void exact_trip(const SlabView sv0, const SlabView sv1, const LineTap t0p, const LineTap t1p, const LineTap t0m,
                                               const LineTap t1m, float w06, float dkappa)
    {
        const unsigned o0p = line_tap_offset(t0p, sv0), o1p = line_tap_offset(t1p, sv1);
        const unsigned o0m = line_tap_offset(t0m, sv0), o1m = line_tap_offset(t1m, sv1);
        const float v0p = line_tap_finish<DERIV>(line_footprint(sv0.origin, o0p), t0p), v1p = line_tap_finish<DERIV>(line_footprint(sv1.origin, o1p), t1p);
        const float v0m = line_tap_finish<DERIV>(line_footprint(sv0.origin, o0m), t0m), v1m = line_tap_finish<DERIV>(line_footprint(sv1.origin, o1m), t1m);
        const float mu_p = line_tap_finish<false>(line_footprint(w0, o0p), t0p) * line_tap_finish<false>(line_footprint(w1, o1p), t1p);
        const float mu_m = line_tap_finish<false>(line_footprint(w0, o0m), t0m) * line_tap_finish<false>(line_footprint(w1, o1m), t1m);
        const float dp = v0p - v1p, dm = v0m - v1m;
        const float f_p = mu_p * robust_weight(L, dp), f_m = mu_m * robust_weight(L, dm);
        add((((f_p * dp) * dp + (f_m * dm) * dm) * w06) * dkappa, mu_p, mu_m, f_p, f_m, dp, dm);  // ref: ...RadonIntermediate.cu:112,269,254
    }

    __device__ __forceinline__ void reference_begin(const EccPairParams& p, int iD0, int iD1)
    {
        d0 = (GlobalFloats)p.slabs[iD0], d1 = (GlobalFloats)p.slabs[iD1];
        rw0 = (GlobalFloats)p.slabs[(long long)p.n_views + iD0], rw1 = (GlobalFloats)p.slabs[(long long)p.n_views + iD1];
        begin(p, iD0, iD1);
    }

    __device__ __forceinline__ void reference_trip(const EccPairParams& p, bool deriv, const PlainTap t0p, const PlainTap t1p,
                                                   const PlainTap t0m, const PlainTap t1m, float w06, float dkappa)
    {
        const float v0p = plain_tap_value(t0p, d0, p.pitch, p.n_alpha, p.n_t, deriv), v1p = plain_tap_value(t1p, d1, p.pitch, p.n_alpha, p.n_t, deriv);
        const float v0m = plain_tap_value(t0m, d0, p.pitch, p.n_alpha, p.n_t, deriv), v1m = plain_tap_value(t1m, d1, p.pitch, p.n_alpha, p.n_t, deriv);
        const float mu_p = plain_tap_value(t0p, rw0, p.pitch, p.n_alpha, p.n_t, false) * plain_tap_value(t1p, rw1, p.pitch, p.n_alpha, p.n_t, false);
        const float mu_m = plain_tap_value(t0m, rw0, p.pitch, p.n_alpha, p.n_t, false) * plain_tap_value(t1m, rw1, p.pitch, p.n_alpha, p.n_t, false);
        const float dp = v0p - v1p, dm = v0m - v1m;
        const float f_p = mu_p * robust_weight(L, dp), f_m = mu_m * robust_weight(L, dm);
        const float consistency = ((f_p * dp) * dp + (f_m * dm) * dm) * w06;  // ref: ...RadonIntermediate.cu:112,254
        add(consistency * dkappa, mu_p, mu_m, f_p, f_m, dp, dm);              // ref: ...RadonIntermediate.cu:269
    }
};

// The pair's four entries from the wave's sums (lane 0): c, u, k, r into columns 0 .. 3.
__device__ __forceinline__ void store_weighted_robust(const EccWeightedRobustParams& g, long long local, const double (&acc)[WEIGHTED_ROBUST_SUMS])
{
    const bool any = acc[COUNT] > 0.0;
    g.values[local] = (float)acc[VALUE];  // pair_value<false>; no trip: 0
    g.values[g.col_stride + local] = any ? (float)(acc[MASS] / acc[COUNT]) : 1.0f;
    g.values[2 * g.col_stride + local] = any ? (float)(acc[KEPT] / acc[COUNT]) : 1.0f;
    g.values[3 * g.col_stride + local] = any ? (float)(acc[RAW] / acc[COUNT]) : 0.0f;
}

// Registers: the 8 gathers of a kappa step as in pairs_weighted_kernel, 10 accumulator registers against its 6, the
// loss in three scalar registers; tests/test_weighted_robust_abi.py pins the plan and what was built.
template <bool DERIV>
__global__ __launch_bounds__(PK_MAIN_THREADS) void pairs_weighted_robust_kernel(EccPairParams p, EccWeightedRobustParams g)
{
    double acc[WEIGHTED_ROBUST_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    WeightedRobustForm form(g, acc);
    long long local;
    if (form_main_sums<DERIV>(p, form, acc, local)) store_weighted_robust(g, local, acc);
}

// ---- ECC_SAMPLING_REFERENCE -------------------------------------------------------------------------
template <int SPLIT>
__global__ __launch_bounds__(PK_THREADS) void pairs_weighted_robust_reference_kernel(EccPairParams p, EccWeightedRobustParams g)
{
    double acc[WEIGHTED_ROBUST_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    WeightedRobustForm form(g, acc);
    long long local;
    if (form_reference_sums<SPLIT>(p, form, acc, local)) store_weighted_robust(g, local, acc);
}

}  // namespace

// The four entries {c, u, k, r} of every pair of the launch p (records of ecc_launch_k01 for the same parameters, earlier on the same
// stream; first = 0, no slots) into g->values; the metric's dtrs are the data of the n_views views, then their line weights.
// p->indices may be set (an index list): the kernels do not read it, the record carries both Radon-intermediate indices, which must
// lie in [0, n_views) -- the weights of a sample come from dtr n_views + that index (the host calls check both, ecc_weighted_robust.hip).
extern "C" hipError_t ecc_launch_pairs_weighted_robust(const EccPairParams* p, const EccWeightedRobustParams* g, hipStream_t stream)
{
    if (p->count <= 0) return hipSuccess;
    if (p->use_corr || p->record_slots || p->skip_enabled || !g->values || g->col_stride < p->count || (g->col_stride & 3) ||
        g->loss < ECC_ROBUST_HUBER || g->loss > ECC_ROBUST_GEMAN_MCCLURE || !(g->delta > 0.f))
        return hipErrorInvalidValue;
    return launch_pair_form(*p, *g, stream, pairs_weighted_robust_reference_kernel<4>, pairs_weighted_robust_reference_kernel<1>,
                            pairs_weighted_robust_kernel<true>, pairs_weighted_robust_kernel<false>);
}
