// variance_robust_kernel.hip -- the metric with inverse-variance sample weights AND a per-sample robust loss in sigma units (gfx950).
//
// A metric over 2 n Radon intermediates as variance_kernel.hip takes it: dtr i is the data of view i, dtr n + i its VARIANCE FIELD
// V_i on the same bin grid.  The variance says how noisy a sample is known to be (a photon-starved line); the loss takes care of what
// nobody flagged (an instrument).  A loss on the raw residual rejects a line that is merely noisy, and known to be; the M-estimator
// for data of known variance applies the loss to the STUDENTISED residual z = d / sigma with sigma^2 = V_i + V_j, and delta is then
// "so many sigmas".  For the pair i < j every +-kappa sample has the positions, kappa range and sampling mode of pairs_kernel's
// evaluation, d = the difference of the two signed data samples as pairs_kernel forms it, and, every line one float32 operation,
//   s   = V_i(sample) + V_j(sample)       UNSIGNED bilinear samples at the data's taps, as in variance_kernel.hip
//   sc  = s < floor ? floor : s
//   om  = 1.0f / sc                       the correctly rounded IEEE division (the compiler's expansion; no reciprocal intrinsic)
//   a   = fabsf(d)
//   huber, truncated    thr = delta * sqrtf(sc);  t = fminf(1.0f, thr / a);   w = t * (2.0f - t)  |  t * t
//   geman-mcclure       q = a * inv_delta;        w = 1.0f / fmaf(q * om, q, 1.0f)
//   f   = om * w
// sqrtf is the correctly rounded one (v_sqrt_f32 and the compiler's fix-up; no intrinsic, no fast-math flag).  |z| <= delta is
// written as |d| <= delta sqrt(sc) so that sc == 1.0f leaves robust_kernel.hip's expressions as they are.  Per kappa step the value
// term is weighted_robust_kernel.hip's with f as it stands there:
//   polynomial loops             fmaf(f_p * dp, dp, (f_m * dm) * dm) * w06_dkappa
//   exact and reference loops    (((f_p * dp) * dp + (f_m * dm) * dm) * K0[6]) * dkappa
// Beside the value each lane adds (double)(om_p + om_m), the weight mass, (double)(f_p + f_m), the mass the loss keeps,
// (double)(om_p * (dp * dp)) + (double)(om_m * (dm * dm)), the squared studentised residuals (products in float32), and 2.0, the
// sample count.  Per pair, four columns
//   c = the float32 value, as pairs_kernel stores it,
//   u = (float)(mass / count), the MEAN WEIGHT of variance_kernel.hip,
//   k = (float)(kept / count), the weight mass the loss keeps: k <= u, k / u is the inlier mass,
//   r = (float)(raw / count), the mean squared studentised residual, a reduced chi^2 of the pair: no loss and no delta in it
//       (ecc_host_variance_robust_scale takes delta from it),
// a pair whose loops ran no trip (count == 0) has {0, 1, 1, 0}.  The order {c, u, k, r} is the weighted-robust form's, so the S = 3
// sums of form_sums_kernel.hip serve the batches as they stand.
// By construction: delta = +inf gives w == 1.0f and f == om, so {c, u} have pairs_variance_kernel's bits and k has u's; V == 0.5f
// with floor <= 1 gives sc == om == 1.0f, thr == delta, q * om == q and f == w, so {c, k, r} have pairs_robust_kernel's {c, u, r}
// bits and u is 1.0f; both give pairs_kernel's bits; all V and the floor x 4 with delta x 1/2 leave thr and q * om * q as they are
// and quarter om, so every column is a quarter of itself, exactly.
// Both kernels run wholly on the frames of ecc_pair_forms.h: form_main_sums and form_reference_sums with every piece
// below them.  VarianceRobustForm's trip is VarianceForm's 8 gathers and reciprocals followed by the studentised weights; five
// per-lane float64 sums in trip order.  loss, delta and floor are launch-uniform kernel arguments and the loss a uniform select, not
// a template parameter; the weight itself is ecc_studentised_weight.h's, shared with the map of this form
// (variance_robust_map_kernel.hip).  Plain vector loads and stores only: no atomics, no inline assembly, no LDS in the main kernels.
// Not here (include/ecc_hip.h): base columns kept between calls; range, group and RCCL forms; the correlation cost; a
// covariance-aware model for derivative data.
#include <hip/hip_runtime.h>
#include <float.h>

#include "ecc_layout.h"
#include "ecc_pair_forms.h"
#include "ecc_studentised_weight.h"

namespace {

// the five per-lane sums: the value, the weight mass, the mass the loss keeps, the squared studentised residuals, the sample count
enum { VALUE, MASS, KEPT, RAW, COUNT, VARIANCE_ROBUST_SUMS };

// the trips of the three loop kinds (ecc_pair_forms.h): the 4 data gathers and, at the same taps of the variance copies, 4 more; the
// residuals of the + and the - sample, their studentised weights, the sums
struct VarianceRobustForm : PairFormDefaults {
    const EccVarianceRobustParams& g;
    double (&acc)[VARIANCE_ROBUST_SUMS];
    StudentisedLoss L;              // the launch-uniform loss and floor, in scalar registers
    GlobalBytes w0, w1;             // the variance copies of the loop's two views (wave-uniform)
    GlobalFloats d0, d1, rw0, rw1;  // the reference loop's slabs: data and variances

    __device__ __forceinline__ VarianceRobustForm(const EccVarianceRobustParams& g, double (&acc)[VARIANCE_ROBUST_SUMS]) : g(g), acc(acc) {}

    __device__ __forceinline__ void begin(const EccPairParams&, int, int)
    {
        L = {__builtin_amdgcn_readfirstlane(g.loss), uniformf(g.delta), uniformf(g.inv_delta), uniformf(g.floor)};
    }

    // the sums of a trip beside its value
    __device__ __forceinline__ void add(float value, const StudentisedWeight p, const StudentisedWeight m, float dp, float dm)
    {
        acc[VALUE] += (double)value;
        acc[MASS] += (double)(p.om + m.om);
        acc[KEPT] += (double)(p.f + m.f);
        acc[RAW] += (double)(p.om * (dp * dp)) + (double)(m.om * (dm * dm));
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
        const float s0p = sample_tap_value(w0, t0p), s1p = sample_tap_value(w1, t1p);  // unsigned, whatever the folds
        const float s0m = sample_tap_value(w0, t0m), s1m = sample_tap_value(w1, t1m);
        const float dp = fmaf(v1p, rel_sign, v0p), dm = fmaf(v1m, rel_sign, v0m);
        const StudentisedWeight p = studentised_weight(L, s0p, s1p, dp), m = studentised_weight(L, s0m, s1m, dm);
        add(fmaf(p.f * dp, dp, (m.f * dm) * dm) * w06_dkappa, p, m, dp, dm);
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
        const float s0p = line_tap_finish<false>(line_footprint(w0, o0p), t0p), s1p = line_tap_finish<false>(line_footprint(w1, o1p), t1p);
        const float s0m = line_tap_finish<false>(line_footprint(w0, o0m), t0m), s1m = line_tap_finish<false>(line_footprint(w1, o1m), t1m);
        const float dp = v0p - v1p, dm = v0m - v1m;
        const StudentisedWeight p = studentised_weight(L, s0p, s1p, dp), m = studentised_weight(L, s0m, s1m, dm);
        add((((p.f * dp) * dp + (m.f * dm) * dm) * w06) * dkappa, p, m, dp, dm);  // ref: ...RadonIntermediate.cu:112,269,254
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
        const float s0p = plain_tap_value(t0p, rw0, p.pitch, p.n_alpha, p.n_t, false), s1p = plain_tap_value(t1p, rw1, p.pitch, p.n_alpha, p.n_t, false);
        const float s0m = plain_tap_value(t0m, rw0, p.pitch, p.n_alpha, p.n_t, false), s1m = plain_tap_value(t1m, rw1, p.pitch, p.n_alpha, p.n_t, false);
        const float dp = v0p - v1p, dm = v0m - v1m;
        const StudentisedWeight wp = studentised_weight(L, s0p, s1p, dp), wm = studentised_weight(L, s0m, s1m, dm);
        const float consistency = ((wp.f * dp) * dp + (wm.f * dm) * dm) * w06;  // ref: ...RadonIntermediate.cu:112,254
        add(consistency * dkappa, wp, wm, dp, dm);                              // ref: ...RadonIntermediate.cu:269
    }
};

// The pair's four entries from the wave's sums (lane 0): c, u, k, r into columns 0 .. 3.
__device__ __forceinline__ void store_variance_robust(const EccVarianceRobustParams& g, long long local, const double (&acc)[VARIANCE_ROBUST_SUMS])
{
    const bool any = acc[COUNT] > 0.0;
    g.values[local] = (float)acc[VALUE];  // pair_value<false>; no trip: 0
    g.values[g.col_stride + local] = any ? (float)(acc[MASS] / acc[COUNT]) : 1.0f;
    g.values[2 * g.col_stride + local] = any ? (float)(acc[KEPT] / acc[COUNT]) : 1.0f;
    g.values[3 * g.col_stride + local] = any ? (float)(acc[RAW] / acc[COUNT]) : 0.0f;
}

// Registers: pairs_weighted_robust_kernel's live values plus the temporaries of two square roots and two more
// divisions, the loss and the floor in four scalar registers; tests/test_variance_robust_abi.py pins the plan and what was built.
template <bool DERIV>
__global__ __launch_bounds__(PK_MAIN_THREADS) void pairs_variance_robust_kernel(EccPairParams p, EccVarianceRobustParams g)
{
    double acc[VARIANCE_ROBUST_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    VarianceRobustForm form(g, acc);
    long long local;
    if (form_main_sums<DERIV>(p, form, acc, local)) store_variance_robust(g, local, acc);
}

// ---- ECC_SAMPLING_REFERENCE -------------------------------------------------------------------------
template <int SPLIT>
__global__ __launch_bounds__(PK_THREADS) void pairs_variance_robust_reference_kernel(EccPairParams p, EccVarianceRobustParams g)
{
    double acc[VARIANCE_ROBUST_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    VarianceRobustForm form(g, acc);
    long long local;
    if (form_reference_sums<SPLIT>(p, form, acc, local)) store_variance_robust(g, local, acc);
}

}  // namespace

// The four entries {c, u, k, r} of every pair of the launch p (records of ecc_launch_k01 for the same parameters, earlier on the same
// stream; first = 0, no slots) into g->values; the metric's dtrs are the data of the n_views views, then their variance fields.
// p->indices may be set (an index list, a batch's grid): the kernels do not read it, the record carries both Radon-intermediate
// indices, which must lie in [0, n_views) -- the variance of a sample comes from dtr n_views + that index (the host calls check both,
// ecc_variance_robust.hip).  g->floor: finite, > 0; g->delta > 0, +infinity allowed.
extern "C" hipError_t ecc_launch_pairs_variance_robust(const EccPairParams* p, const EccVarianceRobustParams* g, hipStream_t stream)
{
    if (p->count <= 0) return hipSuccess;
    if (p->use_corr || p->record_slots || p->skip_enabled || !g->values || g->col_stride < p->count || (g->col_stride & 3) ||
        g->loss < ECC_ROBUST_HUBER || g->loss > ECC_ROBUST_GEMAN_MCCLURE || !(g->delta > 0.f))
        return hipErrorInvalidValue;
    if (!(g->floor > 0.0f) || !(g->floor <= FLT_MAX)) return hipErrorInvalidValue;
    return launch_pair_form(*p, *g, stream, pairs_variance_robust_reference_kernel<4>, pairs_variance_robust_reference_kernel<1>,
                            pairs_variance_robust_kernel<true>, pairs_variance_robust_kernel<false>);
}
