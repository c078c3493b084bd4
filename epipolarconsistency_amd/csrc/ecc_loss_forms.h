// ecc_loss_forms.h -- the trips of the pair forms that carry a per-sample robust loss, stated once for their evaluation kernels and
// their map kernels.  For the kernel files, behind ecc_pair_forms.h, whose frames call the members below.
//
//   RobustForm<G, Map>             one intermediate per view, four sums, three columns {c, u, r}: robust_kernel.hip (Map = NoMap) and
//                                  robust_map_kernel.hip (Map = MapDeposits)
//   FieldLossForm<G, Rule, Map>    2 n channel-major intermediates -- the data and a second field per view --, five sums, four
//                                  columns {c, u, k, r}; the Rule says what the two field samples of a tap pair become:
//       LineWeightRule      mu = W_i * W_j, w = robust_weight(L, d), f = mu * w: weighted_robust_kernel.hip,
//                           weighted_robust_map_kernel.hip
//       StudentisedRule     studentised_weight(L, V_i, V_j, d) (ecc_studentised_weight.h): variance_robust_kernel.hip,
//                           variance_robust_map_kernel.hip
// What each form computes is in the head comment of its evaluation kernel file.  G is the launch's parameter struct (the kernel
// argument; its layout is the file's own), Map the deposit policy: NoMap below has the four hooks empty, MapDeposits
// (ecc_robust_map.h) deposits every sample's footprint behind the sums.  A map kernel therefore returns its evaluation's bits by
// construction: both run the statements below.
// THE ORDER OF STATEMENTS is the one the six kernel files were built with (as in ecc_pair_forms.h, the compiler's output follows it):
// the data gathers, the field gathers, the rule's combination of the two field samples directly behind them, the residuals, the
// weights, the sums, the deposits.
#ifndef ECC_LOSS_FORMS_H
#define ECC_LOSS_FORMS_H

#include "ecc_pair_forms.h"
#include "ecc_robust_weight.h"
#include "ecc_studentised_weight.h"

namespace {

// The deposit policy of an evaluation: none.  The hooks of a policy, in the order a form calls them: map_begin once per pair (from
// begin), then one per trip of the three loop kinds, with the trip's four taps, the loss weights w of the + and the - sample and the
// factor mu their deposits are multiplied by.
struct NoMap {
    template <class G>
    __device__ __forceinline__ void map_begin(const G&, const EccPairParams&, int, int)
    {
    }
    __device__ __forceinline__ void map_poly(const SampleTap, const SampleTap, const SampleTap, const SampleTap, float, float, float, float) const {}
    template <int PITCH4>
    __device__ __forceinline__ void map_exact(const SlabView, const SlabView, const LineTap, const LineTap, const LineTap, const LineTap, float,
                                              float, float, float) const
    {
    }
    __device__ __forceinline__ void map_plain(const EccPairParams&, const PlainTap, const PlainTap, const PlainTap, const PlainTap, float, float,
                                              float, float) const
    {
    }
};

// ---- the loss alone ------------------------------------------------------------------------------------------------------------
// the four per-lane sums: the value, the weight mass, the raw squares, the sample count
enum { VALUE, MASS, RAW, COUNT, ROBUST_SUMS };

// the trips of the three loop kinds (ecc_pair_forms.h): 4 gathers, the residuals of the + and the - sample, their weights, the sums
template <class G, class Map>
struct RobustForm : PairFormDefaults, Map {
    const G& g;
    double (&acc)[ROBUST_SUMS];
    RobustLoss L;         // the launch-uniform loss, in scalar registers
    GlobalFloats d0, d1;  // the reference loop's slabs

    __device__ __forceinline__ RobustForm(const G& g, double (&acc)[ROBUST_SUMS]) : g(g), acc(acc) {}

    __device__ __forceinline__ void begin(const EccPairParams& p, int iD0, int iD1)
    {
        L = {__builtin_amdgcn_readfirstlane(g.loss), uniformf(g.delta), uniformf(g.inv_delta)};
        this->map_begin(g, p, iD0, iD1);
    }

    // the sums of a trip beside its value
    __device__ __forceinline__ void add(float value, float w_p, float w_m, float dp, float dm)
    {
        acc[VALUE] += (double)value;
        acc[MASS] += (double)(w_p + w_m);
        acc[RAW] += (double)(dp * dp) + (double)(dm * dm);
        acc[COUNT] += 2.0;
    }

    __device__ __forceinline__ void poly_trip(const SlabView sv0, const SlabView sv1, const SampleTap t0p, const SampleTap t1p,
                                              const SampleTap t0m, const SampleTap t1m, float rel_sign, float w06_dkappa)
    {
        const float v0p = sample_tap_value(sv0.origin, t0p), v1p = sample_tap_value(sv1.origin, t1p);
        const float v0m = sample_tap_value(sv0.origin, t0m), v1m = sample_tap_value(sv1.origin, t1m);
        const float dp = fmaf(v1p, rel_sign, v0p), dm = fmaf(v1m, rel_sign, v0m);
        const float w_p = robust_weight(L, dp), w_m = robust_weight(L, dm);
        add(fmaf(w_p * dp, dp, (w_m * dm) * dm) * w06_dkappa, w_p, w_m, dp, dm);
        this->map_poly(t0p, t1p, t0m, t1m, w_p, w_m, 1.0f, 1.0f);
    }

    template <bool DERIV, int PITCH4>
    __device__ __forceinline__ void exact_trip(const SlabView sv0, const SlabView sv1, const LineTap t0p, const LineTap t1p, const LineTap t0m,
                                               const LineTap t1m, float w06, float dkappa)
    {
        const auto tap = [](const LineTap& t) { return line_tap_finish<DERIV>(line_footprint((GlobalBytes)t.ptr, 0u), t); };
        const float v0p = tap(t0p), v1p = tap(t1p), v0m = tap(t0m), v1m = tap(t1m);
        const float dp = v0p - v1p, dm = v0m - v1m;
        const float w_p = robust_weight(L, dp), w_m = robust_weight(L, dm);
        add((((w_p * dp) * dp + (w_m * dm) * dm) * w06) * dkappa, w_p, w_m, dp, dm);  // ref: ...RadonIntermediate.cu:112,269,254
        this->template map_exact<PITCH4>(sv0, sv1, t0p, t1p, t0m, t1m, w_p, w_m, 1.0f, 1.0f);
    }

    __device__ __forceinline__ void reference_begin(const EccPairParams& p, int iD0, int iD1)
    {
        d0 = (GlobalFloats)p.slabs[iD0];
        d1 = (GlobalFloats)p.slabs[iD1];
        begin(p, iD0, iD1);
    }

    __device__ __forceinline__ void reference_trip(const EccPairParams& p, bool deriv, const PlainTap t0p, const PlainTap t1p,
                                                   const PlainTap t0m, const PlainTap t1m, float w06, float dkappa)
    {
        const float v0p = plain_tap_value(t0p, d0, p.pitch, p.n_alpha, p.n_t, deriv), v1p = plain_tap_value(t1p, d1, p.pitch, p.n_alpha, p.n_t, deriv);
        const float v0m = plain_tap_value(t0m, d0, p.pitch, p.n_alpha, p.n_t, deriv), v1m = plain_tap_value(t1m, d1, p.pitch, p.n_alpha, p.n_t, deriv);
        const float dp = v0p - v1p, dm = v0m - v1m;
        const float w_p = robust_weight(L, dp), w_m = robust_weight(L, dm);
        const float consistency = ((w_p * dp) * dp + (w_m * dm) * dm) * w06;  // ref: ...RadonIntermediate.cu:112,254
        add(consistency * dkappa, w_p, w_m, dp, dm);                          // ref: ...RadonIntermediate.cu:269
        this->map_plain(p, t0p, t1p, t0m, t1m, w_p, w_m, 1.0f, 1.0f);
    }
};

// The pair's three entries from the wave's sums (lane 0): c into column 0, u into column 1, r into column 2.
template <class G>
__device__ __forceinline__ void store_robust(const G& g, long long local, const double (&acc)[ROBUST_SUMS])
{
    const bool any = acc[COUNT] > 0.0;
    g.values[local] = (float)acc[VALUE];  // pair_value<false>; no trip: 0
    g.values[g.col_stride + local] = any ? (float)(acc[MASS] / acc[COUNT]) : 1.0f;
    g.values[2 * g.col_stride + local] = any ? (float)(acc[RAW] / acc[COUNT]) : 0.0f;
}

// ---- the loss on a metric with a second field per view -------------------------------------------------------------------------
// The two rules.  load(g): the launch-uniform part, into scalar registers (from begin).  field(s0, s1): what is kept of the two
// UNSIGNED field samples of a tap pair, formed right behind the gathers.  weight(field, d): {om, f, w} of the sample with the
// residual d -- om what the sample weighs without the loss, w the loss weight, f = om * w.  deposit_mu(weight): the factor of the
// sample's deposits.

// line weights: the loss takes the RAW residual, a sample counts in the maps as far as the metric counted it
struct LineWeightRule {
    RobustLoss L;

    template <class G>
    __device__ __forceinline__ void load(const G& g)
    {
        L = {__builtin_amdgcn_readfirstlane(g.loss), uniformf(g.delta), uniformf(g.inv_delta)};
    }
    static __device__ __forceinline__ float field(float s0, float s1) { return s0 * s1; }
    __device__ __forceinline__ StudentisedWeight weight(float mu, float d) const
    {
        const float w = robust_weight(L, d);
        return {mu, mu * w, w};
    }
    static __device__ __forceinline__ float deposit_mu(const StudentisedWeight& x) { return x.om; }
};

// variance fields: the loss takes the studentised residual, the maps are in count units (the literal 1.0f: deposit_footprint's
// multiply and test are dropped)
struct StudentisedRule {
    struct Variances {
        float a, b;
    };
    StudentisedLoss L;

    template <class G>
    __device__ __forceinline__ void load(const G& g)
    {
        L = {__builtin_amdgcn_readfirstlane(g.loss), uniformf(g.delta), uniformf(g.inv_delta), uniformf(g.floor)};
    }
    static __device__ __forceinline__ Variances field(float s0, float s1) { return {s0, s1}; }
    __device__ __forceinline__ StudentisedWeight weight(const Variances v, float d) const { return studentised_weight(L, v.a, v.b, d); }
    static __device__ __forceinline__ float deposit_mu(const StudentisedWeight&) { return 1.0f; }
};

// the five per-lane sums: the value, the weight mass, the mass the loss keeps, the weighted squared residuals, the sample count
enum { FL_VALUE, FL_MASS, FL_KEPT, FL_RAW, FL_COUNT, FIELD_LOSS_SUMS };

// the trips of the three loop kinds (ecc_pair_forms.h): the 4 data gathers and, at the same taps of the field copies, 4 more; the
// residuals of the + and the - sample, their weights, the sums
template <class G, class Rule, class Map>
struct FieldLossForm : PairFormDefaults, Map {
    const G& g;
    double (&acc)[FIELD_LOSS_SUMS];
    Rule rule;                      // with the launch-uniform loss, in scalar registers
    GlobalBytes w0, w1;             // the field copies of the loop's two views (wave-uniform)
    GlobalFloats d0, d1, rw0, rw1;  // the reference loop's slabs: data and fields

    __device__ __forceinline__ FieldLossForm(const G& g, double (&acc)[FIELD_LOSS_SUMS]) : g(g), acc(acc) {}

    __device__ __forceinline__ void begin(const EccPairParams& p, int iD0, int iD1)
    {
        rule.load(g);
        this->map_begin(g, p, iD0, iD1);
    }

    // the sums of a trip beside its value
    __device__ __forceinline__ void add(float value, const StudentisedWeight p, const StudentisedWeight m, float dp, float dm)
    {
        acc[FL_VALUE] += (double)value;
        acc[FL_MASS] += (double)(p.om + m.om);
        acc[FL_KEPT] += (double)(p.f + m.f);
        acc[FL_RAW] += (double)(p.om * (dp * dp)) + (double)(m.om * (dm * dm));
        acc[FL_COUNT] += 2.0;
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
        const auto fp = Rule::field(s0p, s1p), fm = Rule::field(s0m, s1m);
        const float dp = fmaf(v1p, rel_sign, v0p), dm = fmaf(v1m, rel_sign, v0m);
        const StudentisedWeight p = rule.weight(fp, dp), m = rule.weight(fm, dm);
        add(fmaf(p.f * dp, dp, (m.f * dm) * dm) * w06_dkappa, p, m, dp, dm);
        this->map_poly(t0p, t1p, t0m, t1m, p.w, m.w, Rule::deposit_mu(p), Rule::deposit_mu(m));
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
        const auto fp = Rule::field(s0p, s1p), fm = Rule::field(s0m, s1m);
        const float dp = v0p - v1p, dm = v0m - v1m;
        const StudentisedWeight p = rule.weight(fp, dp), m = rule.weight(fm, dm);
        add((((p.f * dp) * dp + (m.f * dm) * dm) * w06) * dkappa, p, m, dp, dm);  // ref: ...RadonIntermediate.cu:112,269,254
        this->template map_exact<PITCH4>(sv0, sv1, t0p, t1p, t0m, t1m, p.w, m.w, Rule::deposit_mu(p), Rule::deposit_mu(m));
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
        const auto fp = Rule::field(s0p, s1p), fm = Rule::field(s0m, s1m);
        const float dp = v0p - v1p, dm = v0m - v1m;
        const StudentisedWeight wp = rule.weight(fp, dp), wm = rule.weight(fm, dm);
        const float consistency = ((wp.f * dp) * dp + (wm.f * dm) * dm) * w06;  // ref: ...RadonIntermediate.cu:112,254
        add(consistency * dkappa, wp, wm, dp, dm);                              // ref: ...RadonIntermediate.cu:269
        this->map_plain(p, t0p, t1p, t0m, t1m, wp.w, wm.w, Rule::deposit_mu(wp), Rule::deposit_mu(wm));
    }
};

// The pair's four entries from the wave's sums (lane 0): c, u, k, r into columns 0 .. 3.
template <class G>
__device__ __forceinline__ void store_field_loss(const G& g, long long local, const double (&acc)[FIELD_LOSS_SUMS])
{
    const bool any = acc[FL_COUNT] > 0.0;
    g.values[local] = (float)acc[FL_VALUE];  // pair_value<false>; no trip: 0
    g.values[g.col_stride + local] = any ? (float)(acc[FL_MASS] / acc[FL_COUNT]) : 1.0f;
    g.values[2 * g.col_stride + local] = any ? (float)(acc[FL_KEPT] / acc[FL_COUNT]) : 1.0f;
    g.values[3 * g.col_stride + local] = any ? (float)(acc[FL_RAW] / acc[FL_COUNT]) : 0.0f;
}

// ---- the argument check the six launch functions share -------------------------------------------------------------------------
// no correlation cost, no record slots, no skip list; the columns there, wide enough and 16-byte aligned; a known loss; delta > 0
// (+infinity allowed)
template <class G>
inline bool loss_launch_ok(const EccPairParams& p, const G& g)
{
    return !(p.use_corr || p.record_slots || p.skip_enabled || !g.values || g.col_stride < p.count || (g.col_stride & 3) ||
             g.loss < ECC_ROBUST_HUBER || g.loss > ECC_ROBUST_GEMAN_MCCLURE || !(g.delta > 0.f));
}

}  // namespace

#endif
