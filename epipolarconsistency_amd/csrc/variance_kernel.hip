// variance_kernel.hip -- the metric with inverse-variance sample weights (gfx950).
//
// A metric over 2 n Radon intermediates, channel-major as for the weighted form (ecc_layout.h): dtr i is the data of view i, dtr
// n + i its VARIANCE FIELD V_i on the same bin grid (normally made with FILTER_NONE from the image of pixel variances: the variance
// of a line integral is the integral of the pixel variances along the line; any finite float is taken as it is).  For the pair
// i < j every +-kappa sample has the positions, kappa range and sampling mode of pairs_kernel's evaluation, d = the difference of
// the two signed data samples as pairs_kernel forms it, and
//   s     = V_i(sample) + V_j(sample)       one float32 add of two UNSIGNED bilinear samples taken at the same taps as the data
//   omega = 1.0f / (s < floor ? floor : s)  one correctly rounded IEEE float32 division (the compiler's expansion of 1.0f / x; no
//                                           reciprocal intrinsic, no fast-math flag: the float64 statement rests on it)
// The fold sign is NEVER applied to a variance sample (line_tap_finish<false>, plain_tap_value(.., false), the unsigned
// sample_tap_value without rel_sign).  Per kappa step the value term is weighted_kernel.hip's with omega in mu's place:
//   polynomial loops             fmaf(om_p * dp, dp, (om_m * dm) * dm) * w06_dkappa
//   exact and reference loops    (((om_p * dp) * dp + (om_m * dm) * dm) * K0[6]) * dkappa
// so with omega == 1.0f (V == 0.5f everywhere, floor <= 1) these are pairs_kernel's bits, and a power of two in omega scales c
// exactly.  Beside the value each lane adds (double)(om_p + om_m) and 2.0 per trip.  Per pair
//   c = the float32 value, as pairs_kernel stores it,
//   u = (float)(mass / count), the MEAN WEIGHT of the pair's samples; a pair whose loops ran no trip has c = 0 and u = 1.0f,
// stored as two columns like the weighted form's and summed by the same two-column sums (ecc_variance.hip divides the sums).
// Both kernels run wholly on the frames of ecc_pair_forms.h: VarianceForm's trip gathers the data footprint and,
// at the same tap of the variance copy, the variance footprint, 8 gathers per kappa step, forms both reciprocals as soon as the
// variance samples are there, and adds the value term, om_p + om_m and 2.0 to three per-lane float64 sums in trip order.  Plain
// vector loads and stores only: no atomics, no inline assembly.
// Not here (include/ecc_hip.h): range, group and RCCL forms; the variance form under the correlation cost or combined with the robust
// loss; a covariance-aware model for derivative data.
#include <hip/hip_runtime.h>
#include <float.h>

#include "ecc_layout.h"
#include "ecc_pair_forms.h"

namespace {

// the three per-lane sums: the value, the weight mass, the sample count
enum { VALUE, MASS, COUNT, VARIANCE_SUMS };

// the weight of a sample from the variance samples of its two lines
__device__ __forceinline__ float inverse_variance(float va, float vb, float floor)
{
    const float s = va + vb;
    return 1.0f / (s < floor ? floor : s);
}

// the trips of the three loop kinds (ecc_pair_forms.h): the 4 data gathers and, at the same taps of the variance copies, 4 more
struct VarianceForm : PairFormDefaults {
    const EccVarianceParams& g;
    double (&acc)[VARIANCE_SUMS];
    GlobalBytes w0, w1;                // the variance copies of the loop's two views (wave-uniform)
    GlobalFloats d0, d1, rw0, rw1;     // the reference loop's slabs: data and variances

    __device__ __forceinline__ VarianceForm(const EccVarianceParams& g, double (&acc)[VARIANCE_SUMS]) : g(g), acc(acc) {}

    // the sums of a trip beside its value
    __device__ __forceinline__ void add(float om_p, float om_m)
    {
        acc[MASS] += (double)(om_p + om_m);
        acc[COUNT] += 2.0;
    }

    __device__ __forceinline__ void poly_begin(const SlabView sv0, const SlabView sv1, float, float)
    {
        w0 = sv0.origin + g.paired_channel_bytes, w1 = sv1.origin + g.paired_channel_bytes;
    }

    __device__ __forceinline__ void poly_trip(const SlabView sv0, const SlabView sv1, const SampleTap t0p, const SampleTap t1p,
                                              const SampleTap t0m, const SampleTap t1m, float rel_sign, float w06_dkappa)
    {
        const float om_p = inverse_variance(sample_tap_value(w0, t0p), sample_tap_value(w1, t1p), g.floor);  // unsigned, whatever the folds
        const float om_m = inverse_variance(sample_tap_value(w0, t0m), sample_tap_value(w1, t1m), g.floor);
        const float v0p = sample_tap_value(sv0.origin, t0p), v1p = sample_tap_value(sv1.origin, t1p);
        const float v0m = sample_tap_value(sv0.origin, t0m), v1m = sample_tap_value(sv1.origin, t1m);
        const float dp = fmaf(v1p, rel_sign, v0p), dm = fmaf(v1m, rel_sign, v0m);
        acc[VALUE] += (double)(fmaf(om_p * dp, dp, (om_m * dm) * dm) * w06_dkappa);
        add(om_p, om_m);
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
        const float om_p = inverse_variance(line_tap_finish<false>(line_footprint(w0, o0p), t0p), line_tap_finish<false>(line_footprint(w1, o1p), t1p), g.floor);
        const float om_m = inverse_variance(line_tap_finish<false>(line_footprint(w0, o0m), t0m), line_tap_finish<false>(line_footprint(w1, o1m), t1m), g.floor);
        const float v0p = line_tap_finish<DERIV>(line_footprint(sv0.origin, o0p), t0p), v1p = line_tap_finish<DERIV>(line_footprint(sv1.origin, o1p), t1p);
        const float v0m = line_tap_finish<DERIV>(line_footprint(sv0.origin, o0m), t0m), v1m = line_tap_finish<DERIV>(line_footprint(sv1.origin, o1m), t1m);
        const float dp = v0p - v1p, dm = v0m - v1m;
        acc[VALUE] += (double)((((om_p * dp) * dp + (om_m * dm) * dm) * w06) * dkappa);  // ref: ...RadonIntermediate.cu:112,269,254
        add(om_p, om_m);
    }

    __device__ __forceinline__ void reference_begin(const EccPairParams& p, int iD0, int iD1)
    {
        d0 = (GlobalFloats)p.slabs[iD0], d1 = (GlobalFloats)p.slabs[iD1];
        rw0 = (GlobalFloats)p.slabs[(long long)p.n_views + iD0], rw1 = (GlobalFloats)p.slabs[(long long)p.n_views + iD1];
    }

    __device__ __forceinline__ void reference_trip(const EccPairParams& p, bool deriv, const PlainTap t0p, const PlainTap t1p,
                                                   const PlainTap t0m, const PlainTap t1m, float w06, float dkappa)
    {
        const float v0p = plain_tap_value(t0p, d0, p.pitch, p.n_alpha, p.n_t, deriv), v1p = plain_tap_value(t1p, d1, p.pitch, p.n_alpha, p.n_t, deriv);
        const float v0m = plain_tap_value(t0m, d0, p.pitch, p.n_alpha, p.n_t, deriv), v1m = plain_tap_value(t1m, d1, p.pitch, p.n_alpha, p.n_t, deriv);
        const float om_p = inverse_variance(plain_tap_value(t0p, rw0, p.pitch, p.n_alpha, p.n_t, false), plain_tap_value(t1p, rw1, p.pitch, p.n_alpha, p.n_t, false), g.floor);
        const float om_m = inverse_variance(plain_tap_value(t0m, rw0, p.pitch, p.n_alpha, p.n_t, false), plain_tap_value(t1m, rw1, p.pitch, p.n_alpha, p.n_t, false), g.floor);
        const float dp = v0p - v1p, dm = v0m - v1m;
        const float consistency = ((om_p * dp) * dp + (om_m * dm) * dm) * w06;  // ref: ...RadonIntermediate.cu:112,254
        acc[VALUE] += (double)(consistency * dkappa);                           // ref: ...RadonIntermediate.cu:269
        add(om_p, om_m);
    }
};

// The pair's two entries from the wave's sums (lane 0): c into column 0, u into column 1.
__device__ __forceinline__ void store_variance(const EccVarianceParams& g, long long local, const double (&acc)[VARIANCE_SUMS])
{
    g.values[local] = (float)acc[VALUE];  // pair_value<false>; no trip: 0
    g.values[g.col_stride + local] = acc[COUNT] > 0.0 ? (float)(acc[MASS] / acc[COUNT]) : 1.0f;
}

// Registers: pairs_weighted_kernel's live values plus the two divisions' temporaries; tests/test_variance_abi.py
// pins the plan and what was built.
template <bool DERIV>
__global__ __launch_bounds__(PK_MAIN_THREADS) void pairs_variance_kernel(EccPairParams p, EccVarianceParams g)
{
    double acc[VARIANCE_SUMS] = {0.0, 0.0, 0.0};
    VarianceForm form(g, acc);
    long long local;
    if (form_main_sums<DERIV>(p, form, acc, local)) store_variance(g, local, acc);
}

// ---- ECC_SAMPLING_REFERENCE -------------------------------------------------------------------------
template <int SPLIT>
__global__ __launch_bounds__(PK_THREADS) void pairs_variance_reference_kernel(EccPairParams p, EccVarianceParams g)
{
    double acc[VARIANCE_SUMS] = {0.0, 0.0, 0.0};
    VarianceForm form(g, acc);
    long long local;
    if (form_reference_sums<SPLIT>(p, form, acc, local)) store_variance(g, local, acc);
}

}  // namespace

// The two entries {c, u} of every pair of the launch p (records of ecc_launch_k01 for the same parameters, earlier on the same
// stream; first = 0, no slots) into g->values; the metric's dtrs are the data of the n_views views, then their variance fields.
// p->indices may be set (an index list, a pose batch's grid): the kernels do not read it, the record carries both Radon-intermediate
// indices, which must lie in [0, n_views) -- the variance of a sample comes from dtr n_views + that index.  g->floor: finite, > 0.
extern "C" hipError_t ecc_launch_pairs_variance(const EccPairParams* p, const EccVarianceParams* g, hipStream_t stream)
{
    if (p->count <= 0) return hipSuccess;
    if (p->use_corr || p->record_slots || p->skip_enabled || !g->values || g->col_stride < p->count || (g->col_stride & 3))
        return hipErrorInvalidValue;
    if (!(g->floor > 0.0f) || !(g->floor <= FLT_MAX)) return hipErrorInvalidValue;
    return launch_pair_form(*p, *g, stream, pairs_variance_reference_kernel<4>, pairs_variance_reference_kernel<1>,
                            pairs_variance_kernel<true>, pairs_variance_kernel<false>);
}
