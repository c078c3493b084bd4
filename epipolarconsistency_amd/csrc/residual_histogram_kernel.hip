// residual_histogram_kernel.hip -- the distribution of the per-sample residual, per view, from one pair launch (gfx950).
//
// The robust calls take a scale delta that a caller can only guess from per-pair figures; what the loss is applied to is the sample.
// These kernels run the pair evaluation of pairs_robust_kernel (one intermediate per view) or of pairs_variance_robust_kernel (the data
// and a variance field per view) in the metric's sampling mode -- the same positions, kappa range and gathers, in every loop class --
// and, instead of weighting and summing the residual d of a +-kappa sample, COUNT it: into bin
//   a   = fabsf(d)                                       raw form
//   a   = fabsf(d) / sqrtf(max(V_i + V_j, floor))        variance form: the studentised residual of variance_robust_kernel.hip
//   x   = a * inv_width
//   bin = x < (float)(n_bins - 1) ? (int)x : n_bins - 1  (the last bin is the overflow bin; NaN and +inf land there)
// of the rows of its pair's two views in a table of n_views x n_bins unsigned 64-bit counts (ecc_residual_histogram.h).  Counts are
// integers and integer addition commutes: the same inputs give the same bits in any launch order.
//
// The binning is the hot part.  A global atomic per sample into so small a table would serialise (the maps' eight per sample into
// whole planes already cost more than the gathers).  Each wave therefore owns n_bins 32-bit counters in LDS
// (WaveCounters): zeroed when its pair begins, one LDS integer atomic without return per sample, and flushed by the wave itself
// behind the pair's loops -- lane l adds the non-zero counts of bins l, l + 64, ... to the pair's two rows with plain global
// atomicAdd on unsigned long long, results unused.  EVERY wave flushes its own counters: under the four-waves-per-pair reference
// kernel the waves 1 .. 3 leave form_reference_sums with `false`, so the flush does not hang off the frames' "storing lane" return
// but off the form's own `live`, which the begin hook sets.  No workgroup barrier is used here, and the frames' only one
// (form_reference_sums<4>) lies in front of every non-uniform exit.  The order of the zeroing, the atomics and the flush's loads
// within the wave is wave_counters_order's.
// Both kernels run wholly on the frames of ecc_pair_forms.h; the forms below keep the gather-then-residual order of
// ecc_loss_forms.h's trips, so d is those kernels' d.  They are forms of their own and not a deposit policy of the loss forms: the
// Map hooks carry w and mu, not d.  The frames want a sum to reduce; these forms have none, the one sum stays 0.0.
// Plain vector loads, LDS and global integer atomics without return: no inline assembly, no float atomics.
// Not here (include/ecc_hip.h): pose-delta and transform batches; the form under line weights (counts would not be integers);
// range, group and RCCL forms; use_corr.
#include <hip/hip_runtime.h>
#include <float.h>

#include "ecc_layout.h"
#include "ecc_pair_forms.h"
#include "ecc_residual_histogram.h"

namespace {

// ---- the raw residual: RobustForm's 4 gathers ----------------------------------------------------------------------------------
struct ResidualHistogramForm : PairFormDefaults {
    const EccResidualHistogramParams& g;
    WaveCounters wave;
    GlobalFloats d0, d1;  // the reference loop's slabs

    __device__ __forceinline__ explicit ResidualHistogramForm(const EccResidualHistogramParams& g) : g(g) {}

    __device__ __forceinline__ void begin(const EccPairParams&, int iD0, int iD1) { wave.begin(g.counts, g.n_bins, g.inv_width, iD0, iD1); }

    __device__ __forceinline__ void poly_trip(const SlabView sv0, const SlabView sv1, const SampleTap t0p, const SampleTap t1p,
                                              const SampleTap t0m, const SampleTap t1m, float rel_sign, float)
    {
        const float v0p = sample_tap_value(sv0.origin, t0p), v1p = sample_tap_value(sv1.origin, t1p);
        const float v0m = sample_tap_value(sv0.origin, t0m), v1m = sample_tap_value(sv1.origin, t1m);
        const float dp = fmaf(v1p, rel_sign, v0p), dm = fmaf(v1m, rel_sign, v0m);
        wave.count(fabsf(dp));
        wave.count(fabsf(dm));
    }

    template <bool DERIV, int PITCH4>
    __device__ __forceinline__ void exact_trip(const SlabView, const SlabView, const LineTap t0p, const LineTap t1p, const LineTap t0m,
                                               const LineTap t1m, float, float)
    {
        const auto tap = [](const LineTap& t) { return line_tap_finish<DERIV>(line_footprint((GlobalBytes)t.ptr, 0u), t); };
        const float v0p = tap(t0p), v1p = tap(t1p), v0m = tap(t0m), v1m = tap(t1m);
        const float dp = v0p - v1p, dm = v0m - v1m;
        wave.count(fabsf(dp));
        wave.count(fabsf(dm));
    }

    __device__ __forceinline__ void reference_begin(const EccPairParams& p, int iD0, int iD1)
    {
        d0 = (GlobalFloats)p.slabs[iD0];
        d1 = (GlobalFloats)p.slabs[iD1];
        begin(p, iD0, iD1);
    }

    __device__ __forceinline__ void reference_trip(const EccPairParams& p, bool deriv, const PlainTap t0p, const PlainTap t1p,
                                                   const PlainTap t0m, const PlainTap t1m, float, float)
    {
        const float v0p = plain_tap_value(t0p, d0, p.pitch, p.n_alpha, p.n_t, deriv), v1p = plain_tap_value(t1p, d1, p.pitch, p.n_alpha, p.n_t, deriv);
        const float v0m = plain_tap_value(t0m, d0, p.pitch, p.n_alpha, p.n_t, deriv), v1m = plain_tap_value(t1m, d1, p.pitch, p.n_alpha, p.n_t, deriv);
        const float dp = v0p - v1p, dm = v0m - v1m;
        wave.count(fabsf(dp));
        wave.count(fabsf(dm));
    }
};

// ---- the studentised residual: FieldLossForm's 8 gathers -----------------------------------------------------------------------
struct VarianceResidualHistogramForm : PairFormDefaults {
    const EccVarianceResidualHistogramParams& g;
    WaveCounters wave;
    float floor;                    // launch-uniform, in a scalar register
    GlobalBytes w0, w1;             // the variance copies of the loop's two views (wave-uniform)
    GlobalFloats d0, d1, rw0, rw1;  // the reference loop's slabs: data and variance fields

    __device__ __forceinline__ explicit VarianceResidualHistogramForm(const EccVarianceResidualHistogramParams& g) : g(g) {}

    __device__ __forceinline__ void begin(const EccPairParams&, int iD0, int iD1)
    {
        floor = uniformf(g.floor);
        wave.begin(g.counts, g.n_bins, g.inv_width, iD0, iD1);
    }

    __device__ __forceinline__ void poly_begin(const SlabView sv0, const SlabView sv1, float, float)
    {
        w0 = sv0.origin + g.paired_channel_bytes, w1 = sv1.origin + g.paired_channel_bytes;
    }

    __device__ __forceinline__ void poly_trip(const SlabView sv0, const SlabView sv1, const SampleTap t0p, const SampleTap t1p,
                                              const SampleTap t0m, const SampleTap t1m, float rel_sign, float)
    {
        const float v0p = sample_tap_value(sv0.origin, t0p), v1p = sample_tap_value(sv1.origin, t1p);
        const float v0m = sample_tap_value(sv0.origin, t0m), v1m = sample_tap_value(sv1.origin, t1m);
        const float s0p = sample_tap_value(w0, t0p), s1p = sample_tap_value(w1, t1p);  // unsigned, whatever the folds
        const float s0m = sample_tap_value(w0, t0m), s1m = sample_tap_value(w1, t1m);
        const float dp = fmaf(v1p, rel_sign, v0p), dm = fmaf(v1m, rel_sign, v0m);
        wave.count(studentised_residual(floor, s0p, s1p, dp));
        wave.count(studentised_residual(floor, s0m, s1m, dm));
    }

    template <int PITCH4>
    __device__ __forceinline__ void exact_begin(const SlabView sv0, const SlabView sv1)
    {
        w0 = sv0.origin + channel_bytes<PITCH4>(g), w1 = sv1.origin + channel_bytes<PITCH4>(g);
    }

    template <bool DERIV, int PITCH4>
    __device__ __forceinline__ void exact_trip(const SlabView sv0, const SlabView sv1, const LineTap t0p, const LineTap t1p, const LineTap t0m,
                                               const LineTap t1m, float, float)
    {
        const unsigned o0p = line_tap_offset(t0p, sv0), o1p = line_tap_offset(t1p, sv1);
        const unsigned o0m = line_tap_offset(t0m, sv0), o1m = line_tap_offset(t1m, sv1);
        const float v0p = line_tap_finish<DERIV>(line_footprint(sv0.origin, o0p), t0p), v1p = line_tap_finish<DERIV>(line_footprint(sv1.origin, o1p), t1p);
        const float v0m = line_tap_finish<DERIV>(line_footprint(sv0.origin, o0m), t0m), v1m = line_tap_finish<DERIV>(line_footprint(sv1.origin, o1m), t1m);
        const float s0p = line_tap_finish<false>(line_footprint(w0, o0p), t0p), s1p = line_tap_finish<false>(line_footprint(w1, o1p), t1p);
        const float s0m = line_tap_finish<false>(line_footprint(w0, o0m), t0m), s1m = line_tap_finish<false>(line_footprint(w1, o1m), t1m);
        const float dp = v0p - v1p, dm = v0m - v1m;
        wave.count(studentised_residual(floor, s0p, s1p, dp));
        wave.count(studentised_residual(floor, s0m, s1m, dm));
    }

    __device__ __forceinline__ void reference_begin(const EccPairParams& p, int iD0, int iD1)
    {
        d0 = (GlobalFloats)p.slabs[iD0], d1 = (GlobalFloats)p.slabs[iD1];
        rw0 = (GlobalFloats)p.slabs[(long long)p.n_views + iD0], rw1 = (GlobalFloats)p.slabs[(long long)p.n_views + iD1];
        begin(p, iD0, iD1);
    }

    __device__ __forceinline__ void reference_trip(const EccPairParams& p, bool deriv, const PlainTap t0p, const PlainTap t1p,
                                                   const PlainTap t0m, const PlainTap t1m, float, float)
    {
        const float v0p = plain_tap_value(t0p, d0, p.pitch, p.n_alpha, p.n_t, deriv), v1p = plain_tap_value(t1p, d1, p.pitch, p.n_alpha, p.n_t, deriv);
        const float v0m = plain_tap_value(t0m, d0, p.pitch, p.n_alpha, p.n_t, deriv), v1m = plain_tap_value(t1m, d1, p.pitch, p.n_alpha, p.n_t, deriv);
        const float s0p = plain_tap_value(t0p, rw0, p.pitch, p.n_alpha, p.n_t, false), s1p = plain_tap_value(t1p, rw1, p.pitch, p.n_alpha, p.n_t, false);
        const float s0m = plain_tap_value(t0m, rw0, p.pitch, p.n_alpha, p.n_t, false), s1m = plain_tap_value(t1m, rw1, p.pitch, p.n_alpha, p.n_t, false);
        const float dp = v0p - v1p, dm = v0m - v1m;
        wave.count(studentised_residual(floor, s0p, s1p, dp));
        wave.count(studentised_residual(floor, s0m, s1m, dm));
    }
};

// ---- the kernels ---------------------------------------------------------------------------------------------------------------
// Registers: the gathers of pairs_robust_kernel / pairs_variance_robust_kernel, no float64 sums, one LDS address per
// sample; at most 96 vector registers, no scratch.  LDS: the launch's 4 x n_bins counters (dynamic; the reference kernel for four
// waves per pair adds the frame's 4 wave-sum slots).  tests/test_residual_histogram_abi.py pins the plan and what was built.
// `none`: the frames reduce T >= 1 per-lane sums (form_wave_sums, and under SPLIT = 4 the LDS slots part[T][4] behind a barrier).
// These forms add to none of them, so the one sum is the constant 0.0 and the compiler folds its wave tree and drops the slots: the
// kernels have no static LDS.  That rests on the optimiser; tests/test_residual_histogram_abi.py pins 0 bytes, and at worst the
// four-wave kernel would carry 32 bytes and one dead reduction per pair.
template <bool DERIV, class Form, class G>
__device__ __forceinline__ void histogram_main(const EccPairParams& p, const G& g)
{
    double none[1] = {0.0};
    Form form(g);
    long long local;
    (void)form_main_sums<DERIV>(p, form, none, local);
    form.wave.flush();
}

template <int SPLIT, class Form, class G>
__device__ __forceinline__ void histogram_reference(const EccPairParams& p, const G& g)
{
    double none[1] = {0.0};
    Form form(g);
    long long local;
    (void)form_reference_sums<SPLIT>(p, form, none, local);  // (false in the waves 1 .. 3 of a four-wave pair: they flush as wave 0 does)
    form.wave.flush();
}

template <bool DERIV>
__global__ __launch_bounds__(PK_MAIN_THREADS) void pairs_residual_histogram_kernel(EccPairParams p, EccResidualHistogramParams g)
{
    histogram_main<DERIV, ResidualHistogramForm>(p, g);
}

template <int SPLIT>
__global__ __launch_bounds__(PK_THREADS) void pairs_residual_histogram_reference_kernel(EccPairParams p, EccResidualHistogramParams g)
{
    histogram_reference<SPLIT, ResidualHistogramForm>(p, g);
}

template <bool DERIV>
__global__ __launch_bounds__(PK_MAIN_THREADS) void pairs_variance_residual_histogram_kernel(EccPairParams p, EccVarianceResidualHistogramParams g)
{
    histogram_main<DERIV, VarianceResidualHistogramForm>(p, g);
}

template <int SPLIT>
__global__ __launch_bounds__(PK_THREADS) void pairs_variance_residual_histogram_reference_kernel(EccPairParams p, EccVarianceResidualHistogramParams g)
{
    histogram_reference<SPLIT, VarianceResidualHistogramForm>(p, g);
}

}  // namespace

// Every sample of every pair of the launch p (records of ecc_launch_k01 for the same parameters, earlier on the same stream;
// first = 0, no slots) into the two rows of its pair in g->counts (zeroed earlier on the same stream).  The record carries both
// Radon-intermediate indices, which must lie in [0, n_views): they address the rows (the host calls check them).
extern "C" hipError_t ecc_launch_pairs_residual_histogram(const EccPairParams* p, const EccResidualHistogramParams* g, hipStream_t stream)
{
    if (p->count <= 0) return hipSuccess;
    if (!histogram_launch_ok(*p, *g)) return hipErrorInvalidValue;
    return launch_pair_form(*p, *g, stream, pairs_residual_histogram_reference_kernel<4>, pairs_residual_histogram_reference_kernel<1>,
                            pairs_residual_histogram_kernel<true>, pairs_residual_histogram_kernel<false>,
                            ecc_residual_histogram_lds_bytes(g->n_bins));
}

// The same in sigma units; the metric's dtrs are the data of the n_views views, then their variance fields.  g->floor: finite, > 0.
extern "C" hipError_t ecc_launch_pairs_variance_residual_histogram(const EccPairParams* p, const EccVarianceResidualHistogramParams* g,
                                                                   hipStream_t stream)
{
    if (p->count <= 0) return hipSuccess;
    if (!histogram_launch_ok(*p, *g)) return hipErrorInvalidValue;
    if (!(g->floor > 0.0f) || !(g->floor <= FLT_MAX)) return hipErrorInvalidValue;
    return launch_pair_form(*p, *g, stream, pairs_variance_residual_histogram_reference_kernel<4>,
                            pairs_variance_residual_histogram_reference_kernel<1>, pairs_variance_residual_histogram_kernel<true>,
                            pairs_variance_residual_histogram_kernel<false>, ecc_residual_histogram_lds_bytes(g->n_bins));
}
