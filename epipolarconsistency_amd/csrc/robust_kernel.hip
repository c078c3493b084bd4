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
// Per kappa step the value term is pairs_kernel's expression with w multiplied into the first factor only (as weighted_kernel.hip
// does with its mu):
//   polynomial loops             fmaf(w_p * dp, dp, (w_m * dm) * dm) * w06_dkappa
//   exact and reference loops    (((w_p * dp) * dp + (w_m * dm) * dm) * K0[6]) * dkappa
// so with w == 1.0f (delta = +inf, or any delta no |d| exceeds) these are pairs_kernel's bits.  Beside the value each lane adds
// (double)(w_p + w_m), the weight mass, (double)(dp * dp) + (double)(dm * dm), the raw squares (products in float32), and 2.0, the
// sample count.  Per pair
//   c = the float32 value, as pairs_kernel stores it,
//   u = (float)(mass / count), the INLIER MASS in (0, 1],
//   r = (float)(raw / count), the mean squared raw residual: no loss and no delta in it (ecc_host_robust_scale takes delta from it),
// a pair whose loops ran no trip (count == 0) has {0, 1, 0}; three columns, c and u summed by sum_gram_kernel (ecc_robust.hip).
// Both kernels run wholly on the frames of ecc_pair_forms.h: form_main_sums and form_reference_sums with every piece
// below them.  RobustForm's trip gathers the 4 data footprints of a kappa step, forms the two residuals and their weights, and adds the
// value term, the weight mass, the raw squares and 2.0 to four per-lane float64 sums in trip order.  loss and delta are launch-uniform
// kernel arguments and the loss a uniform select (a scalar branch around one division), not a template parameter: three times the
// instantiations of every loop for the same registers.  Plain vector loads and stores only: no atomics, no inline
// assembly.
// The pose-delta and transform forms (ecc_robust_batches.hip) launch these kernels over their grids as they stand.
// The loss combined with line weights on a 2 n metric is weighted_robust_kernel.hip.
// Not here (include/ecc_hip.h): range, group and RCCL forms; the loss under the correlation cost; Tukey's biweight.
#include <hip/hip_runtime.h>
#include <float.h>

#include "ecc_layout.h"
#include "ecc_pair_forms.h"
#include "ecc_robust_weight.h"

namespace {

// the four per-lane sums: the value, the weight mass, the raw squares, the sample count
enum { VALUE, MASS, RAW, COUNT, ROBUST_SUMS };

// (RobustLoss, the launch-uniform part of the loss, and robust_weight, w(d), are in ecc_robust_weight.h: weighted_robust_kernel.hip
// takes the same ones)

// the trips of the three loop kinds (ecc_pair_forms.h): 4 gathers, the residuals of the + and the - sample, their weights, the sums
struct RobustForm : PairFormDefaults {
    const EccRobustParams& g;
    double (&acc)[ROBUST_SUMS];
    RobustLoss L;         // the launch-uniform loss, in scalar registers
    GlobalFloats d0, d1;  // the reference loop's slabs

    __device__ __forceinline__ RobustForm(const EccRobustParams& g, double (&acc)[ROBUST_SUMS]) : g(g), acc(acc) {}

    __device__ __forceinline__ void begin(const EccPairParams&, int, int)
    {
        L = {__builtin_amdgcn_readfirstlane(g.loss), uniformf(g.delta), uniformf(g.inv_delta)};
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
    }

    template <bool DERIV, int PITCH4>
    __device__ __forceinline__ void exact_trip(const SlabView, const SlabView, const LineTap t0p, const LineTap t1p, const LineTap t0m,
                                               const LineTap t1m, float w06, float dkappa)
    {
        const auto tap = [](const LineTap& t) { return line_tap_finish<DERIV>(line_footprint((GlobalBytes)t.ptr, 0u), t); };
        const float v0p = tap(t0p), v1p = tap(t1p), v0m = tap(t0m), v1m = tap(t1m);
        const float dp = v0p - v1p, dm = v0m - v1m;
        const float w_p = robust_weight(L, dp), w_m = robust_weight(L, dm);
        add((((w_p * dp) * dp + (w_m * dm) * dm) * w06) * dkappa, w_p, w_m, dp, dm);  // ref: ...RadonIntermediate.cu:112,269,254
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
    }
};

// The pair's three entries from the wave's sums (lane 0): c into column 0, u into column 1, r into column 2.
__device__ __forceinline__ void store_robust(const EccRobustParams& g, long long local, const double (&acc)[ROBUST_SUMS])
{
    const bool any = acc[COUNT] > 0.0;
    g.values[local] = (float)acc[VALUE];  // pair_value<false>; no trip: 0
    g.values[g.col_stride + local] = any ? (float)(acc[MASS] / acc[COUNT]) : 1.0f;
    g.values[2 * g.col_stride + local] = any ? (float)(acc[RAW] / acc[COUNT]) : 0.0f;
}

// Registers: the 4 gathers of a kappa step as in pairs_kernel, 8 accumulator registers; tests/test_robust_abi.py pins
// the plan and what was built.
template <bool DERIV>
__global__ __launch_bounds__(PK_MAIN_THREADS) void pairs_robust_kernel(EccPairParams p, EccRobustParams g)
{
    double acc[ROBUST_SUMS] = {0.0, 0.0, 0.0, 0.0};
    RobustForm form(g, acc);
    long long local;
    if (form_main_sums<DERIV>(p, form, acc, local)) store_robust(g, local, acc);
}

// ---- ECC_SAMPLING_REFERENCE -------------------------------------------------------------------------
template <int SPLIT>
__global__ __launch_bounds__(PK_THREADS) void pairs_robust_reference_kernel(EccPairParams p, EccRobustParams g)
{
    double acc[ROBUST_SUMS] = {0.0, 0.0, 0.0, 0.0};
    RobustForm form(g, acc);
    long long local;
    if (form_reference_sums<SPLIT>(p, form, acc, local)) store_robust(g, local, acc);
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
    return launch_pair_form(*p, *g, stream, pairs_robust_reference_kernel<4>, pairs_robust_reference_kernel<1>, pairs_robust_kernel<true>,
                            pairs_robust_kernel<false>);
}
