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
// below them.  The trips are FieldLossForm<EccVarianceRobustParams, StudentisedRule, NoMap>'s (ecc_loss_forms.h, shared with
// variance_robust_map_kernel.hip and, under another rule, the weighted-robust files): the 8 gathers of VarianceForm followed by the
// studentised weights; five per-lane float64 sums in trip order; store_field_loss there makes the columns.  loss, delta and floor are
// launch-uniform kernel arguments and the loss a uniform select, not a template parameter; the weight itself is
// ecc_studentised_weight.h's.  Plain vector loads and stores only: no atomics, no inline assembly, no LDS in the main kernels.
// Not here (include/ecc_hip.h): base columns kept between calls; range, group and RCCL forms; the correlation cost; a
// covariance-aware model for derivative data.
#include <hip/hip_runtime.h>
#include <float.h>

#include "ecc_layout.h"
#include "ecc_loss_forms.h"

namespace {

// Registers: pairs_weighted_robust_kernel's live values plus the temporaries of two square roots and two more
// divisions, the loss and the floor in four scalar registers; tests/test_variance_robust_abi.py pins the plan and what was built.
template <bool DERIV>
__global__ __launch_bounds__(PK_MAIN_THREADS) void pairs_variance_robust_kernel(EccPairParams p, EccVarianceRobustParams g)
{
    double acc[FIELD_LOSS_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    FieldLossForm<EccVarianceRobustParams, StudentisedRule, NoMap> form(g, acc);
    long long local;
    if (form_main_sums<DERIV>(p, form, acc, local)) store_field_loss(g, local, acc);
}

// ---- ECC_SAMPLING_REFERENCE -------------------------------------------------------------------------
template <int SPLIT>
__global__ __launch_bounds__(PK_THREADS) void pairs_variance_robust_reference_kernel(EccPairParams p, EccVarianceRobustParams g)
{
    double acc[FIELD_LOSS_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    FieldLossForm<EccVarianceRobustParams, StudentisedRule, NoMap> form(g, acc);
    long long local;
    if (form_reference_sums<SPLIT>(p, form, acc, local)) store_field_loss(g, local, acc);
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
    if (!loss_launch_ok(*p, *g)) return hipErrorInvalidValue;
    if (!(g->floor > 0.0f) || !(g->floor <= FLT_MAX)) return hipErrorInvalidValue;
    return launch_pair_form(*p, *g, stream, pairs_variance_robust_reference_kernel<4>, pairs_variance_robust_reference_kernel<1>,
                            pairs_variance_robust_kernel<true>, pairs_variance_robust_kernel<false>);
}
