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
// below them.  The trips are FieldLossForm<EccWeightedRobustParams, LineWeightRule, NoMap>'s (ecc_loss_forms.h, shared with
// weighted_robust_map_kernel.hip and, under another rule, the variance-robust files): WeightedForm's 8 gathers followed by
// RobustForm's weights; five per-lane float64 sums in trip order; store_field_loss there makes the columns.  loss and delta are
// launch-uniform kernel arguments and the loss a uniform select, not a template parameter.  Plain
// vector loads and stores only: no atomics, no inline assembly.
// Not here (include/ecc_hip.h): the pose-delta and transform batches of this form (they need no kernel beyond this one); range, group
// and RCCL forms; the correlation cost; Tukey's biweight; a variance form.
#include <hip/hip_runtime.h>
#include <float.h>

#include "ecc_layout.h"
#include "ecc_loss_forms.h"

namespace {

// Registers: the 8 gathers of a kappa step as in pairs_weighted_kernel, 10 accumulator registers against its 6, the
// loss in three scalar registers; tests/test_weighted_robust_abi.py pins the plan and what was built.
template <bool DERIV>
__global__ __launch_bounds__(PK_MAIN_THREADS) void pairs_weighted_robust_kernel(EccPairParams p, EccWeightedRobustParams g)
{
    double acc[FIELD_LOSS_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    FieldLossForm<EccWeightedRobustParams, LineWeightRule, NoMap> form(g, acc);
    long long local;
    if (form_main_sums<DERIV>(p, form, acc, local)) store_field_loss(g, local, acc);
}

// ---- ECC_SAMPLING_REFERENCE -------------------------------------------------------------------------
template <int SPLIT>
__global__ __launch_bounds__(PK_THREADS) void pairs_weighted_robust_reference_kernel(EccPairParams p, EccWeightedRobustParams g)
{
    double acc[FIELD_LOSS_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    FieldLossForm<EccWeightedRobustParams, LineWeightRule, NoMap> form(g, acc);
    long long local;
    if (form_reference_sums<SPLIT>(p, form, acc, local)) store_field_loss(g, local, acc);
}

}  // namespace

// The four entries {c, u, k, r} of every pair of the launch p (records of ecc_launch_k01 for the same parameters, earlier on the same
// stream; first = 0, no slots) into g->values; the metric's dtrs are the data of the n_views views, then their line weights.
// p->indices may be set (an index list): the kernels do not read it, the record carries both Radon-intermediate indices, which must
// lie in [0, n_views) -- the weights of a sample come from dtr n_views + that index (the host calls check both, ecc_weighted_robust.hip).
extern "C" hipError_t ecc_launch_pairs_weighted_robust(const EccPairParams* p, const EccWeightedRobustParams* g, hipStream_t stream)
{
    if (p->count <= 0) return hipSuccess;
    if (!loss_launch_ok(*p, *g)) return hipErrorInvalidValue;
    return launch_pair_form(*p, *g, stream, pairs_weighted_robust_reference_kernel<4>, pairs_weighted_robust_reference_kernel<1>,
                            pairs_weighted_robust_kernel<true>, pairs_weighted_robust_kernel<false>);
}
