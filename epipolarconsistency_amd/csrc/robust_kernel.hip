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
// below them.  The trips are RobustForm<EccRobustParams, NoMap>'s (ecc_loss_forms.h, shared with robust_map_kernel.hip): a trip gathers
// the 4 data footprints of a kappa step, forms the two residuals and their weights, and adds the value term, the weight mass, the raw
// squares and 2.0 to four per-lane float64 sums in trip order; store_robust there makes the columns.  loss and delta are launch-uniform
// kernel arguments and the loss a uniform select (a scalar branch around one division), not a template parameter: three times the
// instantiations of every loop for the same registers.  Plain vector loads and stores only: no atomics, no inline
// assembly.
// The pose-delta and transform forms (ecc_robust_batches.hip) launch these kernels over their grids as they stand.
// The loss combined with line weights on a 2 n metric is weighted_robust_kernel.hip.
// Not here (include/ecc_hip.h): range, group and RCCL forms; the loss under the correlation cost; Tukey's biweight.
#include <hip/hip_runtime.h>
#include <float.h>

#include "ecc_layout.h"
#include "ecc_loss_forms.h"

namespace {

// Registers: the 4 gathers of a kappa step as in pairs_kernel, 8 accumulator registers; tests/test_robust_abi.py pins
// the plan and what was built.
template <bool DERIV>
__global__ __launch_bounds__(PK_MAIN_THREADS) void pairs_robust_kernel(EccPairParams p, EccRobustParams g)
{
    double acc[ROBUST_SUMS] = {0.0, 0.0, 0.0, 0.0};
    RobustForm<EccRobustParams, NoMap> form(g, acc);
    long long local;
    if (form_main_sums<DERIV>(p, form, acc, local)) store_robust(g, local, acc);
}

// ---- ECC_SAMPLING_REFERENCE -------------------------------------------------------------------------
template <int SPLIT>
__global__ __launch_bounds__(PK_THREADS) void pairs_robust_reference_kernel(EccPairParams p, EccRobustParams g)
{
    double acc[ROBUST_SUMS] = {0.0, 0.0, 0.0, 0.0};
    RobustForm<EccRobustParams, NoMap> form(g, acc);
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
    if (!loss_launch_ok(*p, *g)) return hipErrorInvalidValue;
    return launch_pair_form(*p, *g, stream, pairs_robust_reference_kernel<4>, pairs_robust_reference_kernel<1>, pairs_robust_kernel<true>,
                            pairs_robust_kernel<false>);
}
