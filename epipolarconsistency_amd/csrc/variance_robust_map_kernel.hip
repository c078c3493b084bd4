// variance_robust_map_kernel.hip -- where the robust loss rejects IN SIGMA UNITS: the metric with inverse-variance sample weights and
// a per-sample robust loss of the studentised residual as variance_robust_kernel.hip evaluates it, with every sample's bilinear
// footprint deposited into its view's own Radon space (gfx950).
//
// A metric over 2 n Radon intermediates: dtr i the data of view i, dtr n + i its variance field V_i.  Per pair and +-kappa sample the
// positions, the kappa range, the residual d, s = V_i(sample) + V_j(sample), sc, om = 1 / sc, the loss weight w of z = d / sqrt(sc)
// and f = om * w are pairs_variance_robust_kernel's in the metric's sampling mode (the weight is ecc_studentised_weight.h's), and so
// are the five per-lane float64 sums and the four columns {c, u, k, r}: both files run the trips of FieldLossForm under
// StudentisedRule (ecc_loss_forms.h), here with MapDeposits (ecc_robust_map.h) as its deposit policy, the deposits behind the sums.
// A sample of view v with the float32 footprint products b of robust_map_kernel.hip adds, per cell,
//     HITS_v[cell] += b                REJ_v[cell] += b * (1 - w)          (all float32)
// at exactly the cells its gather reads, for v = i with view i's footprint and v = j with view j's.  The deposits are in COUNT units:
// w is the loss weight alone, not f, and b is not multiplied by om -- om carries the data's units and reaches 1 / floor, so b * om
// can leave the fixed point's [0, 2^32); in count units REJ / HITS is the share of a bin's samples with |z| > delta, which has a
// known expectation under a correct noise model, and with V == 0.5f (sc == 1.0f) every deposit has robust_map_kernel.hip's bits.
// deposit_footprint's mu is the literal 1.0f: the compiler drops the multiply and the test.
// The planes, their fixed point (quantum 2^-32, plain atomicAdd on unsigned long long, results unused), their padded geometry, the
// cell addressing of the three loop kinds and the last-cell guard are ecc_robust_map.h's, shared with the two other map kernels;
// robust_map_finish_kernel (robust_map_kernel.hip) folds the borders and makes the float planes.  Whether a view is mapped is
// wave-uniform: a side that is not mapped is skipped by a scalar branch.  REJ deposits of zero are skipped (w == 1.0f).  No address
// depends on w.  variance_robust_map_variances_kernel below turns the held planes into the next pass's variance fields.
// No inline assembly, no float atomics.
// Not here (include/ecc_hip.h): pose-delta, transform, range, group and RCCL forms; use_corr; a third plane of squared residuals.
#include <hip/hip_runtime.h>
#include <float.h>

#include "ecc_layout.h"
#include "ecc_loss_forms.h"
#include "ecc_robust_map.h"

namespace {

// Registers: pairs_variance_robust_kernel's plus what the deposits cost pairs_robust_map_kernel over
// pairs_robust_kernel; tests/test_variance_robust_map_abi.py pins the plan and what was built.
template <bool DERIV>
__global__ __launch_bounds__(PK_MAIN_THREADS) void pairs_variance_robust_map_kernel(EccPairParams p, EccVarianceRobustMapParams g)
{
    double acc[FIELD_LOSS_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    FieldLossForm<EccVarianceRobustMapParams, StudentisedRule, MapDeposits> form(g, acc);
    long long local;
    if (form_main_sums<DERIV>(p, form, acc, local)) store_field_loss(g, local, acc);
}

// ---- ECC_SAMPLING_REFERENCE -------------------------------------------------------------------------
template <int SPLIT>
__global__ __launch_bounds__(PK_THREADS) void pairs_variance_robust_map_reference_kernel(EccPairParams p, EccVarianceRobustMapParams g)
{
    double acc[FIELD_LOSS_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    FieldLossForm<EccVarianceRobustMapParams, StudentisedRule, MapDeposits> form(g, acc);
    long long local;
    if (form_reference_sums<SPLIT>(p, form, acc, local)) store_field_loss(g, local, acc);
}

// ---- the map as the next pass's variance fields ------------------------------------------------------
// One thread per padded element of a variance slab (rows -1 .. n_alpha, all `pitch` columns: written completely).  mu is
// map_mean_weight (ecc_robust_map.h) of the held float planes at the bin the element replicates, the rule of all three feedback
// kernels; the variance of a bin whose samples reached it with mean loss weight mu is V / mu, the IRLS reading (a sample's effective
// variance is sigma^2 / w), capped at max_factor; before the multiply the old variance is raised to half the floor, so that two
// raised samples sum to the floor exactly and a field of zeros can be raised at all.  factor == 1: the old bits.
__global__ __launch_bounds__(256) void variance_robust_map_variances_kernel(const float* __restrict__ hits, const float* __restrict__ rejected,
                                                                            const float* const* __restrict__ variances,
                                                                            const int32_t* __restrict__ views, float* __restrict__ slabs,
                                                                            int n_alpha, int n_t, int pitch, float half, float min_hits,
                                                                            float gain, float max_factor)
{
    const long long slab = (long long)(n_alpha + 2) * pitch;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= slab) return;
    const float mu = map_mean_weight(hits, rejected, e, blockIdx.y, n_alpha, n_t, pitch, min_hits, gain);
    const float factor = (mu * max_factor <= 1.0f) ? max_factor : 1.0f / mu;
    const float old = variances[views[blockIdx.y]][e];
    slabs[(long long)blockIdx.y * slab + e] = factor == 1.0f ? old : (old < half ? half : old) * factor;
}

}  // namespace

// The four entries {c, u, k, r} of every pair of the launch p into g->values, as ecc_launch_pairs_variance_robust (the same
// conditions on p, on the floor and on the metric's intermediates), and the deposits of every sample of a mapped view into
// g->planes (zeroed earlier on the same stream).  g->slot_of has one entry per DATA intermediate, p->n_views of them.
extern "C" hipError_t ecc_launch_pairs_variance_robust_map(const EccPairParams* p, const EccVarianceRobustMapParams* g, hipStream_t stream)
{
    if (p->count <= 0) return hipSuccess;
    if (!loss_launch_ok(*p, *g) || !map_launch_ok(*p, *g)) return hipErrorInvalidValue;
    if (!(g->floor > 0.0f) || !(g->floor <= FLT_MAX)) return hipErrorInvalidValue;
    return launch_pair_form(*p, *g, stream, pairs_variance_robust_map_reference_kernel<4>, pairs_variance_robust_map_reference_kernel<1>,
                            pairs_variance_robust_map_kernel<true>, pairs_variance_robust_map_kernel<false>);
}

extern "C" hipError_t ecc_launch_variance_robust_map_variances(const float* hits, const float* rejected, const float* const* variances,
                                                               const int32_t* views, float* slabs, int n_mapped, int n_alpha, int n_t, int pitch,
                                                               float floor, float min_hits, float gain, float max_factor, hipStream_t stream)
{
    if (n_mapped <= 0) return hipSuccess;
    if (n_mapped > 65535) return hipErrorInvalidValue;
    const long long slab = (long long)(n_alpha + 2) * pitch;
    hipLaunchKernelGGL(variance_robust_map_variances_kernel, dim3((unsigned)((slab + 255) / 256), (unsigned)n_mapped), dim3(256), 0, stream, hits,
                       rejected, variances, views, slabs, n_alpha, n_t, pitch, 0.5f * floor, min_hits, gain, max_factor);
    return hipGetLastError();
}
