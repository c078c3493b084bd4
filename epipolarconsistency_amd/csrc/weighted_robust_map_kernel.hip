// weighted_robust_map_kernel.hip -- where the robust loss rejects on a metric that already carries line weights: the metric with
// per-line weights AND a per-sample robust loss as weighted_robust_kernel.hip evaluates it, with every sample's bilinear footprint
// deposited into its view's own Radon space under the sample's weight product (gfx950).
//
// A metric over 2 n Radon intermediates: dtr i the data of view i, dtr n + i its line weights W_i.  Per pair and +-kappa sample the
// positions, the kappa range, the residual d, mu = W_i(sample) * W_j(sample), the IRLS weight w = robust_weight(L, d) of the RAW
// residual and f = mu * w are pairs_weighted_robust_kernel's in the metric's sampling mode, and so are the five per-lane float64 sums
// and the four columns {c, u, k, r}: both files run the trips of FieldLossForm under LineWeightRule (ecc_loss_forms.h), here with
// MapDeposits (ecc_robust_map.h) as its deposit policy, the deposits behind the sums.  A sample of view v with the float32 footprint
// products b of robust_map_kernel.hip adds, per cell,
//     x = b * mu               HITS_v[cell] += x               REJ_v[cell] += x * (1 - w)          (all float32)
// at exactly the cells its gather reads, for v = i with view i's footprint and v = j with view j's; mu is the product of BOTH views'
// weights in either case: a sample counts in a view's map as far as the metric counted it.  HITS is then the weight mass that
// reached a bin, REJ the part of it the loss refused, and REJ / HITS the rejected share among the trusted lines -- what
// weighted_robust_map_weights_kernel below turns into the next pass's weights, W_v * factor.
// The planes, their fixed point (quantum 2^-32, plain atomicAdd on unsigned long long, results unused), their padded geometry, the
// cell addressing of the three loop kinds and the last-cell guard are ecc_robust_map.h's, shared with robust_map_kernel.hip;
// robust_map_finish_kernel (there) folds the borders and makes the float planes.  Whether a view is mapped is wave-uniform: a side
// that is not mapped is skipped by a scalar branch.  Deposits of zero are skipped (mu == 0.0f: the footprint, w == 1.0f: its REJ
// half).  No address depends on mu or w.  Weights are expected in [0, 1]; outside that range the columns are still
// pairs_weighted_robust_kernel's and every deposit still goes to the same cells, but what it adds is unspecified.
// No inline assembly, no float atomics.
// Not here (include/ecc_hip.h): pose-delta, transform, range, group and RCCL forms; use_corr; a wave-level pre-sum of the deposits.
#include <hip/hip_runtime.h>
#include <float.h>

#include "ecc_layout.h"
#include "ecc_loss_forms.h"
#include "ecc_robust_map.h"

namespace {

// Registers: pairs_weighted_robust_kernel's plus what the deposits cost pairs_robust_map_kernel over
// pairs_robust_kernel; tests/test_weighted_robust_map_abi.py pins the plan and what was built.
template <bool DERIV>
__global__ __launch_bounds__(PK_MAIN_THREADS) void pairs_weighted_robust_map_kernel(EccPairParams p, EccWeightedRobustMapParams g)
{
    double acc[FIELD_LOSS_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    FieldLossForm<EccWeightedRobustMapParams, LineWeightRule, MapDeposits> form(g, acc);
    long long local;
    if (form_main_sums<DERIV>(p, form, acc, local)) store_field_loss(g, local, acc);
}

// ---- ECC_SAMPLING_REFERENCE -------------------------------------------------------------------------
template <int SPLIT>
__global__ __launch_bounds__(PK_THREADS) void pairs_weighted_robust_map_reference_kernel(EccPairParams p, EccWeightedRobustMapParams g)
{
    double acc[FIELD_LOSS_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    FieldLossForm<EccWeightedRobustMapParams, LineWeightRule, MapDeposits> form(g, acc);
    long long local;
    if (form_reference_sums<SPLIT>(p, form, acc, local)) store_field_loss(g, local, acc);
}

// ---- the map as the next pass's line weights ---------------------------------------------------------
// One thread per padded element of a weight slab (rows -1 .. n_alpha, all `pitch` columns: written completely): the old weight at
// that element times the factor of the bin it replicates, one float32 multiply.  The factor is map_mean_weight
// (ecc_robust_map.h) of the held float planes, the rule of all three feedback kernels.
__global__ __launch_bounds__(256) void weighted_robust_map_weights_kernel(const float* __restrict__ hits, const float* __restrict__ rejected,
                                                                          const float* const* __restrict__ weights,
                                                                          const int32_t* __restrict__ views, float* __restrict__ slabs,
                                                                          int n_alpha, int n_t, int pitch, float min_hits, float gain)
{
    const long long slab = (long long)(n_alpha + 2) * pitch;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= slab) return;
    const float factor = map_mean_weight(hits, rejected, e, blockIdx.y, n_alpha, n_t, pitch, min_hits, gain);
    slabs[(long long)blockIdx.y * slab + e] = weights[views[blockIdx.y]][e] * factor;
}

}  // namespace

// The four entries {c, u, k, r} of every pair of the launch p into g->values, as ecc_launch_pairs_weighted_robust (the same
// conditions on p and on the metric's intermediates), and the deposits of every sample of a mapped view into g->planes (zeroed
// earlier on the same stream).  g->slot_of has one entry per DATA intermediate, p->n_views of them.
extern "C" hipError_t ecc_launch_pairs_weighted_robust_map(const EccPairParams* p, const EccWeightedRobustMapParams* g, hipStream_t stream)
{
    if (p->count <= 0) return hipSuccess;
    if (!loss_launch_ok(*p, *g) || !map_launch_ok(*p, *g)) return hipErrorInvalidValue;
    return launch_pair_form(*p, *g, stream, pairs_weighted_robust_map_reference_kernel<4>, pairs_weighted_robust_map_reference_kernel<1>,
                            pairs_weighted_robust_map_kernel<true>, pairs_weighted_robust_map_kernel<false>);
}

extern "C" hipError_t ecc_launch_weighted_robust_map_weights(const float* hits, const float* rejected, const float* const* weights,
                                                             const int32_t* views, float* slabs, int n_mapped, int n_alpha, int n_t, int pitch,
                                                             float min_hits, float gain, hipStream_t stream)
{
    if (n_mapped <= 0) return hipSuccess;
    if (n_mapped > 65535) return hipErrorInvalidValue;
    const long long slab = (long long)(n_alpha + 2) * pitch;
    hipLaunchKernelGGL(weighted_robust_map_weights_kernel, dim3((unsigned)((slab + 255) / 256), (unsigned)n_mapped), dim3(256), 0, stream, hits,
                       rejected, weights, views, slabs, n_alpha, n_t, pitch, min_hits, gain);
    return hipGetLastError();
}
