// weighted_robust_map_kernel.hip -- where the robust loss rejects on a metric that already carries line weights: the metric with
// per-line weights AND a per-sample robust loss as weighted_robust_kernel.hip evaluates it, with every sample's bilinear footprint
// deposited into its view's own Radon space under the sample's weight product (gfx950).
//
// A metric over 2 n Radon intermediates: dtr i the data of view i, dtr n + i its line weights W_i.  Per pair and +-kappa sample the
// positions, the kappa range, the residual d, mu = W_i(sample) * W_j(sample), the IRLS weight w = robust_weight(L, d) of the RAW
// residual and f = mu * w are pairs_weighted_robust_kernel's in the metric's sampling mode, and so are the five per-lane float64 sums
// and the four columns {c, u, k, r}: the trips below are WeightedRobustForm's, statement for statement, with the deposits behind the
// sums.  A sample of view v with the float32 footprint products b of robust_map_kernel.hip adds, per cell,
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
#include "ecc_pair_forms.h"
#include "ecc_robust_weight.h"
#include "ecc_robust_map.h"

namespace {

// the five per-lane sums, as in weighted_robust_kernel.hip: the value, the weight mass, the mass the loss keeps, the weighted raw
// squares, the sample count
enum { VALUE, MASS, KEPT, RAW, COUNT, WEIGHTED_ROBUST_SUMS };

struct WeightedRobustMapForm : PairFormDefaults, MapPlanes {
    const EccWeightedRobustMapParams& g;
    double (&acc)[WEIGHTED_ROBUST_SUMS];
    RobustLoss L;                       // the launch-uniform loss, in scalar registers
    GlobalBytes w0, w1;                 // the weight copies of the loop's two views (wave-uniform)
    GlobalFloats d0, d1, rw0, rw1;      // the reference loop's slabs: data and weights
    unsigned long long *hits0, *hits1;  // the HITS plane of the pair's two views, null: not mapped (wave-uniform)

    __device__ __forceinline__ WeightedRobustMapForm(const EccWeightedRobustMapParams& g, double (&acc)[WEIGHTED_ROBUST_SUMS]) : g(g), acc(acc) {}

    __device__ __forceinline__ unsigned long long* plane_of(int iD) const
    {
        const int slot = __builtin_amdgcn_readfirstlane(g.slot_of[iD]);
        return slot < 0 ? nullptr : g.planes + (long long)slot * g.plane_cells;
    }

    __device__ __forceinline__ void begin(const EccPairParams& p, int iD0, int iD1)
    {
        L = {__builtin_amdgcn_readfirstlane(g.loss), uniformf(g.delta), uniformf(g.inv_delta)};
        hits0 = plane_of(iD0);
        hits1 = plane_of(iD1);
        rej_cells = g.rej_cells;
        pitch = (unsigned)p.pitch;
        last_cell = (unsigned)(g.plane_cells - 1);
    }

    // the sums of a trip beside its value
    __device__ __forceinline__ void add(float value, float mu_p, float mu_m, float f_p, float f_m, float dp, float dm)
    {
        acc[VALUE] += (double)value;
        acc[MASS] += (double)(mu_p + mu_m);
        acc[KEPT] += (double)(f_p + f_m);
        acc[RAW] += (double)(mu_p * (dp * dp)) + (double)(mu_m * (dm * dm));
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
        const float mu_p = sample_tap_value(w0, t0p) * sample_tap_value(w1, t1p);  // unsigned, whatever the folds
        const float mu_m = sample_tap_value(w0, t0m) * sample_tap_value(w1, t1m);
        const float dp = fmaf(v1p, rel_sign, v0p), dm = fmaf(v1m, rel_sign, v0m);
        const float w_p = robust_weight(L, dp), w_m = robust_weight(L, dm);
        const float f_p = mu_p * w_p, f_m = mu_m * w_m;
        add(fmaf(f_p * dp, dp, (f_m * dm) * dm) * w06_dkappa, mu_p, mu_m, f_p, f_m, dp, dm);
        if (hits0) {
            deposit_at(hits0, t0p.off >> 3, t0p.fx, t0p.fy, w_p, mu_p);
            deposit_at(hits0, t0m.off >> 3, t0m.fx, t0m.fy, w_m, mu_m);
        }
        if (hits1) {
            deposit_at(hits1, t1p.off >> 3, t1p.fx, t1p.fy, w_p, mu_p);
            deposit_at(hits1, t1m.off >> 3, t1m.fx, t1m.fy, w_m, mu_m);
        }
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
        const float mu_p = line_tap_finish<false>(line_footprint(w0, o0p), t0p) * line_tap_finish<false>(line_footprint(w1, o1p), t1p);
        const float mu_m = line_tap_finish<false>(line_footprint(w0, o0m), t0m) * line_tap_finish<false>(line_footprint(w1, o1m), t1m);
        const float dp = v0p - v1p, dm = v0m - v1m;
        const float w_p = robust_weight(L, dp), w_m = robust_weight(L, dm);
        const float f_p = mu_p * w_p, f_m = mu_m * w_m;
        add((((f_p * dp) * dp + (f_m * dm) * dm) * w06) * dkappa, mu_p, mu_m, f_p, f_m, dp, dm);  // ref: ...RadonIntermediate.cu:112,269,254
        if (hits0) {
            deposit_at(hits0, cell_of_offset<PITCH4>(o0p), t0p.fx, t0p.fy, w_p, mu_p);
            deposit_at(hits0, cell_of_offset<PITCH4>(o0m), t0m.fx, t0m.fy, w_m, mu_m);
        }
        if (hits1) {
            deposit_at(hits1, cell_of_offset<PITCH4>(o1p), t1p.fx, t1p.fy, w_p, mu_p);
            deposit_at(hits1, cell_of_offset<PITCH4>(o1m), t1m.fx, t1m.fy, w_m, mu_m);
        }
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
        const float mu_p = plain_tap_value(t0p, rw0, p.pitch, p.n_alpha, p.n_t, false) * plain_tap_value(t1p, rw1, p.pitch, p.n_alpha, p.n_t, false);
        const float mu_m = plain_tap_value(t0m, rw0, p.pitch, p.n_alpha, p.n_t, false) * plain_tap_value(t1m, rw1, p.pitch, p.n_alpha, p.n_t, false);
        const float dp = v0p - v1p, dm = v0m - v1m;
        const float w_p = robust_weight(L, dp), w_m = robust_weight(L, dm);
        const float f_p = mu_p * w_p, f_m = mu_m * w_m;
        const float consistency = ((f_p * dp) * dp + (f_m * dm) * dm) * w06;  // ref: ...RadonIntermediate.cu:112,254
        add(consistency * dkappa, mu_p, mu_m, f_p, f_m, dp, dm);              // ref: ...RadonIntermediate.cu:269
        if (hits0) {
            deposit_plain(hits0, p, t0p, w_p, mu_p);
            deposit_plain(hits0, p, t0m, w_m, mu_m);
        }
        if (hits1) {
            deposit_plain(hits1, p, t1p, w_p, mu_p);
            deposit_plain(hits1, p, t1m, w_m, mu_m);
        }
    }
};

// The pair's four entries from the wave's sums (lane 0), as weighted_robust_kernel.hip stores them: c, u, k, r into columns 0 .. 3.
__device__ __forceinline__ void store_weighted_robust(const EccWeightedRobustMapParams& g, long long local, const double (&acc)[WEIGHTED_ROBUST_SUMS])
{
    const bool any = acc[COUNT] > 0.0;
    g.values[local] = (float)acc[VALUE];
    g.values[g.col_stride + local] = any ? (float)(acc[MASS] / acc[COUNT]) : 1.0f;
    g.values[2 * g.col_stride + local] = any ? (float)(acc[KEPT] / acc[COUNT]) : 1.0f;
    g.values[3 * g.col_stride + local] = any ? (float)(acc[RAW] / acc[COUNT]) : 0.0f;
}

// Registers: pairs_weighted_robust_kernel's plus what the deposits cost pairs_robust_map_kernel over
// pairs_robust_kernel; tests/test_weighted_robust_map_abi.py pins the plan and what was built.
template <bool DERIV>
__global__ __launch_bounds__(PK_MAIN_THREADS) void pairs_weighted_robust_map_kernel(EccPairParams p, EccWeightedRobustMapParams g)
{
    double acc[WEIGHTED_ROBUST_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    WeightedRobustMapForm form(g, acc);
    long long local;
    if (form_main_sums<DERIV>(p, form, acc, local)) store_weighted_robust(g, local, acc);
}

// ---- ECC_SAMPLING_REFERENCE -------------------------------------------------------------------------
template <int SPLIT>
__global__ __launch_bounds__(PK_THREADS) void pairs_weighted_robust_map_reference_kernel(EccPairParams p, EccWeightedRobustMapParams g)
{
    double acc[WEIGHTED_ROBUST_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    WeightedRobustMapForm form(g, acc);
    long long local;
    if (form_reference_sums<SPLIT>(p, form, acc, local)) store_weighted_robust(g, local, acc);
}

// ---- the map as the next pass's line weights ---------------------------------------------------------
// One thread per padded element of a weight slab (rows -1 .. n_alpha, all `pitch` columns: written completely): the old weight at
// that element times the factor of the bin it replicates, one float32 multiply.  The factor is robust_map_weights_kernel's rule on
// the held float planes, every operation an IEEE float64 one.
__global__ __launch_bounds__(256) void weighted_robust_map_weights_kernel(const float* __restrict__ hits, const float* __restrict__ rejected,
                                                                          const float* const* __restrict__ weights,
                                                                          const int32_t* __restrict__ views, float* __restrict__ slabs,
                                                                          int n_alpha, int n_t, int pitch, float min_hits, float gain)
{
    const long long slab = (long long)(n_alpha + 2) * pitch, bins = (long long)n_alpha * n_t;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= slab) return;
    const int row = (int)(e / pitch), col = (int)(e - (long long)row * pitch);
    const int i = min(max(row - 1, 0), n_alpha - 1), j = min(max(col - 1, 0), n_t - 1);
    const long long bin = (long long)blockIdx.y * bins + (long long)j * n_alpha + i;
    const float h = hits[bin], r = rejected[bin];
    float factor = 1.0f;
    if (!(h < min_hits)) factor = (float)fmax(0.0, 1.0 - (double)gain * ((double)r / (double)h));
    slabs[(long long)blockIdx.y * slab + e] = weights[views[blockIdx.y]][e] * factor;
}

}  // namespace

// The four entries {c, u, k, r} of every pair of the launch p into g->values, as ecc_launch_pairs_weighted_robust (the same
// conditions on p and on the metric's intermediates), and the deposits of every sample of a mapped view into g->planes (zeroed
// earlier on the same stream).  g->slot_of has one entry per DATA intermediate, p->n_views of them.
extern "C" hipError_t ecc_launch_pairs_weighted_robust_map(const EccPairParams* p, const EccWeightedRobustMapParams* g, hipStream_t stream)
{
    if (p->count <= 0) return hipSuccess;
    if (p->use_corr || p->record_slots || p->skip_enabled || !g->values || g->col_stride < p->count || (g->col_stride & 3) ||
        g->loss < ECC_ROBUST_HUBER || g->loss > ECC_ROBUST_GEMAN_MCCLURE || !(g->delta > 0.f) || !g->planes || !g->slot_of || g->rej_cells < g->plane_cells ||
        g->plane_cells != ecc_robust_map_plane_cells(p->n_alpha, p->n_t) || g->plane_cells >= ((int64_t)1 << 31))
        return hipErrorInvalidValue;
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
