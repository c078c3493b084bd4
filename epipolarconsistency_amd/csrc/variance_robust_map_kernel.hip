// variance_robust_map_kernel.hip -- where the robust loss rejects IN SIGMA UNITS: the metric with inverse-variance sample weights and
// a per-sample robust loss of the studentised residual as variance_robust_kernel.hip evaluates it, with every sample's bilinear
// footprint deposited into its view's own Radon space (gfx950).
//
// A metric over 2 n Radon intermediates: dtr i the data of view i, dtr n + i its variance field V_i.  Per pair and +-kappa sample the
// positions, the kappa range, the residual d, s = V_i(sample) + V_j(sample), sc, om = 1 / sc, the loss weight w of z = d / sqrt(sc)
// and f = om * w are pairs_variance_robust_kernel's in the metric's sampling mode (the weight is ecc_studentised_weight.h's, stated
// once for both files), and so are the five per-lane float64 sums and the four columns {c, u, k, r}: the trips below are
// VarianceRobustForm's, statement for statement, with the deposits behind the sums.  A sample of view v with the float32 footprint
// products b of robust_map_kernel.hip adds, per cell,
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
#include "ecc_pair_forms.h"
#include "ecc_studentised_weight.h"
#include "ecc_robust_map.h"

namespace {

// the five per-lane sums, as in variance_robust_kernel.hip: the value, the weight mass, the mass the loss keeps, the squared
// studentised residuals, the sample count
enum { VALUE, MASS, KEPT, RAW, COUNT, VARIANCE_ROBUST_SUMS };

struct VarianceRobustMapForm : PairFormDefaults, MapPlanes {
    const EccVarianceRobustMapParams& g;
    double (&acc)[VARIANCE_ROBUST_SUMS];
    StudentisedLoss L;                  // the launch-uniform loss and floor, in scalar registers
    GlobalBytes w0, w1;                 // the variance copies of the loop's two views (wave-uniform)
    GlobalFloats d0, d1, rw0, rw1;      // the reference loop's slabs: data and variances
    unsigned long long *hits0, *hits1;  // the HITS plane of the pair's two views, null: not mapped (wave-uniform)

    __device__ __forceinline__ VarianceRobustMapForm(const EccVarianceRobustMapParams& g, double (&acc)[VARIANCE_ROBUST_SUMS]) : g(g), acc(acc) {}

    __device__ __forceinline__ unsigned long long* plane_of(int iD) const
    {
        const int slot = __builtin_amdgcn_readfirstlane(g.slot_of[iD]);
        return slot < 0 ? nullptr : g.planes + (long long)slot * g.plane_cells;
    }

    __device__ __forceinline__ void begin(const EccPairParams& p, int iD0, int iD1)
    {
        L = {__builtin_amdgcn_readfirstlane(g.loss), uniformf(g.delta), uniformf(g.inv_delta), uniformf(g.floor)};
        hits0 = plane_of(iD0);
        hits1 = plane_of(iD1);
        rej_cells = g.rej_cells;
        pitch = (unsigned)p.pitch;
        last_cell = (unsigned)(g.plane_cells - 1);
    }

    // the sums of a trip beside its value
    __device__ __forceinline__ void add(float value, const StudentisedWeight p, const StudentisedWeight m, float dp, float dm)
    {
        acc[VALUE] += (double)value;
        acc[MASS] += (double)(p.om + m.om);
        acc[KEPT] += (double)(p.f + m.f);
        acc[RAW] += (double)(p.om * (dp * dp)) + (double)(m.om * (dm * dm));
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
        const float s0p = sample_tap_value(w0, t0p), s1p = sample_tap_value(w1, t1p);  // unsigned, whatever the folds
        const float s0m = sample_tap_value(w0, t0m), s1m = sample_tap_value(w1, t1m);
        const float dp = fmaf(v1p, rel_sign, v0p), dm = fmaf(v1m, rel_sign, v0m);
        const StudentisedWeight p = studentised_weight(L, s0p, s1p, dp), m = studentised_weight(L, s0m, s1m, dm);
        add(fmaf(p.f * dp, dp, (m.f * dm) * dm) * w06_dkappa, p, m, dp, dm);
        if (hits0) {
            deposit_at(hits0, t0p.off >> 3, t0p.fx, t0p.fy, p.w, 1.0f);
            deposit_at(hits0, t0m.off >> 3, t0m.fx, t0m.fy, m.w, 1.0f);
        }
        if (hits1) {
            deposit_at(hits1, t1p.off >> 3, t1p.fx, t1p.fy, p.w, 1.0f);
            deposit_at(hits1, t1m.off >> 3, t1m.fx, t1m.fy, m.w, 1.0f);
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
        const float s0p = line_tap_finish<false>(line_footprint(w0, o0p), t0p), s1p = line_tap_finish<false>(line_footprint(w1, o1p), t1p);
        const float s0m = line_tap_finish<false>(line_footprint(w0, o0m), t0m), s1m = line_tap_finish<false>(line_footprint(w1, o1m), t1m);
        const float dp = v0p - v1p, dm = v0m - v1m;
        const StudentisedWeight p = studentised_weight(L, s0p, s1p, dp), m = studentised_weight(L, s0m, s1m, dm);
        add((((p.f * dp) * dp + (m.f * dm) * dm) * w06) * dkappa, p, m, dp, dm);  // ref: ...RadonIntermediate.cu:112,269,254
        if (hits0) {
            deposit_at(hits0, cell_of_offset<PITCH4>(o0p), t0p.fx, t0p.fy, p.w, 1.0f);
            deposit_at(hits0, cell_of_offset<PITCH4>(o0m), t0m.fx, t0m.fy, m.w, 1.0f);
        }
        if (hits1) {
            deposit_at(hits1, cell_of_offset<PITCH4>(o1p), t1p.fx, t1p.fy, p.w, 1.0f);
            deposit_at(hits1, cell_of_offset<PITCH4>(o1m), t1m.fx, t1m.fy, m.w, 1.0f);
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
        const float s0p = plain_tap_value(t0p, rw0, p.pitch, p.n_alpha, p.n_t, false), s1p = plain_tap_value(t1p, rw1, p.pitch, p.n_alpha, p.n_t, false);
        const float s0m = plain_tap_value(t0m, rw0, p.pitch, p.n_alpha, p.n_t, false), s1m = plain_tap_value(t1m, rw1, p.pitch, p.n_alpha, p.n_t, false);
        const float dp = v0p - v1p, dm = v0m - v1m;
        const StudentisedWeight wp = studentised_weight(L, s0p, s1p, dp), wm = studentised_weight(L, s0m, s1m, dm);
        const float consistency = ((wp.f * dp) * dp + (wm.f * dm) * dm) * w06;  // ref: ...RadonIntermediate.cu:112,254
        add(consistency * dkappa, wp, wm, dp, dm);                              // ref: ...RadonIntermediate.cu:269
        if (hits0) {
            deposit_plain(hits0, p, t0p, wp.w, 1.0f);
            deposit_plain(hits0, p, t0m, wm.w, 1.0f);
        }
        if (hits1) {
            deposit_plain(hits1, p, t1p, wp.w, 1.0f);
            deposit_plain(hits1, p, t1m, wm.w, 1.0f);
        }
    }
};

// The pair's four entries from the wave's sums (lane 0), as variance_robust_kernel.hip stores them: c, u, k, r into columns 0 .. 3.
__device__ __forceinline__ void store_variance_robust(const EccVarianceRobustMapParams& g, long long local, const double (&acc)[VARIANCE_ROBUST_SUMS])
{
    const bool any = acc[COUNT] > 0.0;
    g.values[local] = (float)acc[VALUE];
    g.values[g.col_stride + local] = any ? (float)(acc[MASS] / acc[COUNT]) : 1.0f;
    g.values[2 * g.col_stride + local] = any ? (float)(acc[KEPT] / acc[COUNT]) : 1.0f;
    g.values[3 * g.col_stride + local] = any ? (float)(acc[RAW] / acc[COUNT]) : 0.0f;
}

// Registers: pairs_variance_robust_kernel's plus what the deposits cost pairs_robust_map_kernel over
// pairs_robust_kernel; tests/test_variance_robust_map_abi.py pins the plan and what was built.
template <bool DERIV>
__global__ __launch_bounds__(PK_MAIN_THREADS) void pairs_variance_robust_map_kernel(EccPairParams p, EccVarianceRobustMapParams g)
{
    double acc[VARIANCE_ROBUST_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    VarianceRobustMapForm form(g, acc);
    long long local;
    if (form_main_sums<DERIV>(p, form, acc, local)) store_variance_robust(g, local, acc);
}

// ---- ECC_SAMPLING_REFERENCE -------------------------------------------------------------------------
template <int SPLIT>
__global__ __launch_bounds__(PK_THREADS) void pairs_variance_robust_map_reference_kernel(EccPairParams p, EccVarianceRobustMapParams g)
{
    double acc[VARIANCE_ROBUST_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    VarianceRobustMapForm form(g, acc);
    long long local;
    if (form_reference_sums<SPLIT>(p, form, acc, local)) store_variance_robust(g, local, acc);
}

// ---- the map as the next pass's variance fields ------------------------------------------------------
// One thread per padded element of a variance slab (rows -1 .. n_alpha, all `pitch` columns: written completely).  mu is
// robust_map_weights_kernel's rule on the held float planes at the bin the element replicates, every operation an IEEE float64
// one; the variance of a bin whose samples reached it with mean loss weight mu is V / mu, the IRLS reading (a sample's effective
// variance is sigma^2 / w), capped at max_factor; before the multiply the old variance is raised to half the floor, so that two
// raised samples sum to the floor exactly and a field of zeros can be raised at all.  factor == 1: the old bits.
__global__ __launch_bounds__(256) void variance_robust_map_variances_kernel(const float* __restrict__ hits, const float* __restrict__ rejected,
                                                                            const float* const* __restrict__ variances,
                                                                            const int32_t* __restrict__ views, float* __restrict__ slabs,
                                                                            int n_alpha, int n_t, int pitch, float half, float min_hits,
                                                                            float gain, float max_factor)
{
    const long long slab = (long long)(n_alpha + 2) * pitch, bins = (long long)n_alpha * n_t;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= slab) return;
    const int row = (int)(e / pitch), col = (int)(e - (long long)row * pitch);
    const int i = min(max(row - 1, 0), n_alpha - 1), j = min(max(col - 1, 0), n_t - 1);
    const long long bin = (long long)blockIdx.y * bins + (long long)j * n_alpha + i;
    const float h = hits[bin], r = rejected[bin];
    float mu = 1.0f;
    if (!(h < min_hits)) mu = (float)fmax(0.0, 1.0 - (double)gain * ((double)r / (double)h));
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
    if (p->use_corr || p->record_slots || p->skip_enabled || !g->values || g->col_stride < p->count || (g->col_stride & 3) ||
        g->loss < ECC_ROBUST_HUBER || g->loss > ECC_ROBUST_GEMAN_MCCLURE || !(g->delta > 0.f) || !g->planes || !g->slot_of || g->rej_cells < g->plane_cells ||
        g->plane_cells != ecc_robust_map_plane_cells(p->n_alpha, p->n_t) || g->plane_cells >= ((int64_t)1 << 31))
        return hipErrorInvalidValue;
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
