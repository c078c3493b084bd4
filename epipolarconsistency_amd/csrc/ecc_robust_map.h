// ecc_robust_map.h -- what the three map kernels (robust_map_kernel.hip, weighted_robust_map_kernel.hip,
// variance_robust_map_kernel.hip) and their host files (ecc_robust_map.hip, ecc_weighted_robust_map.hip,
// ecc_variance_robust_map.hip) share: the parameters of the map launches, the geometry of the planes, the
// deposits, the deposit policy MapDeposits of the loss forms (ecc_loss_forms.h), the feedback kernels' rule and the map launches'
// argument check (for the kernel files) and the launch sequence of a map call (for the host files) (DESIGN.md 4.24, 4.25, 4.31,
// 4.33).
//
// The map of a view is two planes, HITS and REJ, of unsigned 64-bit fixed point with quantum 2^-32.  On the device a plane has the
// geometry of the view's slab (ecc_layout.h): (n_alpha + 2) rows of `pitch` cells, cell (row, bin) for the padded element
// (ix = row - 1, iy = bin - 1).  One cell is 8 bytes, as one cell of the row-paired copy is, and the pitch is the same: a tap's byte
// offset inside the paired copy IS the byte offset of its first cell inside a plane, the other three are +8, +pitch4 and +pitch4 + 8.
// The deposits of a sample go to the four padded cells its gather reads; robust_map_finish_kernel folds the replicated border back
// into the clamped bins and writes float planes of n_t x n_alpha, alpha fastest.
#ifndef ECC_ROBUST_MAP_H
#define ECC_ROBUST_MAP_H

#include "ecc_layout.h"

static inline int64_t ecc_robust_map_plane_cells(int n_alpha, int n_t) { return ecc_layout_floats(n_alpha, n_t); }

struct EccRobustMapParams {
    float* values;               // 3 columns of col_stride floats: c, u, r as EccRobustParams
    int64_t col_stride;
    int loss;                    // ECC_ROBUST_*, launch-uniform
    float delta;                 // the scale, > 0; +infinity: no sample is down-weighted
    float inv_delta;             // (float)(1.0 / (double)delta), formed on the host
    unsigned long long* planes;  // the HITS plane of every mapped view, then their REJ planes: plane_cells cells each, zero before the launch
    const int32_t* slot_of;      // per Radon intermediate of the metric: which plane is its view's, or -1: not mapped
    int64_t plane_cells;         // (n_alpha + 2) * pitch
    int64_t rej_cells;           // cells from a view's HITS plane to its REJ plane: mapped views * plane_cells
};

// The map under line weights (weighted_robust_map_kernel.hip): EccWeightedRobustParams' fields -- 2 n_views channel-major
// intermediates, four columns {c, u, k, r} -- then the planes as above; slot_of has n_views entries, one per DATA intermediate.
struct EccWeightedRobustMapParams {
    int64_t paired_channel_bytes;  // as in EccGramParams
    int64_t quad_channel_bytes;
    float* values;                 // 4 columns of col_stride floats
    int64_t col_stride;
    int loss;
    float delta;
    float inv_delta;
    unsigned long long* planes;
    const int32_t* slot_of;
    int64_t plane_cells;
    int64_t rej_cells;
};

// The map in sigma units (variance_robust_map_kernel.hip): EccVarianceRobustParams' fields -- 2 n_views channel-major intermediates,
// the data and their variance fields, four columns {c, u, k, r} -- then the planes as above; slot_of has n_views entries, one per
// DATA intermediate.
struct EccVarianceRobustMapParams {
    int64_t paired_channel_bytes;  // as in EccGramParams
    int64_t quad_channel_bytes;
    float* values;                 // 4 columns of col_stride floats
    int64_t col_stride;
    float floor;                   // as in EccVarianceParams; launch-uniform
    int loss;
    float delta;                   // the scale in sigmas
    float inv_delta;
    unsigned long long* planes;
    const int32_t* slot_of;
    int64_t plane_cells;
    int64_t rej_cells;
};

#if defined(__HIPCC__)
extern "C" hipError_t ecc_launch_pairs_robust_map(const EccPairParams* p, const EccRobustMapParams* g, hipStream_t stream);
// fixed[n_planes][plane_cells] -> out[n_planes][n_t][n_alpha] floats, (float)((double)q * 2^-32) of the folded sums
extern "C" hipError_t ecc_launch_robust_map_finish(const unsigned long long* fixed, float* out, int n_planes, int n_alpha, int n_t, int pitch,
                                                   hipStream_t stream);
// hits, rejected: n_views float planes each (n_t x n_alpha) -> n_views weight slabs in the private layout, written completely
extern "C" hipError_t ecc_launch_robust_map_weights(const float* hits, const float* rejected, float* slabs, int n_views, int n_alpha, int n_t,
                                                    int pitch, float min_hits, float gain, hipStream_t stream);
extern "C" hipError_t ecc_launch_pairs_weighted_robust_map(const EccPairParams* p, const EccWeightedRobustMapParams* g, hipStream_t stream);
// slabs[k] = weights[views[k]] * factor(hits[k], rejected[k]) per padded element, k in [0, n_mapped): weights are the slabs of the
// metric's weight intermediates (device table), views the mapped data indices (device), written completely
extern "C" hipError_t ecc_launch_weighted_robust_map_weights(const float* hits, const float* rejected, const float* const* weights,
                                                             const int32_t* views, float* slabs, int n_mapped, int n_alpha, int n_t, int pitch,
                                                             float min_hits, float gain, hipStream_t stream);
extern "C" hipError_t ecc_launch_pairs_variance_robust_map(const EccPairParams* p, const EccVarianceRobustMapParams* g, hipStream_t stream);
// slabs[k] = the next pass's variance field of view views[k] per padded element, k in [0, n_mapped), written completely: variances
// are the slabs of the metric's variance intermediates (device table), views the mapped data indices (device); the rule is
// include/ecc_hip.h's (ecc_metric_variance_robust_map_variances), half = 0.5f * floor
extern "C" hipError_t ecc_launch_variance_robust_map_variances(const float* hits, const float* rejected, const float* const* variances,
                                                               const int32_t* views, float* slabs, int n_mapped, int n_alpha, int n_t, int pitch,
                                                               float floor, float min_hits, float gain, float max_factor, hipStream_t stream);
#endif

// ---- the deposits: for the kernel files, behind ecc_pair_forms.h ---------------------------------------------------------------
#if defined(ECC_PAIR_FORMS_H)
namespace {

// a deposit in fixed point: exact for a float32 in [0, 2^32)
__device__ __forceinline__ void deposit(unsigned long long* cell, float x)
{
    atomicAdd(cell, (unsigned long long)(x * 4294967296.0f));
}

// The footprint of one sample into the HITS plane `hits` and the REJ plane `rej_cells` cells behind it.  c00 = (i0, j0), c10 = (i1, j0),
// c01 = (i0, j1), c11 = (i1, j1) as cell indices; fx runs over i (angle rows), fy over j (distance bins).  mu: the sample's product of
// line weights, one float32 multiply per cell (the literal 1.0f for the map without weights: x * 1.0f is x and the compiler drops
// both the multiply and the test).  Deposits of zero are skipped, they change no bit: all of them where mu == 0.0f, the REJ half
// where w == 1.0f.  No address depends on mu or w.
__device__ __forceinline__ void deposit_footprint(unsigned long long* hits, long long rej_cells, unsigned c00, unsigned c10, unsigned c01,
                                                  unsigned c11, float fx, float fy, float w, float mu)
{
    if (mu == 0.0f) return;
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const float b00 = (gx * gy) * mu, b10 = (fx * gy) * mu, b01 = (gx * fy) * mu, b11 = (fx * fy) * mu;
    deposit(hits + c00, b00);
    deposit(hits + c10, b10);
    deposit(hits + c01, b01);
    deposit(hits + c11, b11);
    if (w != 1.0f) {
        const float q = 1.0f - w;
        unsigned long long* rej = hits + rej_cells;
        deposit(rej + c00, b00 * q);
        deposit(rej + c10, b10 * q);
        deposit(rej + c01, b01 * q);
        deposit(rej + c11, b11 * q);
    }
}

// What a map form knows of its planes (wave-uniform, set in the form's begin hook), and the deposits of the three loop kinds.
struct MapPlanes {
    long long rej_cells;        // cells from a HITS plane to its REJ plane
    unsigned pitch, last_cell;  // cells per row; the last cell of a plane

    // a footprint whose first cell is `cell` of the padded plane: the gather's own four cells (never past the plane: a footprint the
    // gather may read lies inside the paired copy, one row shorter than the plane; the comparison is the deposit's own guard)
    __device__ __forceinline__ void deposit_at(unsigned long long* hits, unsigned cell, float fx, float fy, float w, float mu) const
    {
        if (cell + pitch + 1u > last_cell) return;
        deposit_footprint(hits, rej_cells, cell, cell + pitch, cell + 1u, cell + pitch + 1u, fx, fy, w, mu);
    }

    // byte offset of a footprint inside a copy of the layout PITCH4 -> its first cell
    template <int PITCH4>
    __device__ __forceinline__ unsigned cell_of_offset(unsigned off) const
    {
        if (PITCH4 != ECC_QUAD_LAYOUT) return off >> 3;
        // row-quad copy (footprint_offset): group (r >> 2) of pitch * 64 bytes, 64 bytes per bin, 16 per row of the group
        const unsigned line = off >> 6, group = line / pitch;
        return ((group << 2) + ((off >> 4) & 3u)) * pitch + (line - group * pitch);
    }

    // the footprint of slab_tex2d_norm at (a, d): its cell, its fractions and its four clamped texels, as padded cells
    __device__ __forceinline__ void deposit_plain(unsigned long long* hits, const EccPairParams& p, const PlainTap t, float w, float mu) const
    {
        const float x = t.a * (float)p.n_alpha, y = t.d * (float)p.n_t;
        const float xb = x - 0.5f, yb = y - 0.5f;
        const float fi = floorf(xb), fj = floorf(yb);
        const float fx = xb - fi, fy = yb - fj;
        const int i = (int)fmaxf(fminf(fi, 1e9f), -1e9f), j = (int)fmaxf(fminf(fj, 1e9f), -1e9f);
        const unsigned r0 = (unsigned)(min(max(i, 0), p.n_alpha - 1) + 1), r1 = (unsigned)(min(max(i + 1, 0), p.n_alpha - 1) + 1);
        const unsigned b0 = (unsigned)(min(max(j, 0), p.n_t - 1) + 1), b1 = (unsigned)(min(max(j + 1, 0), p.n_t - 1) + 1);
        deposit_footprint(hits, rej_cells, r0 * pitch + b0, r1 * pitch + b0, r0 * pitch + b1, r1 * pitch + b1, fx, fy, w, mu);
    }
};

// The deposit policy of a map kernel: the base a loss form (ecc_loss_forms.h) takes in NoMap's place.  The hooks run behind the
// sums of a trip with the trip's four taps, the loss weights w of the + and the - sample and the factor mu of their deposits (the
// literal 1.0f for the maps in count units: it reaches deposit_footprint as a constant).  A sample is deposited into both views of
// its pair, each with its own footprint.
struct MapDeposits : MapPlanes {
    unsigned long long *hits0, *hits1;  // the HITS plane of the pair's two views, null: not mapped (wave-uniform)

    template <class G>
    __device__ __forceinline__ void map_begin(const G& g, const EccPairParams& p, int iD0, int iD1)
    {
        const auto plane_of = [&g](int iD) -> unsigned long long* {
            const int slot = __builtin_amdgcn_readfirstlane(g.slot_of[iD]);
            return slot < 0 ? nullptr : g.planes + (long long)slot * g.plane_cells;
        };
        hits0 = plane_of(iD0);
        hits1 = plane_of(iD1);
        rej_cells = g.rej_cells;
        pitch = (unsigned)p.pitch;
        last_cell = (unsigned)(g.plane_cells - 1);
    }

    // a polynomial loop's taps: the byte offset inside the row-paired copy is the cell's
    __device__ __forceinline__ void map_poly(const SampleTap t0p, const SampleTap t1p, const SampleTap t0m, const SampleTap t1m, float w_p,
                                             float w_m, float mu_p, float mu_m) const
    {
        if (hits0) {
            deposit_at(hits0, t0p.off >> 3, t0p.fx, t0p.fy, w_p, mu_p);
            deposit_at(hits0, t0m.off >> 3, t0m.fx, t0m.fy, w_m, mu_m);
        }
        if (hits1) {
            deposit_at(hits1, t1p.off >> 3, t1p.fx, t1p.fy, w_p, mu_p);
            deposit_at(hits1, t1m.off >> 3, t1m.fx, t1m.fy, w_m, mu_m);
        }
    }

    // an exact loop's taps: the offset inside the copy of the layout PITCH4, decoded
    template <int PITCH4>
    __device__ __forceinline__ void map_exact(const SlabView sv0, const SlabView sv1, const LineTap t0p, const LineTap t1p, const LineTap t0m,
                                              const LineTap t1m, float w_p, float w_m, float mu_p, float mu_m) const
    {
        if (hits0) {
            deposit_at(hits0, cell_of_offset<PITCH4>(line_tap_offset(t0p, sv0)), t0p.fx, t0p.fy, w_p, mu_p);
            deposit_at(hits0, cell_of_offset<PITCH4>(line_tap_offset(t0m, sv0)), t0m.fx, t0m.fy, w_m, mu_m);
        }
        if (hits1) {
            deposit_at(hits1, cell_of_offset<PITCH4>(line_tap_offset(t1p, sv1)), t1p.fx, t1p.fy, w_p, mu_p);
            deposit_at(hits1, cell_of_offset<PITCH4>(line_tap_offset(t1m, sv1)), t1m.fx, t1m.fy, w_m, mu_m);
        }
    }

    // the reference loop's taps: the clamped cells of the plain sampler
    __device__ __forceinline__ void map_plain(const EccPairParams& p, const PlainTap t0p, const PlainTap t1p, const PlainTap t0m,
                                              const PlainTap t1m, float w_p, float w_m, float mu_p, float mu_m) const
    {
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

// What the three feedback kernels share: the padded element e of view `view`'s slab -> the bin it replicates -> the mean loss
// weight of the samples that reached the bin, max(0, 1 - gain * REJ / HITS) on the held float planes, every operation an IEEE
// float64 one; 1.0f where fewer than min_hits reached it.
__device__ __forceinline__ float map_mean_weight(const float* __restrict__ hits, const float* __restrict__ rejected, long long e, long long view,
                                                 int n_alpha, int n_t, int pitch, float min_hits, float gain)
{
    const long long bins = (long long)n_alpha * n_t;
    const int row = (int)(e / pitch), col = (int)(e - (long long)row * pitch);
    const int i = min(max(row - 1, 0), n_alpha - 1), j = min(max(col - 1, 0), n_t - 1);
    const long long bin = view * bins + (long long)j * n_alpha + i;
    const float h = hits[bin], r = rejected[bin];
    float mu = 1.0f;
    if (!(h < min_hits)) mu = (float)fmax(0.0, 1.0 - (double)gain * ((double)r / (double)h));
    return mu;
}

// the argument check the three map launch functions share, behind the loss's own (ecc_loss_forms.h): the planes and their table
// there, the REJ planes behind all HITS planes, a plane of the launch's padded geometry and addressable by an unsigned cell
template <class G>
inline bool map_launch_ok(const EccPairParams& p, const G& g)
{
    return !(!g.planes || !g.slot_of || g.rej_cells < g.plane_cells || g.plane_cells != ecc_robust_map_plane_cells(p.n_alpha, p.n_t) ||
             g.plane_cells >= ((int64_t)1 << 31));
}

}  // namespace
#endif

// ---- the launch sequence of a map call: for the host files, behind ecc_form_call.h ---------------------------------------------
#if defined(ECC_FORM_CALL_H)
namespace ecc_internal {
// ecc_robust_map.hip: everything of a map call behind the checks of its evaluation.  f: the evaluation's form with the map kernels
// behind its launch; nD: the intermediates a sample can lie in (the entries of the plane table); kind: which kind of map the
// metric holds afterwards.
int robust_map_call(ecc_metric* m, const PairForm& f, EccMapKind kind, const int32_t* idx4, int64_t count, int nD, const int32_t* views,
                    int n_mapped, float* hits, float* rejected, float* pair_terms);
// ecc_robust_map.hip: everything of a feedback call (the held map as the next pass's weights or variances) behind its own argument
// checks and its held-map check: one slab per mapped view on the metric's device, launch(hits, rejected, slabs, n_mapped) on the
// context's stream -- hits and rejected the held float planes --, no wait, and the handles over the slabs in out[0 .. n_mapped).
int robust_map_feedback(ecc_metric* m, const std::function<hipError_t(const float*, const float*, float*, int)>& launch, ecc_dtr** out);
}  // namespace ecc_internal
#endif

#endif
