// robust_map_kernel.hip -- where the robust loss rejects: the metric under a per-sample robust loss as robust_kernel.hip evaluates it,
// with every sample's bilinear footprint deposited into its view's own Radon space (gfx950).
//
// Per pair and +-kappa sample the positions, the kappa range, the residual d and the IRLS weight w = robust_weight(L, d) are
// pairs_robust_kernel's in the metric's sampling mode, and so are the four per-lane float64 sums and the three columns {c, u, r}: the
// trips below are RobustForm's, statement for statement, with the deposits behind the sums.  A sample of view v with the footprint
// (i0, i1) x (j0, j1), the fractions fx (angle) and fy (distance) and the weight w adds, with b the float32 products
// (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy of the four cells,
//     HITS_v[cell] += b                 REJ_v[cell] += b * (1 - w)            ((1 - w) and the product in float32)
// at exactly the cells its gather reads: the map is the adjoint of the sampling.  Both planes are unsigned 64-bit FIXED POINT with
// quantum 2^-32: a deposit is (unsigned long long)(x * 4294967296.0f), exact (a power of two times 24 bits), and integer addition
// commutes -- the same inputs give the same bits in any launch order, which a float atomic sum does not.  The deposits are plain
// atomicAdd on unsigned long long, results unused: vector global atomics without return.  No inline assembly here.
// Where the deposits go (ecc_robust_map.h): a plane has the slab's padded geometry, one 8-byte cell per 8-byte cell of the row-paired
// copy at the same pitch, so a SampleTap's byte offset (a LineTap's pointer minus the copy's origin) addresses the first cell; the
// row-quad copies' offsets are decoded to (row, bin) first; the reference loop forms the clamped cells as slab_tex2d_norm does.
// robust_map_finish_kernel folds the replicated border into the clamped bins -- clamped cells that coincide have received both
// deposits -- and turns the sums into float planes, n_t x n_alpha, alpha fastest; robust_map_weights_kernel turns two float planes
// into a line-weight slab.
// Whether a view is mapped, and where its planes are, is wave-uniform (the record's two data indices are): a side that is not mapped
// is skipped by a scalar branch.  The REJ deposits of a sample with w == 1.0f add zero and are skipped: most samples are inliers.
// The deposits themselves (deposit, deposit_footprint, MapPlanes) are in ecc_robust_map.h, shared with the map under line weights,
// weighted_robust_map_kernel.hip.
// Not here (include/ecc_hip.h): pose-delta, transform, range, group and RCCL forms; use_corr.
#include <hip/hip_runtime.h>
#include <float.h>

#include "ecc_layout.h"
#include "ecc_pair_forms.h"
#include "ecc_robust_weight.h"
#include "ecc_robust_map.h"

namespace {

// the four per-lane sums, as in robust_kernel.hip: the value, the weight mass, the raw squares, the sample count
enum { VALUE, MASS, RAW, COUNT, ROBUST_SUMS };

struct RobustMapForm : PairFormDefaults, MapPlanes {
    const EccRobustMapParams& g;
    double (&acc)[ROBUST_SUMS];
    RobustLoss L;                      // the launch-uniform loss, in scalar registers
    GlobalFloats d0, d1;               // the reference loop's slabs
    unsigned long long *hits0, *hits1;  // the HITS plane of the pair's two views, null: not mapped (wave-uniform)

    __device__ __forceinline__ RobustMapForm(const EccRobustMapParams& g, double (&acc)[ROBUST_SUMS]) : g(g), acc(acc) {}

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
        if (hits0) {
            deposit_at(hits0, t0p.off >> 3, t0p.fx, t0p.fy, w_p, 1.0f);
            deposit_at(hits0, t0m.off >> 3, t0m.fx, t0m.fy, w_m, 1.0f);
        }
        if (hits1) {
            deposit_at(hits1, t1p.off >> 3, t1p.fx, t1p.fy, w_p, 1.0f);
            deposit_at(hits1, t1m.off >> 3, t1m.fx, t1m.fy, w_m, 1.0f);
        }
    }

    template <bool DERIV, int PITCH4>
    __device__ __forceinline__ void exact_trip(const SlabView sv0, const SlabView sv1, const LineTap t0p, const LineTap t1p, const LineTap t0m,
                                               const LineTap t1m, float w06, float dkappa)
    {
        const auto tap = [](const LineTap& t) { return line_tap_finish<DERIV>(line_footprint((GlobalBytes)t.ptr, 0u), t); };
        const float v0p = tap(t0p), v1p = tap(t1p), v0m = tap(t0m), v1m = tap(t1m);
        const float dp = v0p - v1p, dm = v0m - v1m;
        const float w_p = robust_weight(L, dp), w_m = robust_weight(L, dm);
        add((((w_p * dp) * dp + (w_m * dm) * dm) * w06) * dkappa, w_p, w_m, dp, dm);  // ref: ...RadonIntermediate.cu:112,269,254
        if (hits0) {
            deposit_at(hits0, cell_of_offset<PITCH4>(line_tap_offset(t0p, sv0)), t0p.fx, t0p.fy, w_p, 1.0f);
            deposit_at(hits0, cell_of_offset<PITCH4>(line_tap_offset(t0m, sv0)), t0m.fx, t0m.fy, w_m, 1.0f);
        }
        if (hits1) {
            deposit_at(hits1, cell_of_offset<PITCH4>(line_tap_offset(t1p, sv1)), t1p.fx, t1p.fy, w_p, 1.0f);
            deposit_at(hits1, cell_of_offset<PITCH4>(line_tap_offset(t1m, sv1)), t1m.fx, t1m.fy, w_m, 1.0f);
        }
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
        if (hits0) {
            deposit_plain(hits0, p, t0p, w_p, 1.0f);
            deposit_plain(hits0, p, t0m, w_m, 1.0f);
        }
        if (hits1) {
            deposit_plain(hits1, p, t1p, w_p, 1.0f);
            deposit_plain(hits1, p, t1m, w_m, 1.0f);
        }
    }
};

// The pair's three entries from the wave's sums (lane 0), as robust_kernel.hip stores them.
__device__ __forceinline__ void store_robust(const EccRobustMapParams& g, long long local, const double (&acc)[ROBUST_SUMS])
{
    const bool any = acc[COUNT] > 0.0;
    g.values[local] = (float)acc[VALUE];
    g.values[g.col_stride + local] = any ? (float)(acc[MASS] / acc[COUNT]) : 1.0f;
    g.values[2 * g.col_stride + local] = any ? (float)(acc[RAW] / acc[COUNT]) : 0.0f;
}

// Registers: pairs_robust_kernel's plus the two plane pointers, the four cells and the four products of a footprint;
// tests/test_robust_map_abi.py pins the plan and what was built.
template <bool DERIV>
__global__ __launch_bounds__(PK_MAIN_THREADS) void pairs_robust_map_kernel(EccPairParams p, EccRobustMapParams g)
{
    double acc[ROBUST_SUMS] = {0.0, 0.0, 0.0, 0.0};
    RobustMapForm form(g, acc);
    long long local;
    if (form_main_sums<DERIV>(p, form, acc, local)) store_robust(g, local, acc);
}

// ---- ECC_SAMPLING_REFERENCE -------------------------------------------------------------------------
template <int SPLIT>
__global__ __launch_bounds__(PK_THREADS) void pairs_robust_map_reference_kernel(EccPairParams p, EccRobustMapParams g)
{
    double acc[ROBUST_SUMS] = {0.0, 0.0, 0.0, 0.0};
    RobustMapForm form(g, acc);
    long long local;
    if (form_reference_sums<SPLIT>(p, form, acc, local)) store_robust(g, local, acc);
}

// ---- fixed point -> float planes -------------------------------------------------------------------
// One 32 x 32 tile of bins per workgroup of 32 x 8 threads: the padded cells are read along the distance axis (their fast one), the
// float planes written along the angle axis (theirs).  Bin (i, j) is the sum of the padded cells that clamp to it: rows {0, 1} for
// i = 0, {n_alpha, n_alpha + 1} for i = n_alpha - 1, the same for the bins -- integer sums, in a fixed order.
constexpr int FIN_TILE = 32, FIN_ROWS = 8;

__global__ __launch_bounds__(FIN_TILE* FIN_ROWS) void robust_map_finish_kernel(const unsigned long long* __restrict__ fixed, float* __restrict__ out,
                                                                               int n_alpha, int n_t, int pitch)
{
    __shared__ float tile[FIN_TILE][FIN_TILE + 1];
    const long long cells = (long long)(n_alpha + 2) * pitch;
    const unsigned long long* plane = fixed + (long long)blockIdx.z * cells;
    float* dst = out + (long long)blockIdx.z * n_alpha * n_t;
    const int i0 = blockIdx.y * FIN_TILE, j0 = blockIdx.x * FIN_TILE;
    for (int r = threadIdx.y; r < FIN_TILE; r += FIN_ROWS) {
        const int i = i0 + r, j = j0 + (int)threadIdx.x;
        if (i < n_alpha && j < n_t) {
            const int ra = i == 0 ? 0 : i + 1, rb = i == n_alpha - 1 ? n_alpha + 1 : i + 1;
            const int ba = j == 0 ? 0 : j + 1, bb = j == n_t - 1 ? n_t + 1 : j + 1;
            unsigned long long q = 0;
            for (int row = ra; row <= rb; ++row)
                for (int bin = ba; bin <= bb; ++bin) q += plane[(long long)row * pitch + bin];
            tile[r][threadIdx.x] = (float)((double)q * 2.3283064365386963e-10);  // 2^-32
        }
    }
    __syncthreads();
    for (int r = threadIdx.y; r < FIN_TILE; r += FIN_ROWS) {
        const int j = j0 + r, i = i0 + (int)threadIdx.x;
        if (i < n_alpha && j < n_t) dst[(long long)j * n_alpha + i] = tile[threadIdx.x][r];
    }
}

// ---- the map as line weights -------------------------------------------------------------------------
// One thread per padded element of a weight slab (rows -1 .. n_alpha, all `pitch` columns: written completely): the weight of the bin
// it replicates.  Every operation an IEEE float64 one.
__global__ __launch_bounds__(256) void robust_map_weights_kernel(const float* __restrict__ hits, const float* __restrict__ rejected,
                                                                 float* __restrict__ slabs, int n_alpha, int n_t, int pitch, float min_hits, float gain)
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
    slabs[(long long)blockIdx.y * slab + e] = mu;
}

}  // namespace

// The three entries {c, u, r} of every pair of the launch p into g->values, as ecc_launch_pairs_robust, and the deposits of every
// sample of a mapped view into g->planes (zeroed earlier on the same stream).
extern "C" hipError_t ecc_launch_pairs_robust_map(const EccPairParams* p, const EccRobustMapParams* g, hipStream_t stream)
{
    if (p->count <= 0) return hipSuccess;
    if (p->use_corr || p->record_slots || p->skip_enabled || !g->values || g->col_stride < p->count || (g->col_stride & 3) ||
        g->loss < ECC_ROBUST_HUBER || g->loss > ECC_ROBUST_GEMAN_MCCLURE || !(g->delta > 0.f) || !g->planes || !g->slot_of || g->rej_cells < g->plane_cells ||
        g->plane_cells != ecc_robust_map_plane_cells(p->n_alpha, p->n_t) || g->plane_cells >= ((int64_t)1 << 31))
        return hipErrorInvalidValue;
    return launch_pair_form(*p, *g, stream, pairs_robust_map_reference_kernel<4>, pairs_robust_map_reference_kernel<1>,
                            pairs_robust_map_kernel<true>, pairs_robust_map_kernel<false>);
}

extern "C" hipError_t ecc_launch_robust_map_finish(const unsigned long long* fixed, float* out, int n_planes, int n_alpha, int n_t, int pitch,
                                                   hipStream_t stream)
{
    if (n_planes <= 0) return hipSuccess;
    if (n_planes > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((n_t + FIN_TILE - 1) / FIN_TILE), (unsigned)((n_alpha + FIN_TILE - 1) / FIN_TILE), (unsigned)n_planes);
    hipLaunchKernelGGL(robust_map_finish_kernel, grid, dim3(FIN_TILE, FIN_ROWS), 0, stream, fixed, out, n_alpha, n_t, pitch);
    return hipGetLastError();
}

extern "C" hipError_t ecc_launch_robust_map_weights(const float* hits, const float* rejected, float* slabs, int n_views, int n_alpha, int n_t,
                                                    int pitch, float min_hits, float gain, hipStream_t stream)
{
    if (n_views <= 0) return hipSuccess;
    if (n_views > 65535) return hipErrorInvalidValue;
    const long long slab = (long long)(n_alpha + 2) * pitch;
    hipLaunchKernelGGL(robust_map_weights_kernel, dim3((unsigned)((slab + 255) / 256), (unsigned)n_views), dim3(256), 0, stream, hits, rejected,
                       slabs, n_alpha, n_t, pitch, min_hits, gain);
    return hipGetLastError();
}
