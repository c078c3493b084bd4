// robust_map_kernel.hip -- where the robust loss rejects: the metric under a per-sample robust loss as robust_kernel.hip evaluates it,
// with every sample's bilinear footprint deposited into its view's own Radon space (gfx950).
//
// Per pair and +-kappa sample the positions, the kappa range, the residual d and the IRLS weight w = robust_weight(L, d) are
// pairs_robust_kernel's in the metric's sampling mode, and so are the four per-lane float64 sums and the three columns {c, u, r}: both
// files run the trips of RobustForm (ecc_loss_forms.h), here with MapDeposits (ecc_robust_map.h) as its deposit policy, the deposits
// behind the sums.  A sample of view v with the footprint
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
// The deposits themselves (deposit, deposit_footprint, MapPlanes, MapDeposits) are in ecc_robust_map.h, shared with the maps under
// line weights and in sigma units, weighted_robust_map_kernel.hip and variance_robust_map_kernel.hip.
// Not here (include/ecc_hip.h): pose-delta, transform, range, group and RCCL forms; use_corr.
#include <hip/hip_runtime.h>
#include <float.h>

#include "ecc_layout.h"
#include "ecc_loss_forms.h"
#include "ecc_robust_map.h"

namespace {

// Registers: pairs_robust_kernel's plus the two plane pointers, the four cells and the four products of a footprint;
// tests/test_robust_map_abi.py pins the plan and what was built.
template <bool DERIV>
__global__ __launch_bounds__(PK_MAIN_THREADS) void pairs_robust_map_kernel(EccPairParams p, EccRobustMapParams g)
{
    double acc[ROBUST_SUMS] = {0.0, 0.0, 0.0, 0.0};
    RobustForm<EccRobustMapParams, MapDeposits> form(g, acc);
    long long local;
    if (form_main_sums<DERIV>(p, form, acc, local)) store_robust(g, local, acc);
}

// ---- ECC_SAMPLING_REFERENCE -------------------------------------------------------------------------
template <int SPLIT>
__global__ __launch_bounds__(PK_THREADS) void pairs_robust_map_reference_kernel(EccPairParams p, EccRobustMapParams g)
{
    double acc[ROBUST_SUMS] = {0.0, 0.0, 0.0, 0.0};
    RobustForm<EccRobustMapParams, MapDeposits> form(g, acc);
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
// it replicates, map_mean_weight (ecc_robust_map.h): the rule of all three feedback kernels.
__global__ __launch_bounds__(256) void robust_map_weights_kernel(const float* __restrict__ hits, const float* __restrict__ rejected,
                                                                 float* __restrict__ slabs, int n_alpha, int n_t, int pitch, float min_hits, float gain)
{
    const long long slab = (long long)(n_alpha + 2) * pitch;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= slab) return;
    const float mu = map_mean_weight(hits, rejected, e, blockIdx.y, n_alpha, n_t, pitch, min_hits, gain);
    slabs[(long long)blockIdx.y * slab + e] = mu;
}

}  // namespace

// The three entries {c, u, r} of every pair of the launch p into g->values, as ecc_launch_pairs_robust, and the deposits of every
// sample of a mapped view into g->planes (zeroed earlier on the same stream).
extern "C" hipError_t ecc_launch_pairs_robust_map(const EccPairParams* p, const EccRobustMapParams* g, hipStream_t stream)
{
    if (p->count <= 0) return hipSuccess;
    if (!loss_launch_ok(*p, *g) || !map_launch_ok(*p, *g)) return hipErrorInvalidValue;
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
