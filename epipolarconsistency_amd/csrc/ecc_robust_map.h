// ecc_robust_map.h -- what robust_map_kernel.hip and ecc_robust_map.hip share: the parameters of the map launch and the geometry of
// its planes.
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

#if defined(__HIPCC__)
extern "C" hipError_t ecc_launch_pairs_robust_map(const EccPairParams* p, const EccRobustMapParams* g, hipStream_t stream);
// fixed[n_planes][plane_cells] -> out[n_planes][n_t][n_alpha] floats, (float)((double)q * 2^-32) of the folded sums
extern "C" hipError_t ecc_launch_robust_map_finish(const unsigned long long* fixed, float* out, int n_planes, int n_alpha, int n_t, int pitch,
                                                   hipStream_t stream);
// hits, rejected: n_views float planes each (n_t x n_alpha) -> n_views weight slabs in the private layout, written completely
extern "C" hipError_t ecc_launch_robust_map_weights(const float* hits, const float* rejected, float* slabs, int n_views, int n_alpha, int n_t,
                                                    int pitch, float min_hits, float gain, hipStream_t stream);
#endif

#endif
