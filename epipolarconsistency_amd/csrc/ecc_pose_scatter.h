// ecc_pose_scatter.h -- where the pair values of a pose batch's grid go in the all-pairs order (host and device).
//
// A pose of ecc_metric_evaluate_pose_deltas / ecc_metric_evaluate_weighted_pose_deltas moves the views M[0 .. c), strictly ascending.
// Its grid has one column per moved view and one entry per partner u = 0 .. n - 1: entry (u, a) is the pair {u, M[a]} -- or a HOLE,
// which holds nothing anybody reads:
//   u == M[a]                the moved view with itself;
//   u == M[b] for a b < a    a pair of two moved views: it is counted ONCE, at entry (M[a], b) in the column of the lower of the two
//                            views, where pose_list_kernel (ecc_poses.hip) evaluates it with both moved geometries.
// Every other entry is the value of pair (i, j) = (min, max) of {u, M[a]}, which an all-pairs evaluation keeps at
//   ij = i n - i (i + 1) / 2 + (j - i - 1)                                        (ecc_get_ij's order, ecc_layout.h).
// The segmented sums walk the base's values in chunks of STAGE_F4 float4 and put the pose's own over them at these positions.
//
// Readers: sum_weighted_poses_kernel (weighted_poses_kernel.hip) and tests/c/pose_scatter.cpp.  sum_poses_kernel and
// pose_list_kernel (ecc_poses.hip) state the same rule inline and were left as they are: rewritten on position() both compile to
// other instructions than before (other register assignment and branch layout in pose_list_kernel, which also finds the extended
// geometry index of a moved partner in its scan over M; 75 differing lines of disassembly in sum_poses_kernel), and the device
// code of existing kernels is held to the previous build's instruction for instruction (CHANGELOG).
#ifndef ECC_POSE_SCATTER_H
#define ECC_POSE_SCATTER_H

#include "ecc_sum_order.h"

#if defined(__HIPCC__)
#define ECC_POSE_SCATTER_HD __host__ __device__ __forceinline__
#else
#define ECC_POSE_SCATTER_HD inline
#endif

namespace ecc_pose_scatter {

constexpr int STAGE_F4 = 2 * ecc_sum::THREADS;  // float4 per staged chunk: every thread's k, k + THREADS -- its own order is kept across chunks
constexpr long long HOLE = -1;

// Entry (partner u, column a) of a pose that moves M[0 .. a] (and possibly more views behind them): HOLE, or the pair's position.
ECC_POSE_SCATTER_HD long long position(int u, int a, const int* M, int n)
{
    const int v = M[a];
    bool hole = u == v;
    for (int b = 0; b < a; ++b) hole = hole || M[b] == u;
    if (hole) return HOLE;
    const long long i = u < v ? u : v, j = u < v ? v : u;
    return i * n - i * (i + 1) / 2 + (j - i - 1);
}

}  // namespace ecc_pose_scatter

#endif
