// ecc_transform_grid.h -- where the entries of a transform batch's grid lie (host and device).
//
// A batch of ecc_metric_evaluate_transforms / ecc_metric_evaluate_weighted_transforms evaluates K transforms over one cross list of
// `count` = n_source n_target pairs, q = j n_source + i.  Its grid is PAIR-major and TRANSFORM-minor:
//   entry e = q K + k        pair q of transform k
// so that neighbours in a launch sample the same Radon intermediates under slightly different geometries.  The
// values of ONE transform therefore lie K floats apart in a column of the grid, and float4 kk of the order of ecc_sum_order.h -- the
// transform's values 4 kk .. 4 kk + 3 -- is the four entries (4 kk + c) K + k.
//
// Readers: sum_weighted_transforms_kernel (weighted_transforms_kernel.hip), the host transposition of
// ecc_metric_evaluate_weighted_transforms (ecc_weighted_transforms.hip) and tests/c/transform_grid.cpp.  transform_list_kernel
// (ecc_transforms.hip) writes the grid and states the same rule inline (q = e / K, k = e - q K); it was left as it is, because the
// device code of existing kernels is held to the previous build's instruction for instruction (CHANGELOG).
#ifndef ECC_TRANSFORM_GRID_H
#define ECC_TRANSFORM_GRID_H

#if defined(__HIPCC__)
#define ECC_TRANSFORM_GRID_HD __host__ __device__ __forceinline__
#else
#define ECC_TRANSFORM_GRID_HD inline
#endif

namespace ecc_transform_grid {

// Pair q of transform k in a grid of K transforms.
ECC_TRANSFORM_GRID_HD long long entry(long long q, int k, int K) { return q * K + k; }

// Value q of transform k in a column of the grid.
ECC_TRANSFORM_GRID_HD float value(const float* col, long long q, int k, int K) { return col[entry(q, k, K)]; }

// float4 kk of transform k's values: out[c] = value 4 kk + c.
ECC_TRANSFORM_GRID_HD void gather4(const float* col, long long kk, int k, int K, float out[4])
{
    for (int c = 0; c < 4; ++c) out[c] = value(col, 4 * kk + c, k, K);
}

}  // namespace ecc_transform_grid

#endif
