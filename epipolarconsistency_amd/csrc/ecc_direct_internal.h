// ecc_direct_internal.h -- MetricDirect behind its handle: shared by ecc_direct_api.hip (all pairs, one pair) and
// ecc_direct_lists.hip (index lists, pose batches).
#ifndef ECC_DIRECT_INTERNAL_H
#define ECC_DIRECT_INTERNAL_H

#include "ecc_capi_internal.h"

struct ecc_direct {
    ecc_ctx* ctx = nullptr;
    int n_images = 0, n_u = 0, n_v = 0, n_views = 0;
    const float* images_d = nullptr;
    float* owned_images = nullptr;
    float* imagesT_d = nullptr;  // transposed copies (see direct_lines_kernel); refreshed by ecc_direct_update_images
    double object_radius_mm = 0, dkappa = 0;
    int use_fbcc = 0;
    std::vector<double> P_first;
    double* Ps_d = nullptr;
    EccDirectView* views_d = nullptr;
    int view_capacity = 0;
    // scratch, grown on demand
    EccDirectPair* pairs_d = nullptr;
    float* samples_d = nullptr;
    double* pair_metric_d = nullptr;
    int64_t batch_capacity = 0;
    int n_max_capacity = 0;
    double* total_d = nullptr;
    float* cost_d = nullptr;
    int cost_capacity = 0;
    // per view: source position (4) and object radius, on the host; per pair: the plane-angle range (see direct_ranges)
    std::vector<double> centers, radii, ranges;
    double* ranges_d = nullptr;
    int64_t ranges_capacity = 0;
    // index lists and pose batches (ecc_direct_lists.hip): everything a call hands to the device in one pinned block and its
    // device copy, the float64 values of the whole list, the segment sums, and the view table with the candidates behind it
    ecc_internal::PinnedArray<char> list_stage;
    ecc_internal::DeviceArray<char> list_in;
    ecc_internal::DeviceArray<double> list_values, list_sums;
    ecc_internal::DeviceArray<EccDirectView> list_views;
    int64_t list_batch_max = 0;  // ecc_debug_set_direct_batch; 0 = the library's own bound
};

namespace ecc_internal {
// the bound on a pair's epipolar lines for the metric's plane step
int direct_n_max(const ecc_direct* d, int* n_max);
// ref: Metric::getObjectRadius: the user's value or the first view's estimate (0 before matrices are set)
double direct_radius(const ecc_direct* d);
// room for `batch` records, 2 x batch x n_max line integrals and `batch` values
int direct_scratch(ecc_direct* d, int64_t batch, int n_max);
// ref: estimateAngularRange as computeForImagePair calls it: the upper end of the plane-angle range of the pair of source
// positions C0, C1 (4 doubles each) with the estimates r0, r1 of their views, with the HOST's asin
double direct_range(const double* C0, const double* C1, double user_radius, double r0, double r1);
}  // namespace ecc_internal

#endif
