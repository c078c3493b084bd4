// ecc_variance.hip -- ecc_metric_evaluate_variance and its index-list, pose-delta and transform forms, ecc_host_variance_floor: the
// metric with inverse-variance sample weights (host code; include/ecc_hip.h states the contract, variance_kernel.hip has the pair
// kernels, sum_kernel.hip, weighted_poses_kernel.hip and weighted_transforms_kernel.hip the sums).  The caller knows how noisy
// every line integral is -- a low-dose or photon-starved scan, a view behind metal -- and gives every view a second Radon
// intermediate that holds the variance of each line; a squared difference of two samples then counts with 1 / (V_i + V_j), which
// no product of per-view line weights expresses.
//
// The launch sequences are ecc_form_call.h's: form_call (all pairs, an index list), form_pose_deltas, form_transforms.  What is the
// variance form's own -- its columns, its pair launch with the floor, its division -- is variance_form below.  S = 2: the batches'
// sums are sum_weighted_poses_kernel and sum_weighted_transforms_kernel as they stand.
// Every value and mean weight of a batch has the bits of ecc_metric_set_projections + the sequential call for that pose or
// transform (tests/test_gpu_variance_batches.py); what a batch does not take is evaluated that way inside the call.
// The form combined with the robust loss is ecc_variance_robust.hip; it takes variance_check from here.
// Not here: base columns kept between calls; range, group and RCCL forms; the form under the correlation cost; a covariance-aware
// model for derivative data.
#include "ecc_form_call.h"
#include "ecc_variance_host.h"

using namespace ecc_internal;

static_assert(ecc_variance_host::OK == ECC_OK && ecc_variance_host::INVALID_ARGUMENT == ECC_ERR_INVALID_ARGUMENT,
              "ecc_variance_host.h returns the ABI's codes");

namespace ecc_internal {
// What every variance call needs of the metric and the floor (after its own null checks), before the device is touched.
int variance_check(const ecc_metric* m, float floor)
{
    if (m->n_views < 1) return fail(ECC_ERR_INVALID_ARGUMENT, "projection matrices have not been set");
    if (m->n_views < 2) return fail(ECC_ERR_INVALID_ARGUMENT, "need at least two views (the reference divides 0/0 here)");
    if ((int64_t)m->dtrs.size() != (int64_t)2 * m->n_views)
        return fail(ECC_ERR_INVALID_ARGUMENT, "the metric must hold 2 * n_views Radon intermediates: the data of every view, then its variance field");
    if (!(floor > 0.0f) || !std::isfinite(floor)) return fail(ECC_ERR_INVALID_ARGUMENT, "the variance floor must be finite and > 0");
    if (m->use_corr) return fail(ECC_ERR_UNSUPPORTED, "inverse-variance weights are not defined for the correlation cost");
    return ECC_OK;
}

PairForm variance_form(float floor, double* values, double* mean_weights)
{
    return {2, 2,  // columns: c, u; both summed
            [=](ecc_metric* m, const EccPairParams& p, float* cols, int64_t col_stride) {
                EccVarianceParams g;
                set_channel_strides(m, &g);
                g.values = cols;
                g.col_stride = col_stride;
                g.floor = floor;
                return launch_timed(m->ctx, [&](hipStream_t s) { return ecc_launch_pairs_variance(&p, &g, s); });  // (variance_kernel.hip)
            },
            [=](const double* totals, int64_t count, int64_t k) {
                // ref: ...RadonIntermediate.cpp:224 (sum value w / sum w)
                const bool none = totals[1] == 0.0;
                values[k] = none ? 0.0 : totals[0] / totals[1];
                if (mean_weights) mean_weights[k] = none ? 0.0 : totals[1] / (double)count;
            },
            ecc_form_base::VARIANCE, 0, 0.f, floor};
}
}  // namespace ecc_internal

ECC_EXPORT int ecc_metric_evaluate_variance(ecc_metric* m, float floor, double* value, double* mean_weight, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!value) return fail(ECC_ERR_INVALID_ARGUMENT, "value is null");
    int rc = variance_check(m, floor);
    if (rc) return rc;
    return form_call_all_pairs(m, variance_form(floor, value, mean_weight), pair_terms);
}

ECC_EXPORT int ecc_metric_evaluate_variance_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, float floor, double* value,
                                                  double* mean_weight, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!value) return fail(ECC_ERR_INVALID_ARGUMENT, "value is null");
    if (n_pairs < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "negative list length");
    if (n_pairs == 0) return ECC_OK;
    if (!idx4) return fail(ECC_ERR_INVALID_ARGUMENT, "index list is null");
    int rc = variance_check(m, floor);
    if (rc) return rc;
    // P index the current matrices, D the DATA intermediates: the variance of a sample comes from dtr n_views + D
    rc = check_index_list(idx4, n_pairs, m->n_views, m->n_views,
                          "index array contains invalid indices (matrices and data intermediates lie in [0, n_views))");
    if (rc) return rc;
    return form_call(m, variance_form(floor, value, mean_weight), idx4, n_pairs, pair_terms);  // the sampling mode of a list of n_pairs tuples
}

ECC_EXPORT int ecc_metric_evaluate_variance_pose_deltas(ecc_metric* m, int n_poses, const int32_t* moved_offsets, const int32_t* moved_views,
                                                        const double* moved_Ps, float floor, double* values, double* mean_weights)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!moved_offsets || !values) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    if (n_poses < 1) return ECC_OK;
    if (moved_offsets[n_poses] > 0 && (!moved_views || !moved_Ps)) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    int rc = variance_check(m, floor);
    if (!rc) rc = check_lists(m, n_poses, moved_offsets, moved_views);
    if (rc) return rc;
    return form_pose_deltas(m, variance_form(floor, values, mean_weights), n_poses, moved_offsets, moved_views, moved_Ps, [&](int k) {
        return ecc_metric_evaluate_variance(m, floor, &values[k], mean_weights ? &mean_weights[k] : nullptr, nullptr);
    });
}

ECC_EXPORT int ecc_metric_evaluate_variance_transforms(ecc_metric* m, int n_source, int n_transforms, const double* Ts, float floor,
                                                       double* values, double* mean_weights, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (n_transforms < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "n_transforms must not be negative");
    if (n_transforms > 0 && (!Ts || !values)) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    int rc = variance_check(m, floor);
    if (rc) return rc;
    if (n_source < 1 || n_source >= m->n_views)
        return fail(ECC_ERR_INVALID_ARGUMENT, "n_source must be in [1, n_views): the views [0, n_source) are the source, the rest the target");
    return form_transforms(m, variance_form(floor, values, mean_weights), n_source, n_transforms, Ts, pair_terms, "transform",
                           [&](int k, const int32_t* idx, int len, float* rows) {
                               return ecc_metric_evaluate_variance_pairs(m, idx, len, floor, &values[k], mean_weights ? &mean_weights[k] : nullptr, rows);
                           });
}

// Host only, no device (ecc_variance_host.h).
ECC_EXPORT int ecc_host_variance_floor(const float* v, int64_t count, double fraction, float* floor)
{
    const int rc = ecc_variance_host::variance_floor(v, count, fraction, floor);
    return rc ? fail(ECC_ERR_INVALID_ARGUMENT, "ecc_host_variance_floor: null pointer, negative count, a fraction not in (0, infinity), or no positive entry")
              : ECC_OK;
}
