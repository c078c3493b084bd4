// ecc_weighted_poses.hip -- the metric with per-line weights (ecc_weighted.hip, weighted_kernel.hip) for the callers that have such
// data: pose optimisers.  Host code; include/ecc_hip.h states the contracts.
//
// ecc_metric_evaluate_weighted_pairs        an index list of (P0, P1, D0, D1) tuples: form_call over the list (ecc_form_call.h)
// ecc_metric_evaluate_weighted_pose_deltas  K poses that each replace a few views of the current matrices (the lists of
//                                           ecc_metric_evaluate_pose_deltas, ecc_poses.hip): form_pose_deltas with the weighted form;
//                                           values[k] = sum c / sum u, coverages[k] = sum u / n_pairs
// Every value and coverage has the bits of ecc_metric_set_projections + ecc_metric_evaluate_weighted for that pose
// (tests/test_gpu_weighted_poses.py).  What the batch does not take is evaluated that way inside the call.
// Not here: base columns kept between calls (a stale column is a silently wrong result; keeping them needs change tracking over
// matrices, parameters, sampling mode, quad copies and ecc_metric_refresh_dtrs); the full-matrices, strided, group and RCCL forms;
// an incremental mode for the weighted value; a one-launch small path for weighted lists.
#include "ecc_form_call.h"

using namespace ecc_internal;

ECC_EXPORT int ecc_metric_evaluate_weighted_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, double* value, double* coverage, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!value) return fail(ECC_ERR_INVALID_ARGUMENT, "value is null");
    if (n_pairs < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "negative list length");
    if (n_pairs == 0) return ECC_OK;
    if (!idx4) return fail(ECC_ERR_INVALID_ARGUMENT, "index list is null");
    int rc = weighted_check(m);
    if (rc) return rc;
    // P index the current matrices, D the DATA intermediates: the weights of a sample come from dtr n_views + D
    rc = check_index_list(idx4, n_pairs, m->n_views, m->n_views,
                          "index array contains invalid indices (matrices and data intermediates lie in [0, n_views))");
    if (rc) return rc;
    return form_call(m, weighted_form(value, coverage), idx4, n_pairs, pair_terms);  // the sampling mode of a list of n_pairs tuples, as ecc_metric_evaluate_pairs
}

ECC_EXPORT int ecc_metric_evaluate_weighted_pose_deltas(ecc_metric* m, int n_poses, const int32_t* moved_offsets, const int32_t* moved_views,
                                                        const double* moved_Ps, double* values, double* coverages)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!moved_offsets || !values) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    if (n_poses < 1) return ECC_OK;
    if (moved_offsets[n_poses] > 0 && (!moved_views || !moved_Ps)) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    int rc = weighted_check(m);
    if (!rc) rc = check_lists(m, n_poses, moved_offsets, moved_views);
    if (rc) return rc;
    return form_pose_deltas(m, weighted_form(values, coverages), n_poses, moved_offsets, moved_views, moved_Ps, [&](int k) {
        return ecc_metric_evaluate_weighted(m, &values[k], coverages ? &coverages[k] : nullptr, nullptr);
    });
}
