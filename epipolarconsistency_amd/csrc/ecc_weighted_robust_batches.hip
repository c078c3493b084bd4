// ecc_weighted_robust_batches.hip -- the metric under line weights AND a per-sample robust loss (ecc_weighted_robust.hip,
// weighted_robust_kernel.hip) for the callers that sit in optimiser loops: a population of poses or of source-to-target transforms per
// call.  Host code only; include/ecc_hip.h states the contracts, DESIGN.md 4.26 the launch sequence.  The pair launch is
// ecc_launch_pairs_weighted_robust as it stands, the grids are ecc_poses.hip's and ecc_transforms.hip's; the segmented sums are
// form_sums_kernel.hip's, which take the form's three summed columns {c, u, k} in one walk (ecc_form_call.h picks them by the form's S).
//
// ecc_metric_evaluate_weighted_robust_pose_deltas  form_pose_deltas with the weighted-robust form (ecc_form_call.h): values[k] =
//                                                  sum c / sum u, coverages[k] = sum u / n_pairs, inlier_masses[k] = sum k / sum u
// ecc_metric_evaluate_weighted_robust_transforms   form_transforms with it, count in place of n_pairs
// Every result has the bits of the sequential calls (tests/test_gpu_weighted_robust_poses.py,
// tests/test_gpu_weighted_robust_transforms.py); what a batch does not take is evaluated that way inside the call.
// Not here: base columns kept between calls; the full-matrices and strided pose forms; range, group and RCCL forms; use_corr; the
// batches of the maps.
#include "ecc_form_call.h"

using namespace ecc_internal;

ECC_EXPORT int ecc_metric_evaluate_weighted_robust_pose_deltas(ecc_metric* m, int n_poses, const int32_t* moved_offsets, const int32_t* moved_views,
                                                               const double* moved_Ps, int loss, float delta, double* values, double* coverages,
                                                               double* inlier_masses)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!moved_offsets || !values) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    if (n_poses < 1) return ECC_OK;
    if (moved_offsets[n_poses] > 0 && (!moved_views || !moved_Ps)) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    int rc = weighted_robust_check(m, values, loss, delta);
    if (rc) return rc;
    rc = check_lists(m, n_poses, moved_offsets, moved_views);
    if (rc) return rc;
    return form_pose_deltas(m, weighted_robust_form(loss, delta, values, coverages, inlier_masses), n_poses, moved_offsets, moved_views, moved_Ps,
                            [&](int k) {
                                return ecc_metric_evaluate_weighted_robust(m, loss, delta, &values[k], coverages ? &coverages[k] : nullptr,
                                                                           inlier_masses ? &inlier_masses[k] : nullptr, nullptr);
                            });
}

ECC_EXPORT int ecc_metric_evaluate_weighted_robust_transforms(ecc_metric* m, int n_source, int n_transforms, const double* Ts, int loss, float delta,
                                                              double* values, double* coverages, double* inlier_masses, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (n_transforms < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "n_transforms must not be negative");
    if (n_transforms > 0 && (!Ts || !values)) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    double unused = 0.0;  // (n_transforms == 0: values may be null, and nothing is written)
    const int rc = weighted_robust_check(m, values ? values : &unused, loss, delta);
    if (rc) return rc;
    if (n_source < 1 || n_source >= m->n_views)
        return fail(ECC_ERR_INVALID_ARGUMENT, "n_source must be in [1, n_views): the views [0, n_source) are the source, the rest the target");
    return form_transforms(m, weighted_robust_form(loss, delta, values, coverages, inlier_masses), n_source, n_transforms, Ts, pair_terms, "transform",
                           [&](int k, const int32_t* idx, int len, float* rows) {
                               return ecc_metric_evaluate_weighted_robust_pairs(m, idx, len, loss, delta, &values[k],
                                                                                coverages ? &coverages[k] : nullptr,
                                                                                inlier_masses ? &inlier_masses[k] : nullptr, rows);
                           });
}
