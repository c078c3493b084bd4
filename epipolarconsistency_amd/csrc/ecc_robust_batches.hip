// ecc_robust_batches.hip -- the metric under a per-sample robust loss (ecc_robust.hip, robust_kernel.hip) for the callers that sit
// in optimiser loops: a population of poses or of source-to-target transforms per call.  Host code only; include/ecc_hip.h states the
// contracts, DESIGN.md 4.22 the launch sequence.  Nothing here is a kernel of its own: the pair launch is ecc_launch_pairs_robust as
// it stands, the segmented sums are those of the weighted siblings (they read columns 0 and 1 of a column-form buffer and know
// nothing of line weights), the grids are ecc_poses.hip's and ecc_transforms.hip's.
//
// ecc_metric_evaluate_robust_pose_deltas  form_pose_deltas with the robust form (ecc_form_call.h): values[k] = sum c / n_pairs,
//                                         inlier_masses[k] = sum u / n_pairs
// ecc_metric_evaluate_robust_transforms   form_transforms with it: values[k] = sum c / count, inlier_masses[k] = sum u / count
// Every result has the bits of the sequential calls (tests/test_gpu_robust_poses.py, tests/test_gpu_robust_transforms.py); what a
// batch does not take is evaluated that way inside the call.
// Not here: base columns kept between calls; the full-matrices and strided pose forms; range, group and RCCL forms; the loss under
// use_corr.  (These batches for the loss combined with line weights: ecc_weighted_robust_batches.hip.)
#include "ecc_form_call.h"

using namespace ecc_internal;

ECC_EXPORT int ecc_metric_evaluate_robust_pose_deltas(ecc_metric* m, int n_poses, const int32_t* moved_offsets, const int32_t* moved_views,
                                                      const double* moved_Ps, int loss, float delta, double* values, double* inlier_masses)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!moved_offsets || !values) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    if (n_poses < 1) return ECC_OK;
    if (moved_offsets[n_poses] > 0 && (!moved_views || !moved_Ps)) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    int rc = robust_check(m, values, loss, delta);
    if (rc) return rc;
    if ((int64_t)m->dtrs.size() < (int64_t)m->n_views) return fail(ECC_ERR_INVALID_ARGUMENT, "fewer Radon intermediates than projection matrices");
    rc = check_lists(m, n_poses, moved_offsets, moved_views);
    if (rc) return rc;
    return form_pose_deltas(m, robust_form(loss, delta, values, inlier_masses), n_poses, moved_offsets, moved_views, moved_Ps, [&](int k) {
        return ecc_metric_evaluate_robust(m, loss, delta, &values[k], inlier_masses ? &inlier_masses[k] : nullptr, nullptr);
    });
}

ECC_EXPORT int ecc_metric_evaluate_robust_transforms(ecc_metric* m, int n_source, int n_transforms, const double* Ts, int loss, float delta,
                                                     double* values, double* inlier_masses, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (n_transforms < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "n_transforms must not be negative");
    if (n_transforms > 0 && (!Ts || !values)) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    double unused = 0.0;  // (n_transforms == 0: values may be null, and nothing is written)
    int rc = robust_check(m, values ? values : &unused, loss, delta);
    if (rc) return rc;
    if ((int64_t)m->dtrs.size() < (int64_t)m->n_views) return fail(ECC_ERR_INVALID_ARGUMENT, "fewer Radon intermediates than projection matrices");
    if (n_source < 1 || n_source >= m->n_views)
        return fail(ECC_ERR_INVALID_ARGUMENT, "n_source must be in [1, n_views): the views [0, n_source) are the source, the rest the target");
    return form_transforms(m, robust_form(loss, delta, values, inlier_masses), n_source, n_transforms, Ts, pair_terms, "transform",
                           [&](int k, const int32_t* idx, int len, float* rows) {
                               return ecc_metric_evaluate_robust_pairs(m, idx, len, loss, delta, &values[k],
                                                                       inlier_masses ? &inlier_masses[k] : nullptr, rows);
                           });
}
