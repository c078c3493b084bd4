// ecc_variance_robust.hip -- ecc_metric_evaluate_variance_robust and its index-list, pose-delta and transform forms,
// ecc_host_variance_robust_scale: the metric with inverse-variance sample weights AND a robust loss of the studentised residual (host
// code; include/ecc_hip.h states the contract, variance_robust_kernel.hip has the pair kernels, sum_kernel.hip and
// form_sums_kernel.hip the sums).  A low-dose fluoroscopy sequence has photon-starved lines whose variance is known, and a catheter
// nobody flagged.  ecc_metric_evaluate_robust thresholds the raw residual, so a line that is merely noisy, and known to be, is
// rejected as an outlier; ecc_metric_evaluate_variance keeps the catheter at full weight.  Here the loss sees z = d / sigma with
// sigma^2 = V_i + V_j, and delta counts sigmas.
//
// The launch sequences are ecc_form_call.h's: form_call (all pairs, an index list), form_pose_deltas, form_transforms.  What is this
// form's own -- its columns, its pair launch with loss, delta and floor, its three results -- is variance_robust_form below.  T = 4,
// S = 3: the batches' sums are sum_form_poses_kernel and sum_form_transforms_kernel as they stand.
// Every result of a batch has the bits of ecc_metric_set_projections + the sequential call for that pose or transform
// (tests/test_gpu_variance_robust_batches.py); what a batch does not take is evaluated that way inside the call.
// Not here: base columns kept between calls; range, group and RCCL forms; use_corr; the maps of this form; a covariance-aware model
// for derivative data.
#include "ecc_form_call.h"
#include "ecc_variance_robust_host.h"

using namespace ecc_internal;

namespace ecc_internal {

// What every call needs of its arguments and of the metric (after the null check of m and the list's own checks), before the device
// is touched: the robust calls' conditions on value, loss and delta, then variance_check's in its order -- the metric's shape and
// the floor before use_corr.
int variance_robust_check(const ecc_metric* m, const double* value, int loss, float delta, float floor)
{
    if (!value) return fail(ECC_ERR_INVALID_ARGUMENT, "value is null");
    if (loss < ECC_LOSS_HUBER || loss > ECC_LOSS_GEMAN_MCCLURE) return fail(ECC_ERR_INVALID_ARGUMENT, "loss is none of ECC_LOSS_*");
    if (!(delta > 0.f)) return fail(ECC_ERR_INVALID_ARGUMENT, "delta must be positive (+infinity allowed)");
    return variance_check(m, floor);
}

PairForm variance_robust_form(int loss, float delta, float floor, double* values, double* mean_weights, double* inlier_masses)
{
    return {4, 3,  // columns: c, u, k, r; r is not summed
            [=](ecc_metric* m, const EccPairParams& p, float* cols, int64_t col_stride) {
                EccVarianceRobustParams g;
                set_channel_strides(m, &g);  // the data channel and, one channel behind it, the variance fields
                g.values = cols;
                g.col_stride = col_stride;
                g.floor = floor;
                g.loss = loss;
                g.delta = delta;
                g.inv_delta = (float)(1.0 / (double)delta);  // formed here, on the host, in float64 (as robust_form)
                return launch_timed(m->ctx, [&](hipStream_t s) { return ecc_launch_pairs_variance_robust(&p, &g, s); });
            },
            [=](const double* totals, int64_t count, int64_t k) {
                // sum c / sum u as ecc_metric_evaluate_variance divides -- never by the mass the loss keeps: that would reward
                // pushing samples into the tails
                const bool none = totals[1] == 0.0;
                values[k] = none ? 0.0 : totals[0] / totals[1];
                if (mean_weights) mean_weights[k] = none ? 0.0 : totals[1] / (double)count;
                if (inlier_masses) inlier_masses[k] = none ? 0.0 : totals[2] / totals[1];
            },
            ecc_form_base::VARIANCE_ROBUST, loss, delta, floor};
}

}  // namespace ecc_internal

ECC_EXPORT int ecc_metric_evaluate_variance_robust(ecc_metric* m, int loss, float delta, float floor, double* value, double* mean_weight,
                                                   double* inlier_mass, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    const int rc = variance_robust_check(m, value, loss, delta, floor);
    if (rc) return rc;
    return form_call_all_pairs(m, variance_robust_form(loss, delta, floor, value, mean_weight, inlier_mass), pair_terms);
}

ECC_EXPORT int ecc_metric_evaluate_variance_robust_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, int loss, float delta, float floor,
                                                         double* value, double* mean_weight, double* inlier_mass, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (n_pairs < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "negative list length");
    if (n_pairs > 0 && !idx4) return fail(ECC_ERR_INVALID_ARGUMENT, "index list is null");
    int rc = variance_robust_check(m, value, loss, delta, floor);
    if (rc) return rc;
    // P index the current matrices, D the DATA intermediates: the variance of a sample comes from dtr n_views + D
    rc = check_index_list(idx4, n_pairs, m->n_views, m->n_views,
                          "index array contains invalid indices (matrices and data intermediates lie in [0, n_views))");
    if (rc) return rc;
    if (n_pairs == 0) return ECC_OK;
    return form_call(m, variance_robust_form(loss, delta, floor, value, mean_weight, inlier_mass), idx4, n_pairs, pair_terms);
}

ECC_EXPORT int ecc_metric_evaluate_variance_robust_pose_deltas(ecc_metric* m, int n_poses, const int32_t* moved_offsets, const int32_t* moved_views,
                                                               const double* moved_Ps, int loss, float delta, float floor, double* values,
                                                               double* mean_weights, double* inlier_masses)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!moved_offsets || !values) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    if (n_poses < 1) return ECC_OK;
    if (moved_offsets[n_poses] > 0 && (!moved_views || !moved_Ps)) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    int rc = variance_robust_check(m, values, loss, delta, floor);
    if (rc) return rc;
    rc = check_lists(m, n_poses, moved_offsets, moved_views);
    if (rc) return rc;
    return form_pose_deltas(m, variance_robust_form(loss, delta, floor, values, mean_weights, inlier_masses), n_poses, moved_offsets, moved_views,
                            moved_Ps, [&](int k) {
                                return ecc_metric_evaluate_variance_robust(m, loss, delta, floor, &values[k], mean_weights ? &mean_weights[k] : nullptr,
                                                                           inlier_masses ? &inlier_masses[k] : nullptr, nullptr);
                            });
}

ECC_EXPORT int ecc_metric_evaluate_variance_robust_transforms(ecc_metric* m, int n_source, int n_transforms, const double* Ts, int loss, float delta,
                                                              float floor, double* values, double* mean_weights, double* inlier_masses,
                                                              float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (n_transforms < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "n_transforms must not be negative");
    if (n_transforms > 0 && (!Ts || !values)) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    double unused = 0.0;  // (n_transforms == 0: values may be null, and nothing is written)
    const int rc = variance_robust_check(m, values ? values : &unused, loss, delta, floor);
    if (rc) return rc;
    if (n_source < 1 || n_source >= m->n_views)
        return fail(ECC_ERR_INVALID_ARGUMENT, "n_source must be in [1, n_views): the views [0, n_source) are the source, the rest the target");
    return form_transforms(m, variance_robust_form(loss, delta, floor, values, mean_weights, inlier_masses), n_source, n_transforms, Ts, pair_terms,
                           "transform", [&](int k, const int32_t* idx, int len, float* rows) {
                               return ecc_metric_evaluate_variance_robust_pairs(m, idx, len, loss, delta, floor, &values[k],
                                                                                mean_weights ? &mean_weights[k] : nullptr,
                                                                                inlier_masses ? &inlier_masses[k] : nullptr, rows);
                           });
}

// Host only, no device (ecc_variance_robust_host.h).
ECC_EXPORT double ecc_host_variance_robust_scale(const float* pair_terms, int64_t n_pairs, double k)
{
    return ecc_variance_robust_host::variance_robust_scale(pair_terms, n_pairs, k);
}
