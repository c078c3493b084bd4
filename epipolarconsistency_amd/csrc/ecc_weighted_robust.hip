// ecc_weighted_robust.hip -- ecc_metric_evaluate_weighted_robust[_pairs], ecc_host_weighted_robust_scale: the metric with per-line
// weights AND a per-sample robust loss (host code; include/ecc_hip.h states the contract, weighted_robust_kernel.hip has the pair
// kernels, sum_kernel.hip the sums).  Real scans have both kinds of bad data at once: a fluoroscopy sequence has collimator blades,
// known and flagged once per view (ecc_radon_line_weights), and a catheter nobody flagged.  Weights alone leave the instrument in;
// the loss alone spends its scale on lines whose badness was known in advance and cannot be called on a 2 n metric's weights at all.
//
// The launch sequence is form_call's (ecc_form_call.h); what is this form's own -- its columns, its pair launch, its three results
// -- is weighted_robust_form below; the map under line weights (ecc_weighted_robust_map.hip) takes it and weighted_robust_check
// from here.
// The pose-delta and transform batches of this form are ecc_weighted_robust_batches.hip's.
// Not here: range, group and RCCL forms; use_corr; Tukey's biweight; a variance form.
#include "ecc_form_call.h"

using namespace ecc_internal;

namespace ecc_internal {

// What both calls need of their arguments and of the metric (after the null check of m and the list's own checks), before the device
// is touched: robust_check's conditions, then weighted_check's, each with its code.  Behind it the metric holds exactly 2 n_views
// intermediates, which is what keeps the kernel's gathers at `origin + channel offset` inside the copies.
int weighted_robust_check(const ecc_metric* m, const double* value, int loss, float delta)
{
    const int rc = robust_check(m, value, loss, delta);
    return rc ? rc : weighted_check(m);
}

PairForm weighted_robust_form(int loss, float delta, double* value, double* coverage, double* inlier_mass)
{
    return {4, 3,  // columns: c, u, k, r; r is not summed
            [=](ecc_metric* m, const EccPairParams& p, float* cols, int64_t col_stride) {
                EccWeightedRobustParams g;
                set_channel_strides(m, &g);  // the data channel and, one channel behind it, the weights
                g.values = cols;
                g.col_stride = col_stride;
                g.loss = loss;
                g.delta = delta;
                g.inv_delta = (float)(1.0 / (double)delta);  // formed here, on the host, in float64 (as robust_form)
                return launch_timed(m->ctx, [&](hipStream_t s) { return ecc_launch_pairs_weighted_robust(&p, &g, s); });
            },
            [=](const double* totals, int64_t count, int64_t k) {
                // sum c / sum u as ecc_metric_evaluate_weighted divides, and for its reason (an optimiser must not gain by pushing
                // lines into masked regions) -- never by the mass the loss keeps, as ecc_metric_evaluate_robust refuses to, and for
                // its reason (that would reward pushing samples into the tails)
                const bool none = totals[1] == 0.0;
                value[k] = none ? 0.0 : totals[0] / totals[1];
                if (coverage) coverage[k] = none ? 0.0 : totals[1] / (double)count;
                if (inlier_mass) inlier_mass[k] = none ? 0.0 : totals[2] / totals[1];
            },
            ecc_form_base::WEIGHTED_ROBUST, loss, delta, 0.f};
}

}  // namespace ecc_internal

ECC_EXPORT int ecc_metric_evaluate_weighted_robust(ecc_metric* m, int loss, float delta, double* value, double* coverage,
                                                   double* inlier_mass, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    const int rc = weighted_robust_check(m, value, loss, delta);
    if (rc) return rc;
    return form_call_all_pairs(m, weighted_robust_form(loss, delta, value, coverage, inlier_mass), pair_terms);
}

ECC_EXPORT int ecc_metric_evaluate_weighted_robust_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, int loss, float delta,
                                                         double* value, double* coverage, double* inlier_mass, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (n_pairs < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "negative list length");
    if (n_pairs > 0 && !idx4) return fail(ECC_ERR_INVALID_ARGUMENT, "index list is null");
    int rc = weighted_robust_check(m, value, loss, delta);
    if (rc) return rc;
    // P index the current matrices, D the DATA intermediates: the weights of a sample come from dtr n_views + D
    rc = check_index_list(idx4, n_pairs, m->n_views, m->n_views,
                          "index array contains invalid indices (matrices and data intermediates lie in [0, n_views))");
    if (rc) return rc;
    if (n_pairs == 0) return ECC_OK;
    return form_call(m, weighted_robust_form(loss, delta, value, coverage, inlier_mass), idx4, n_pairs, pair_terms);
}

// k x the median of sqrt(r_q / u_q) over the rows {c, u, k, r} with r_q > 0 and u_q > 0 (even count: the mean of the two middle
// values); 0.0 with no such row.  Host only.  u_q == 1.0f: the division leaves r_q as it is, ecc_host_robust_scale's figure.
ECC_EXPORT double ecc_host_weighted_robust_scale(const float* pair_terms, int64_t n_pairs, double k)
{
    std::vector<double> rms;
    if (pair_terms)
        for (int64_t q = 0; q < n_pairs; ++q) {
            const float u = pair_terms[(size_t)q * 4 + 1], r = pair_terms[(size_t)q * 4 + 3];
            if (r > 0.f && u > 0.f) rms.push_back(std::sqrt((double)r / (double)u));
        }
    return scaled_median(rms, k);
}
