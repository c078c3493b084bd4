// ecc_weighted_robust.hip -- ecc_metric_evaluate_weighted_robust[_pairs], ecc_host_weighted_robust_scale: the metric with per-line
// weights AND a per-sample robust loss (host code; include/ecc_hip.h states the contract, weighted_robust_kernel.hip has the pair
// kernels, sum_kernel.hip the sums).  Real scans have both kinds of bad data at once: a fluoroscopy sequence has collimator blades,
// known and flagged once per view (ecc_radon_line_weights), and a catheter nobody flagged.  Weights alone leave the instrument in;
// the loss alone spends its scale on lines whose badness was known in advance and cannot be called on a 2 n metric's weights at all.
//
// The launches: E1 (if the device geometry is behind the matrices), k01_kernel over all pairs or the list into the Gram call's
// records (scratch of the Gram-family calls alone; column_call_begin, ecc_column_call.h), pairs_weighted_robust_kernel,
// sum_gram_kernel over the columns c, u and k, the copies (column_call_finish).  The metric's kept records, kept values and pose-batch
// values are not touched (the list form stages its tuples in the pose batch's index scratch, as ecc_metric_evaluate_weighted_pairs
// does).
// Not here: the pose-delta and transform batches of this form (the kernel serves them as it stands); range, group and RCCL forms;
// use_corr; Tukey's biweight; a variance form.
#include "ecc_column_call.h"

using namespace ecc_internal;

namespace {

constexpr int T = 4;  // columns: c, u, k, r
constexpr int S = 3;  // summed: c, u, k

// What both calls need of their arguments and of the metric (after the null check of m and the list's own checks), before the device
// is touched: robust_check's conditions, then weighted_check's, each with its code.  Behind it the metric holds exactly 2 n_views
// intermediates, which is what keeps the kernel's gathers at `origin + channel offset` inside the copies.
int weighted_robust_check(const ecc_metric* m, const double* value, int loss, float delta)
{
    const int rc = robust_check(m, value, loss, delta);
    return rc ? rc : weighted_check(m);
}

// Everything behind the checks: `count` pairs -- all pairs (idx4 null) or the list -- under the sampling mode of that many values.
int weighted_robust_run(ecc_metric* m, const int32_t* idx4, int64_t count, int loss, float delta, double* value, double* coverage,
                        double* inlier_mass, float* pair_terms)
{
    ColumnCall c;
    int rc = column_call_begin(m, idx4, count, T, S, &c);
    if (rc) return rc;
    EccWeightedRobustParams g;
    set_channel_strides(m, &g);  // the data channel and, one channel behind it, the weights
    g.values = m->gram_values_d.ptr;
    g.col_stride = c.col_stride;
    g.loss = loss;
    g.delta = delta;
    g.inv_delta = (float)(1.0 / (double)delta);  // formed here, on the host, in float64 (as fill_robust_params)
    HIP_TRY(launch_weighted_robust_timed(m->ctx, &c.p, &g));
    double totals[S];  // c, u and k in the order an evaluation of `count` values is added in (ecc_sum_order.h); r is not summed
    rc = column_call_finish(m, c, S, totals, T, m->gram_values_d.ptr, pair_terms);
    if (rc) return rc;
    // sum c / sum u as ecc_metric_evaluate_weighted divides, and for its reason (an optimiser must not gain by pushing lines into
    // masked regions) -- never by the mass the loss keeps, as ecc_metric_evaluate_robust refuses to, and for its reason (that would
    // reward pushing samples into the tails)
    const bool none = totals[1] == 0.0;
    *value = none ? 0.0 : totals[0] / totals[1];
    if (coverage) *coverage = none ? 0.0 : totals[1] / (double)count;
    if (inlier_mass) *inlier_mass = none ? 0.0 : totals[2] / totals[1];
    return ECC_OK;
}

}  // namespace

ECC_EXPORT int ecc_metric_evaluate_weighted_robust(ecc_metric* m, int loss, float delta, double* value, double* coverage,
                                                   double* inlier_mass, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    const int rc = weighted_robust_check(m, value, loss, delta);
    if (rc) return rc;
    const int64_t n = m->n_views;
    return weighted_robust_run(m, nullptr, n * (n - 1) / 2, loss, delta, value, coverage, inlier_mass, pair_terms);
}

ECC_EXPORT int ecc_metric_evaluate_weighted_robust_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, int loss, float delta,
                                                         double* value, double* coverage, double* inlier_mass, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (n_pairs < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "negative list length");
    if (n_pairs > 0 && !idx4) return fail(ECC_ERR_INVALID_ARGUMENT, "index list is null");
    const int rc = weighted_robust_check(m, value, loss, delta);
    if (rc) return rc;
    // P index the current matrices, D the DATA intermediates: the weights of a sample come from dtr n_views + D
    const int nP = m->n_views;
    for (int q = 0; q < n_pairs; ++q) {
        const int32_t* t = idx4 + 4 * (size_t)q;
        if (t[0] < 0 || t[0] >= nP || t[1] < 0 || t[1] >= nP || t[2] < 0 || t[2] >= nP || t[3] < 0 || t[3] >= nP)
            return fail(ECC_ERR_INVALID_ARGUMENT, "index array contains invalid indices (matrices and data intermediates lie in [0, n_views))");
    }
    if (n_pairs == 0) return ECC_OK;
    return weighted_robust_run(m, idx4, n_pairs, loss, delta, value, coverage, inlier_mass, pair_terms);
}

// k x the median of sqrt(r_q / u_q) over the rows {c, u, k, r} with r_q > 0 and u_q > 0 (even count: the mean of the two middle
// values); 0.0 with no such row.  Host only.  u_q == 1.0f: the division leaves r_q as it is, ecc_host_robust_scale's figure.
ECC_EXPORT double ecc_host_weighted_robust_scale(const float* pair_terms, int64_t n_pairs, double k)
{
    std::vector<double> rms;
    if (pair_terms)
        for (int64_t q = 0; q < n_pairs; ++q) {
            const float u = pair_terms[(size_t)q * T + 1], r = pair_terms[(size_t)q * T + 3];
            if (r > 0.f && u > 0.f) rms.push_back(std::sqrt((double)r / (double)u));
        }
    if (rms.empty()) return 0.0;
    std::sort(rms.begin(), rms.end());
    const size_t h = rms.size() / 2;
    return k * (rms.size() & 1 ? rms[h] : (rms[h - 1] + rms[h]) / 2.0);
}
