// ecc_robust.hip -- ecc_metric_evaluate_robust[_pairs], ecc_host_robust_scale: the metric under a per-sample robust loss (host
// code; include/ecc_hip.h states the contract, robust_kernel.hip has the pair kernels, sum_kernel.hip the sums).  Line weights
// (ecc_weighted.hip) need a caller who knows where the bad lines are; a fluoroscopy tracker or an FD-CT motion correction often
// does not -- an instrument nobody flagged, a truncated view, a detector defect that appears mid-scan -- and the squared difference
// then lets a few percent of the samples decide the value.  Every loss here is rho(d) = w(d) d^2, so the kernel is the weighted
// kernel with its per-sample factor computed from the residual instead of gathered.
//
// The launches: E1 (if the device geometry is behind the matrices), k01_kernel over all pairs or the list into the Gram call's
// records (scratch of the Gram-family calls alone; column_call_begin, ecc_column_call.h), pairs_robust_kernel, sum_gram_kernel over
// the columns c and u, the copies (column_call_finish).  The metric's kept records, kept values and pose-batch values are not
// touched (the list form stages its tuples in the pose batch's index scratch, as ecc_metric_evaluate_weighted_pairs does).
// The pose-delta and transform forms are in ecc_robust_batches.hip; they take the checks, the launch parameters and the base's columns
// from robust_check, fill_robust_params and robust_base_columns below.
// The loss combined with line weights on a 2 n metric is ecc_weighted_robust.hip; it takes robust_check from here.
// Not here: range, group and RCCL forms; the loss under use_corr; Tukey's biweight (not d^2 near zero: no bit link to
// ecc_metric_evaluate_all).
#include "ecc_column_call.h"

using namespace ecc_internal;

static_assert(ECC_LOSS_HUBER == ECC_ROBUST_HUBER && ECC_LOSS_TRUNCATED == ECC_ROBUST_TRUNCATED &&
                  ECC_LOSS_GEMAN_MCCLURE == ECC_ROBUST_GEMAN_MCCLURE,
              "the kernels' loss codes are the header's");

namespace {
constexpr int T = 3;  // columns: c, u, r
}  // namespace

namespace ecc_internal {
// What every robust call needs of its arguments and of the metric (after the null check of m), before the device is touched.
int robust_check(const ecc_metric* m, const double* value, int loss, float delta)
{
    if (!value) return fail(ECC_ERR_INVALID_ARGUMENT, "value is null");
    if (loss < ECC_LOSS_HUBER || loss > ECC_LOSS_GEMAN_MCCLURE) return fail(ECC_ERR_INVALID_ARGUMENT, "loss is none of ECC_LOSS_*");
    if (!(delta > 0.f)) return fail(ECC_ERR_INVALID_ARGUMENT, "delta must be positive (+infinity allowed)");
    if (m->n_views < 1) return fail(ECC_ERR_INVALID_ARGUMENT, "projection matrices have not been set");
    if (m->n_views < 2) return fail(ECC_ERR_INVALID_ARGUMENT, "need at least two views (the reference divides 0/0 here)");
    if (m->use_corr) return fail(ECC_ERR_UNSUPPORTED, "the robust loss is not defined for the correlation cost");
    return ECC_OK;
}

// The launch's loss: three columns in `values`, col_stride apart; 1 / delta is formed here, on the host, in float64.
void fill_robust_params(EccRobustParams* g, float* values, int64_t col_stride, int loss, float delta)
{
    g->values = values;
    g->col_stride = col_stride;
    g->loss = loss;
    g->delta = delta;
    g->inv_delta = (float)(1.0 / (double)delta);
}

// {c, u, r} of all pairs at the current matrices: everything of ecc_metric_evaluate_robust up to and including its pair launch.
// The three columns are in m->gram_values_d, g->col_stride apart, once the stream gets there; c->p and *g are the launches as they
// were made (ecc_robust_batches.hip launches the grids of its poses with the same parameters).
int robust_base_columns(ecc_metric* m, int loss, float delta, ColumnCall* c, EccRobustParams* g)
{
    const int64_t n = m->n_views;
    const int rc = column_call_begin(m, nullptr, n * (n - 1) / 2, T, 2, c);  // the sampling mode of an all-pairs evaluation
    if (rc) return rc;
    fill_robust_params(g, m->gram_values_d.ptr, c->col_stride, loss, delta);
    HIP_TRY(launch_robust_timed(m->ctx, &c->p, g));
    return ECC_OK;
}
}  // namespace ecc_internal

namespace {

// Everything behind the checks: `count` pairs -- all pairs (idx4 null) or the list -- under the sampling mode of that many values.
int robust_run(ecc_metric* m, const int32_t* idx4, int64_t count, int loss, float delta, double* value, double* inlier_mass, float* pair_terms)
{
    ColumnCall c;
    int rc = column_call_begin(m, idx4, count, T, 2, &c);
    if (rc) return rc;
    EccRobustParams g;
    fill_robust_params(&g, m->gram_values_d.ptr, c.col_stride, loss, delta);
    HIP_TRY(launch_robust_timed(m->ctx, &c.p, &g));  // (robust_kernel.hip)
    double totals[2];  // c and u in the order an evaluation of `count` values is added in (ecc_sum_order.h); r is not summed
    rc = column_call_finish(m, c, 2, totals, T, m->gram_values_d.ptr, pair_terms);
    if (rc) return rc;
    // a mean over the pairs, ref: ...RadonIntermediate.cpp:224 with all weights 1 -- NOT divided by the inlier mass: that would reward
    // pushing samples into the tails
    *value = totals[0] / (double)count;
    if (inlier_mass) *inlier_mass = totals[1] / (double)count;
    return ECC_OK;
}

}  // namespace

ECC_EXPORT int ecc_metric_evaluate_robust(ecc_metric* m, int loss, float delta, double* value, double* inlier_mass, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    int rc = robust_check(m, value, loss, delta);
    if (rc) return rc;
    const int64_t n = m->n_views;
    if ((int64_t)m->dtrs.size() < n) return fail(ECC_ERR_INVALID_ARGUMENT, "fewer Radon intermediates than projection matrices");
    return robust_run(m, nullptr, n * (n - 1) / 2, loss, delta, value, inlier_mass, pair_terms);
}

ECC_EXPORT int ecc_metric_evaluate_robust_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, int loss, float delta, double* value,
                                                double* inlier_mass, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (n_pairs < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "negative list length");
    if (n_pairs > 0 && !idx4) return fail(ECC_ERR_INVALID_ARGUMENT, "index list is null");
    int rc = robust_check(m, value, loss, delta);
    if (rc) return rc;
    // range check as ecc_metric_evaluate_pairs: P index the current matrices, D the Radon intermediates
    const int nP = m->n_views, nD = (int)m->dtrs.size();
    for (int q = 0; q < n_pairs; ++q) {
        const int32_t* t = idx4 + 4 * (size_t)q;
        if (t[0] < 0 || t[0] >= nP || t[1] < 0 || t[1] >= nP || t[2] < 0 || t[2] >= nD || t[3] < 0 || t[3] >= nD)
            return fail(ECC_ERR_INVALID_ARGUMENT, "index array contains invalid indices");
    }
    if (n_pairs == 0) return ECC_OK;
    return robust_run(m, idx4, n_pairs, loss, delta, value, inlier_mass, pair_terms);
}

// k x the median of sqrt(r_q) over the rows {c, u, r} with r_q > 0 (even count: the mean of the two middle values); 0.0 with no such
// row.  Host only.
ECC_EXPORT double ecc_host_robust_scale(const float* pair_terms, int64_t n_pairs, double k)
{
    std::vector<double> rms;
    if (pair_terms)
        for (int64_t q = 0; q < n_pairs; ++q) {
            const float r = pair_terms[(size_t)q * T + 2];
            if (r > 0.f) rms.push_back(std::sqrt((double)r));
        }
    if (rms.empty()) return 0.0;
    std::sort(rms.begin(), rms.end());
    const size_t h = rms.size() / 2;
    return k * (rms.size() & 1 ? rms[h] : (rms[h - 1] + rms[h]) / 2.0);
}
