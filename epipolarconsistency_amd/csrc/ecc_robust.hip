// ecc_robust.hip -- ecc_metric_evaluate_robust[_pairs], ecc_host_robust_scale: the metric under a per-sample robust loss (host
// code; include/ecc_hip.h states the contract, robust_kernel.hip has the pair kernels, sum_kernel.hip the sums).  Line weights
// (ecc_weighted.hip) need a caller who knows where the bad lines are; a fluoroscopy tracker or an FD-CT motion correction often
// does not -- an instrument nobody flagged, a truncated view, a detector defect that appears mid-scan -- and the squared difference
// then lets a few percent of the samples decide the value.  Every loss here is rho(d) = w(d) d^2, so the kernel is the weighted
// kernel with its per-sample factor computed from the residual instead of gathered.
//
// The launch sequence is form_call's (ecc_form_call.h); what is the robust form's own -- its columns, its pair launch with the loss,
// its division -- is robust_form below.  The pose-delta and transform forms are in ecc_robust_batches.hip; they take robust_check
// and robust_form from here.  The loss combined with line weights on a 2 n metric is ecc_weighted_robust.hip; it takes robust_check.
// Not here: range, group and RCCL forms; the loss under use_corr; Tukey's biweight (not d^2 near zero: no bit link to
// ecc_metric_evaluate_all).
#include "ecc_form_call.h"

using namespace ecc_internal;

static_assert(ECC_LOSS_HUBER == ECC_ROBUST_HUBER && ECC_LOSS_TRUNCATED == ECC_ROBUST_TRUNCATED &&
                  ECC_LOSS_GEMAN_MCCLURE == ECC_ROBUST_GEMAN_MCCLURE,
              "the kernels' loss codes are the header's");

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

PairForm robust_form(int loss, float delta, double* values, double* inlier_masses)
{
    return {3, 2,  // columns: c, u, r; r is not summed
            [=](ecc_metric* m, const EccPairParams& p, float* cols, int64_t col_stride) {
                EccRobustParams g;
                g.values = cols;
                g.col_stride = col_stride;
                g.loss = loss;
                g.delta = delta;
                g.inv_delta = (float)(1.0 / (double)delta);  // formed here, on the host, in float64
                return launch_timed(m->ctx, [&](hipStream_t s) { return ecc_launch_pairs_robust(&p, &g, s); });  // (robust_kernel.hip)
            },
            [=](const double* totals, int64_t count, int64_t k) {
                // a mean over the pairs, ref: ...RadonIntermediate.cpp:224 with all weights 1 -- NOT divided by the inlier mass: that
                // would reward pushing samples into the tails
                values[k] = totals[0] / (double)count;
                if (inlier_masses) inlier_masses[k] = totals[1] / (double)count;
            },
            ecc_form_base::ROBUST, loss, delta, 0.f};
}
}  // namespace ecc_internal

ECC_EXPORT int ecc_metric_evaluate_robust(ecc_metric* m, int loss, float delta, double* value, double* inlier_mass, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    int rc = robust_check(m, value, loss, delta);
    if (rc) return rc;
    if ((int64_t)m->dtrs.size() < (int64_t)m->n_views) return fail(ECC_ERR_INVALID_ARGUMENT, "fewer Radon intermediates than projection matrices");
    return form_call_all_pairs(m, robust_form(loss, delta, value, inlier_mass), pair_terms);
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
    rc = check_index_list(idx4, n_pairs, m->n_views, (int)m->dtrs.size(), "index array contains invalid indices");
    if (rc) return rc;
    if (n_pairs == 0) return ECC_OK;
    return form_call(m, robust_form(loss, delta, value, inlier_mass), idx4, n_pairs, pair_terms);
}

// k x the median of sqrt(r_q) over the rows {c, u, r} with r_q > 0 (even count: the mean of the two middle values); 0.0 with no such
// row.  Host only.
ECC_EXPORT double ecc_host_robust_scale(const float* pair_terms, int64_t n_pairs, double k)
{
    std::vector<double> rms;
    if (pair_terms)
        for (int64_t q = 0; q < n_pairs; ++q) {
            const float r = pair_terms[(size_t)q * 3 + 2];
            if (r > 0.f) rms.push_back(std::sqrt((double)r));
        }
    return scaled_median(rms, k);
}
