// ecc_weighted.hip -- ecc_metric_evaluate_weighted: the metric with per-line weights in Radon space (host code; include/ecc_hip.h
// states the contract, weighted_kernel.hip has the pair kernels, sum_kernel.hip the sums).  The caller has data in which SOME lines
// of SOME views cannot be trusted -- an instrument in one view of a fluoroscopy sequence, a collimator blade, a defective detector
// column, a table edge present in some views only -- and gives every view a second Radon intermediate that says how much each line
// counts.  The reference has the weight slot and wires it to 1.0f (ref: EpipolarConsistencyRadonIntermediate.cu:254); its host
// epilogue already returns sum value w / sum w (ref: ...RadonIntermediate.cpp:197-224).
//
// The launches: E1 (if the device geometry is behind the matrices), k01_kernel over all pairs into the Gram call's records (scratch
// of the Gram-family calls alone; column_call_begin, ecc_column_call.h), pairs_weighted_kernel, sum_gram_kernel over the two
// columns, the copies (column_call_finish).  The metric's kept records, kept values and pose-batch scratch are not touched.
// The index-list and pose-delta forms are in ecc_weighted_poses.hip; they take the base's columns from weighted_base_columns below.
// The transform form is in ecc_weighted_transforms.hip.
// Not here: base columns kept between calls; full-matrices, strided, group and RCCL forms; an incremental mode.
#include "ecc_column_call.h"

using namespace ecc_internal;

namespace ecc_internal {
// What every weighted call needs of the metric (after its own null checks), before the device is touched.
int weighted_check(const ecc_metric* m)
{
    if (m->n_views < 1) return fail(ECC_ERR_INVALID_ARGUMENT, "projection matrices have not been set");
    if (m->n_views < 2) return fail(ECC_ERR_INVALID_ARGUMENT, "need at least two views (the reference divides 0/0 here)");
    if ((int64_t)m->dtrs.size() != (int64_t)2 * m->n_views)
        return fail(ECC_ERR_INVALID_ARGUMENT, "the metric must hold 2 * n_views Radon intermediates: the data of every view, then its line weights");
    if (m->use_corr) return fail(ECC_ERR_UNSUPPORTED, "line weights are not defined for the correlation cost");
    return ECC_OK;
}

// {c, u} of all pairs at the current matrices: everything of ecc_metric_evaluate_weighted up to and including its pair launch.
// The two columns are in m->gram_values_d, g->col_stride apart, once the stream gets there; c->p and *g are the launches as they
// were made (ecc_weighted_poses.hip launches the grids of its poses with the same parameters).
int weighted_base_columns(ecc_metric* m, ColumnCall* c, EccWeightedParams* g)
{
    const int64_t n = m->n_views;
    const int rc = column_call_begin(m, nullptr, n * (n - 1) / 2, 2, 2, c);  // columns: c, u; the sampling mode of an all-pairs evaluation
    if (rc) return rc;
    set_channel_strides(m, g);
    g->values = m->gram_values_d.ptr;
    g->col_stride = c->col_stride;
    HIP_TRY(launch_weighted_timed(m->ctx, &c->p, g));
    return ECC_OK;
}

void finish_weighted(double sum_c, double sum_u, int64_t count, double* value, double* coverage)
{
    // ref: ...RadonIntermediate.cpp:224 (sum value w / sum w); all weights 1: sum_u == count, the division of an unweighted evaluation
    const bool none = sum_u == 0.0;
    *value = none ? 0.0 : sum_c / sum_u;
    if (coverage) *coverage = none ? 0.0 : sum_u / (double)count;
}
}  // namespace ecc_internal

ECC_EXPORT int ecc_metric_evaluate_weighted(ecc_metric* m, double* value, double* coverage, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!value) return fail(ECC_ERR_INVALID_ARGUMENT, "value is null");
    int rc = weighted_check(m);
    if (rc) return rc;
    ColumnCall c;
    EccWeightedParams g;
    rc = weighted_base_columns(m, &c, &g);
    if (rc) return rc;
    double totals[2];  // both columns in the order an all-pairs evaluation of n_pairs values is added in (ecc_sum_order.h)
    rc = column_call_finish(m, c, 2, totals, 2, m->gram_values_d.ptr, pair_terms);
    if (rc) return rc;
    finish_weighted(totals[0], totals[1], c.count, value, coverage);
    return ECC_OK;
}
