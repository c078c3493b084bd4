// ecc_weighted.hip -- ecc_metric_evaluate_weighted: the metric with per-line weights in Radon space (host code; include/ecc_hip.h
// states the contract, weighted_kernel.hip has the pair kernels, sum_kernel.hip the sums).  The caller has data in which SOME lines
// of SOME views cannot be trusted -- an instrument in one view of a fluoroscopy sequence, a collimator blade, a defective detector
// column, a table edge present in some views only -- and gives every view a second Radon intermediate that says how much each line
// counts.  The reference has the weight slot and wires it to 1.0f (ref: EpipolarConsistencyRadonIntermediate.cu:254); its host
// epilogue already returns sum value w / sum w (ref: ...RadonIntermediate.cpp:197-224).
//
// The launch sequence is form_call's (ecc_form_call.h); what is the weighted form's own -- its columns, its pair launch, its
// division -- is weighted_form below, which the index-list and pose-delta forms (ecc_weighted_poses.hip) and the transform form
// (ecc_weighted_transforms.hip) build their calls from as well.
// Not here: base columns kept between calls; full-matrices, strided, group and RCCL forms; an incremental mode.
#include "ecc_form_call.h"

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

PairForm weighted_form(double* values, double* coverages)
{
    return {2, 2,  // columns: c, u; both summed
            [](ecc_metric* m, const EccPairParams& p, float* cols, int64_t col_stride) {
                EccWeightedParams g;
                set_channel_strides(m, &g);
                g.values = cols;
                g.col_stride = col_stride;
                return launch_timed(m->ctx, [&](hipStream_t s) { return ecc_launch_pairs_weighted(&p, &g, s); });  // (weighted_kernel.hip)
            },
            [=](const double* totals, int64_t count, int64_t k) {
                // ref: ...RadonIntermediate.cpp:224 (sum value w / sum w); all weights 1: sum_u == count, the division of an unweighted evaluation
                const bool none = totals[1] == 0.0;
                values[k] = none ? 0.0 : totals[0] / totals[1];
                if (coverages) coverages[k] = none ? 0.0 : totals[1] / (double)count;
            },
            ecc_form_base::WEIGHTED, 0, 0.f, 0.f};
}
}  // namespace ecc_internal

ECC_EXPORT int ecc_metric_evaluate_weighted(ecc_metric* m, double* value, double* coverage, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!value) return fail(ECC_ERR_INVALID_ARGUMENT, "value is null");
    int rc = weighted_check(m);
    if (rc) return rc;
    return form_call_all_pairs(m, weighted_form(value, coverage), pair_terms);
}
