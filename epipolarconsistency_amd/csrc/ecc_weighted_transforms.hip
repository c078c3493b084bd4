// ecc_weighted_transforms.hip -- the metric with per-line weights (ecc_weighted.hip, weighted_kernel.hip) for the registration of two
// scans (ecc_transforms.hip; ref: tools/Registration/Registration3D3D.hxx:56-62, :91-110).  Host code; include/ecc_hip.h states the
// contract.  A truncated second scan, a table edge that one scan sees, an instrument present in one acquisition break exactly the
// lines that cross them, in every cross pair of that view; the caller flags those lines in the view's weight intermediate.
//
// ecc_metric_evaluate_weighted_transforms is form_transforms with the weighted form (ecc_form_call.h): values[k] = sum c / sum u,
// coverages[k] = sum u / count.  The grid's DATA indices stay i and n_source + j, so the weights of a sample come from dtr
// n_views + D whatever the extended matrix index is.
// Every value, coverage and pair term has the bits of ecc_metric_set_projections(composed matrices) +
// ecc_metric_evaluate_weighted_pairs(the cross list) (tests/test_gpu_weighted_transforms.py).  What the batch does not take is
// evaluated that way inside the call.  Nothing of the metric's own state is written; the scratch is the pose batch's.
// Not here: the full-matrices and strided pose forms of the weighted metric; kept base columns; range, group and RCCL forms.
#include "ecc_form_call.h"

using namespace ecc_internal;

ECC_EXPORT int ecc_metric_evaluate_weighted_transforms(ecc_metric* m, int n_source, int n_transforms, const double* Ts, double* values,
                                                       double* coverages, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (n_transforms < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "n_transforms must not be negative");
    if (n_transforms > 0 && (!Ts || !values)) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    int rc = weighted_check(m);
    if (rc) return rc;
    if (n_source < 1 || n_source >= m->n_views)
        return fail(ECC_ERR_INVALID_ARGUMENT, "n_source must be in [1, n_views): the views [0, n_source) are the source, the rest the target");
    // ("pose": the word this call's batches have always waited under)
    return form_transforms(m, weighted_form(values, coverages), n_source, n_transforms, Ts, pair_terms, "pose",
                           [&](int k, const int32_t* idx, int len, float* rows) {
                               return ecc_metric_evaluate_weighted_pairs(m, idx, len, &values[k], coverages ? &coverages[k] : nullptr, rows);
                           });
}
