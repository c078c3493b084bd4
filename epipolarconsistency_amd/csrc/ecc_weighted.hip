// ecc_weighted.hip -- ecc_metric_evaluate_weighted: the metric with per-line weights in Radon space (host code; include/ecc_hip.h
// states the contract, weighted_kernel.hip has the pair kernels, sum_kernel.hip the sums).  The caller has data in which SOME lines
// of SOME views cannot be trusted -- an instrument in one view of a fluoroscopy sequence, a collimator blade, a defective detector
// column, a table edge present in some views only -- and gives every view a second Radon intermediate that says how much each line
// counts.  The reference has the weight slot and wires it to 1.0f (ref: EpipolarConsistencyRadonIntermediate.cu:254); its host
// epilogue already returns sum value w / sum w (ref: ...RadonIntermediate.cpp:197-224).
//
// The launches: E1 (if the device geometry is behind the matrices), k01_kernel over all pairs into the Gram call's records (scratch
// of the Gram-family calls alone), pairs_weighted_kernel, sum_gram_kernel over the two columns, the copies.  The metric's kept
// records, kept values and pose-batch scratch are not touched.  The index-list and pose-delta forms are in ecc_weighted_poses.hip; they
// take the base's columns from weighted_base_columns below.
// The transform form is in ecc_weighted_transforms.hip.
// Not here: base columns kept between calls; full-matrices, strided, group and RCCL forms; an incremental mode.
#include "ecc_capi_internal.h"
#include "ecc_sum_order.h"

using namespace ecc_internal;

extern "C" hipError_t ecc_launch_sum_gram(const float* values_d, long long col_stride, long long count, int n_columns, int n_slices,
                                          double* partial_d, hipStream_t stream);

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
// The two columns are in m->gram_values_d, g->col_stride apart, once the stream gets there; *p and *g are the launch as it was made
// (ecc_weighted_poses.hip launches the grids of its poses with the same parameters).
int weighted_base_columns(ecc_metric* m, EccPairParams* p_out, EccWeightedParams* g_out)
{
    ecc_ctx* ctx = m->ctx;
    int rc = set_device(ctx);
    if (rc) return rc;
    const int T = 2;  // columns: c, u
    const int64_t n = m->n_views, n_pairs = n * (n - 1) / 2;
    const int64_t col_stride = (n_pairs + 3) & ~(int64_t)3;

    // (as the first large all-pairs evaluation does: whether this scan's pairs would read row-quad copies; the same bits either way)
    if (!m->quads_decided && n_pairs >= 32768) decide_quad_copies(m);
    EccPairParams& p = *p_out;
    rc = fill_pair_params(m, &p, n_pairs, /*need_e1=*/false);  // the sampling mode of an all-pairs evaluation
    if (rc) return rc;
    rc = m->gram_records_d.ensure(n_pairs, ctx->stream);
    if (!rc) rc = m->gram_values_d.ensure((int64_t)T * col_stride, ctx->stream);
    if (!rc) rc = m->gram_partial_d.ensure((int64_t)T * ecc_sum::SLICES, ctx->stream);
    if (rc) return rc;
    ecc_mark_busy(m);
    rc = ensure_e1(m);  // (see ecc_metric_evaluate_gram)
    if (rc) return rc;
    p.first = 0;
    p.count = n_pairs;
    p.records = m->gram_records_d.ptr;
    HIP_TRY(ecc_launch_k01(&p, ctx->stream));
    const int64_t paired_bytes = (int64_t)(m->n_alpha + 1) * m->pitch * 2 * (int64_t)sizeof(float);
    EccWeightedParams& g = *g_out;
    g.paired_channel_bytes = n * paired_bytes;
    g.quad_channel_bytes = n * m->quad_floats * (int64_t)sizeof(float);
    g.values = m->gram_values_d.ptr;
    g.col_stride = col_stride;
    HIP_TRY(launch_weighted_timed(ctx, &p, &g));
    return ECC_OK;
}
}  // namespace ecc_internal

ECC_EXPORT int ecc_metric_evaluate_weighted(ecc_metric* m, double* value, double* coverage, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!value) return fail(ECC_ERR_INVALID_ARGUMENT, "value is null");
    int rc = weighted_check(m);
    if (rc) return rc;
    ecc_ctx* ctx = m->ctx;
    EccPairParams p;
    EccWeightedParams g;
    rc = weighted_base_columns(m, &p, &g);
    if (rc) return rc;
    const int T = 2;
    const int64_t n = m->n_views, n_pairs = n * (n - 1) / 2;
    const int64_t col_stride = g.col_stride;
    // both columns in the order an all-pairs evaluation of n_pairs values is added in (ecc_sum_order.h)
    const int n_slices = ecc_sum::slices(n_pairs, m->sum_scratch_d.ptr != nullptr);
    HIP_TRY(ecc_launch_sum_gram(m->gram_values_d.ptr, col_stride, n_pairs, T, n_slices, m->gram_partial_d.ptr, ctx->stream));
    std::vector<double> partial((size_t)T * ecc_sum::SLICES);
    HIP_TRY(hipMemcpyAsync(partial.data(), m->gram_partial_d.ptr, sizeof(double) * partial.size(), hipMemcpyDeviceToHost, ctx->stream));
    std::vector<float> cols;
    if (pair_terms) {
        cols.resize((size_t)T * (size_t)col_stride);
        HIP_TRY(hipMemcpyAsync(cols.data(), m->gram_values_d.ptr, sizeof(float) * cols.size(), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(wait_stream_spin(ctx->stream));
    m->done_generation = m->set_generation;
    m->quiet = true;  // the copies are the last thing this call queued, and they have landed
    double sum_c = 0.0, sum_u = 0.0;
    for (int s = 0; s < n_slices; ++s) sum_c += partial[(size_t)s];
    for (int s = 0; s < n_slices; ++s) sum_u += partial[(size_t)ecc_sum::SLICES + s];
    // ref: ...RadonIntermediate.cpp:224 (sum value w / sum w); all weights 1: sum_u == n_pairs, the division of an all-pairs evaluation
    const bool none = sum_u == 0.0;
    *value = none ? 0.0 : sum_c / sum_u;
    if (coverage) *coverage = none ? 0.0 : sum_u / (double)n_pairs;
    if (pair_terms)
        for (int64_t q = 0; q < n_pairs; ++q)
            for (int u = 0; u < T; ++u) pair_terms[(size_t)q * T + u] = cols[(size_t)u * col_stride + q];
    return ECC_OK;
}
