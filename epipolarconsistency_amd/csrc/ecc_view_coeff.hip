// ecc_view_coeff.hip -- ecc_metric_evaluate_view_coefficients: the metric at per-view channel coefficients and its gradient (host
// code; include/ecc_hip.h states the contract, view_coeff_kernel.hip has the pair kernels, sum_kernel.hip the sums).  The caller is
// an image-domain correction with coefficients per VIEW -- a gain, an offset or a scatter scale for every view: corrected
// intermediate of view i = sum_c a_c,i D_c,i -- that minimises over n K coefficients with gradient descent, L-BFGS or conjugate
// gradients: the metric is a quadratic form a^T G a, its gradient 2 G a is linear in a, so the same call at a direction v is the
// Hessian-vector product, and the (n K) x (n K) matrix is never formed.  Nothing in the reference corresponds to it.
//
// The launches: E1 (if the device geometry is behind the matrices), one copy of the coefficients, k01_kernel over all pairs into
// the Gram call's records (scratch of these two calls alone), pairs_coeff_kernel, sum_gram_kernel over the value column,
// sum_view_terms_kernel over the gradient columns, the copies of the sums.  The metric's kept records, kept values and pose-batch
// scratch are not touched.
#include "ecc_capi_internal.h"
#include "ecc_sum_order.h"

using namespace ecc_internal;

extern "C" hipError_t ecc_launch_pairs_coeff(const EccPairParams* p, const EccViewCoeffParams* g, int n_channels, hipStream_t stream);
extern "C" hipError_t ecc_launch_sum_gram(const float* values_d, long long col_stride, long long count, int n_columns, int n_slices,
                                          double* partial_d, hipStream_t stream);
extern "C" hipError_t ecc_launch_sum_view_terms(const float* values_d, long long col_stride, int n_views, int n_channels, double* sums_d,
                                                hipStream_t stream);

static_assert(ECC_VIEW_COEFF_MAX_CHANNELS == ECC_GRAM_CHANNELS_MAX, "header and kernels disagree");

ECC_EXPORT int ecc_metric_evaluate_view_coefficients(ecc_metric* m, int n_channels, const float* coeffs, double* value, double* grad,
                                                     float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!value) return fail(ECC_ERR_INVALID_ARGUMENT, "value is null");
    if (!coeffs) return fail(ECC_ERR_INVALID_ARGUMENT, "coeffs is null");
    if (n_channels < 1 || n_channels > ECC_VIEW_COEFF_MAX_CHANNELS)
        return fail(ECC_ERR_INVALID_ARGUMENT, "n_channels must be in [1, ECC_VIEW_COEFF_MAX_CHANNELS]");
    if (m->n_views < 1) return fail(ECC_ERR_INVALID_ARGUMENT, "projection matrices have not been set");
    if (m->n_views < 2) return fail(ECC_ERR_INVALID_ARGUMENT, "need at least two views (the reference divides 0/0 here)");
    if ((int64_t)m->dtrs.size() != (int64_t)n_channels * m->n_views)
        return fail(ECC_ERR_INVALID_ARGUMENT, "the metric must hold n_channels * n_views Radon intermediates, channel-major");
    if (m->use_corr) return fail(ECC_ERR_UNSUPPORTED, "the correlation cost is not a quadratic form of the coefficients");
    ecc_ctx* ctx = m->ctx;
    int rc = set_device(ctx);
    if (rc) return rc;
    const int K = n_channels, T = 1 + 2 * K;
    const int64_t n = m->n_views, n_pairs = n * (n - 1) / 2;
    const int64_t col_stride = (n_pairs + 3) & ~(int64_t)3;

    // (as the first large all-pairs evaluation does: whether this scan's pairs would read row-quad copies; the same bits either way)
    if (!m->quads_decided && n_pairs >= 32768) decide_quad_copies(m);
    EccPairParams p;
    rc = fill_pair_params(m, &p, n_pairs, /*need_e1=*/false);  // the sampling mode of an all-pairs evaluation
    if (rc) return rc;
    rc = m->gram_records_d.ensure(n_pairs, ctx->stream);
    if (!rc) rc = m->gram_values_d.ensure((int64_t)T * col_stride, ctx->stream);
    if (!rc) rc = m->gram_partial_d.ensure(ecc_sum::SLICES, ctx->stream);
    if (!rc) rc = m->coeff_d.ensure((int64_t)K * n, ctx->stream);
    if (!rc) rc = m->coeff_sums_d.ensure((int64_t)K * n, ctx->stream);
    if (rc) return rc;
    ecc_mark_busy(m);
    rc = ensure_e1(m);  // (see ecc_metric_evaluate_gram)
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(m->coeff_d.ptr, coeffs, sizeof(float) * (size_t)(K * n), hipMemcpyHostToDevice, ctx->stream));
    p.first = 0;
    p.count = n_pairs;
    p.records = m->gram_records_d.ptr;
    HIP_TRY(ecc_launch_k01(&p, ctx->stream));
    const int64_t paired_bytes = (int64_t)(m->n_alpha + 1) * m->pitch * 2 * (int64_t)sizeof(float);
    EccViewCoeffParams g;
    g.paired_channel_bytes = n * paired_bytes;
    g.quad_channel_bytes = n * m->quad_floats * (int64_t)sizeof(float);
    g.values = m->gram_values_d.ptr;
    g.col_stride = col_stride;
    g.coeffs = m->coeff_d.ptr;
    if (ctx->timing) HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
    HIP_TRY(ecc_launch_pairs_coeff(&p, &g, K, ctx->stream));
    if (ctx->timing) {
        HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
        ctx->ev_valid[0] = true;
    }
    // the value column in the order an all-pairs evaluation of n_pairs values is added in (ecc_sum_order.h); the gradient columns per
    // (view, channel) in sum_view_terms_kernel's order
    const int n_slices = ecc_sum::slices(n_pairs, m->sum_scratch_d.ptr != nullptr);
    HIP_TRY(ecc_launch_sum_gram(m->gram_values_d.ptr, col_stride, n_pairs, 1, n_slices, m->gram_partial_d.ptr, ctx->stream));
    std::vector<double> partial(ecc_sum::SLICES), sums;
    HIP_TRY(hipMemcpyAsync(partial.data(), m->gram_partial_d.ptr, sizeof(double) * partial.size(), hipMemcpyDeviceToHost, ctx->stream));
    if (grad) {
        HIP_TRY(ecc_launch_sum_view_terms(m->gram_values_d.ptr, col_stride, (int)n, K, m->coeff_sums_d.ptr, ctx->stream));
        sums.resize((size_t)(K * n));
        HIP_TRY(hipMemcpyAsync(sums.data(), m->coeff_sums_d.ptr, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, ctx->stream));
    }
    std::vector<float> cols;
    if (pair_terms) {
        cols.resize((size_t)T * (size_t)col_stride);
        HIP_TRY(hipMemcpyAsync(cols.data(), m->gram_values_d.ptr, sizeof(float) * cols.size(), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(wait_stream_spin(ctx->stream));
    m->done_generation = m->set_generation;
    m->quiet = true;  // the copies are the last thing this call queued, and they have landed
    double tot = 0.0;
    for (int s = 0; s < n_slices; ++s) tot += partial[(size_t)s];
    *value = tot / (double)n_pairs;  // ref: ...RadonIntermediate.cpp:224 (all weights are 1)
    if (grad)
        for (int64_t k = 0; k < K * n; ++k) grad[k] = 2.0 * sums[(size_t)k] / (double)n_pairs;
    if (pair_terms)
        for (int64_t q = 0; q < n_pairs; ++q)
            for (int u = 0; u < T; ++u) pair_terms[(size_t)q * T + u] = cols[(size_t)u * col_stride + q];
    return ECC_OK;
}
