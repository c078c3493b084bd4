// ecc_view_coeff.hip -- ecc_metric_evaluate_view_coefficients: the metric at per-view channel coefficients and its gradient (host
// code; include/ecc_hip.h states the contract, view_coeff_kernel.hip has the pair kernels, sum_kernel.hip the sums).  The caller is
// an image-domain correction with coefficients per VIEW -- a gain, an offset or a scatter scale for every view: corrected
// intermediate of view i = sum_c a_c,i D_c,i -- that minimises over n K coefficients with gradient descent, L-BFGS or conjugate
// gradients: the metric is a quadratic form a^T G a, its gradient 2 G a is linear in a, so the same call at a direction v is the
// Hessian-vector product, and the (n K) x (n K) matrix is never formed.  Nothing in the reference corresponds to it.
//
// The launches: E1 (if the device geometry is behind the matrices), one copy of the coefficients, k01_kernel over all pairs into
// the Gram call's records (scratch of the Gram-family calls alone; column_call_begin, ecc_column_call.h), pairs_coeff_kernel,
// sum_gram_kernel over the value column, sum_view_terms_kernel over the gradient columns, the copies of the sums
// (column_call_finish).  The metric's kept records, kept values and pose-batch scratch are not touched.
#include "ecc_column_call.h"

using namespace ecc_internal;

extern "C" hipError_t ecc_launch_pairs_coeff(const EccPairParams* p, const EccViewCoeffParams* g, int n_channels, hipStream_t stream);
extern "C" hipError_t ecc_launch_sum_view_terms(const float* values_d, long long col_stride, int n_views, int n_channels, double* sums_d,
                                                hipStream_t stream);

static_assert(ECC_VIEW_COEFF_MAX_CHANNELS == ECC_GRAM_CHANNELS_MAX, "header and kernels disagree");

ECC_EXPORT int ecc_metric_evaluate_view_coefficients(ecc_metric* m, int n_channels, const float* coeffs, double* value, double* grad,
                                                     float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!value) return fail(ECC_ERR_INVALID_ARGUMENT, "value is null");
    if (!coeffs) return fail(ECC_ERR_INVALID_ARGUMENT, "coeffs is null");
    int rc = channel_form_check(m, n_channels, "n_channels must be in [1, ECC_VIEW_COEFF_MAX_CHANNELS]",
                                "the correlation cost is not a quadratic form of the coefficients");
    if (rc) return rc;
    ecc_ctx* ctx = m->ctx;
    const int K = n_channels, T = 1 + 2 * K;
    const int64_t n = m->n_views, n_pairs = n * (n - 1) / 2;
    ColumnCall c;
    rc = column_call_begin(
        m, nullptr, n_pairs, T, 1, &c,  // the sampling mode of an all-pairs evaluation
        [&]() -> int {
            const int e = m->coeff_d.ensure((int64_t)K * n, ctx->stream);
            return e ? e : m->coeff_sums_d.ensure((int64_t)K * n, ctx->stream);
        },
        [&]() -> int {
            HIP_TRY(hipMemcpyAsync(m->coeff_d.ptr, coeffs, sizeof(float) * (size_t)(K * n), hipMemcpyHostToDevice, ctx->stream));
            return ECC_OK;
        });
    if (rc) return rc;
    EccViewCoeffParams g;
    set_channel_strides(m, &g);
    g.values = m->gram_values_d.ptr;
    g.col_stride = c.col_stride;
    g.coeffs = m->coeff_d.ptr;
    HIP_TRY(launch_timed(ctx, [&](hipStream_t s) { return ecc_launch_pairs_coeff(&c.p, &g, K, s); }));
    // the value column in the order an all-pairs evaluation of n_pairs values is added in (ecc_sum_order.h); the gradient columns per
    // (view, channel) in sum_view_terms_kernel's order
    double total = 0.0;
    std::vector<double> sums;
    rc = column_call_finish(m, c, 1, &total, T, m->gram_values_d.ptr, pair_terms, [&]() -> int {
        if (!grad) return ECC_OK;
        HIP_TRY(ecc_launch_sum_view_terms(m->gram_values_d.ptr, c.col_stride, (int)n, K, m->coeff_sums_d.ptr, ctx->stream));
        sums.resize((size_t)(K * n));
        HIP_TRY(hipMemcpyAsync(sums.data(), m->coeff_sums_d.ptr, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, ctx->stream));
        return ECC_OK;
    });
    if (rc) return rc;
    *value = total / (double)n_pairs;  // ref: ...RadonIntermediate.cpp:224 (all weights are 1)
    if (grad)
        for (int64_t k = 0; k < K * n; ++k) grad[k] = 2.0 * sums[(size_t)k] / (double)n_pairs;
    return ECC_OK;
}
