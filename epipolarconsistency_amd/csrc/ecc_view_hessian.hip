// ecc_view_hessian.hip -- ecc_metric_evaluate_view_hessian: the quadratic form of per-view channel coefficients as a matrix (host
// code; include/ecc_hip.h states the contract, view_hessian_kernel.hip has the kernels).  The caller needs the form itself and not
// its products: a direct constrained solve, a regularisation sweep, many gauge or constraint choices on one data set, an
// eigen-analysis of what the data do not determine.  One call, then every coefficient vector in closed form on the host -- what
// ecc_metric_evaluate_gram gives the shared case.  Nothing in the reference corresponds to it.
//
// The launches: E1 (if the device geometry is behind the matrices), k01_kernel over all pairs into the Gram call's records (scratch
// of these calls alone; column_call_begin, ecc_column_call.h), pairs_moments_kernel into float64 columns of this call's own,
// assemble_view_hessian_kernel, the copies (column_call_finish: no column is summed).
// The metric's kept records, kept values and pose-batch scratch are not touched.
#include "ecc_column_call.h"

using namespace ecc_internal;

extern "C" hipError_t ecc_launch_pairs_moments(const EccPairParams* p, const EccViewMomentParams* g, int n_channels, hipStream_t stream);
extern "C" hipError_t ecc_launch_assemble_view_hessian(const double* values_d, long long col_stride, int n_views, int n_channels, double* H_d,
                                                       hipStream_t stream);

static_assert(ECC_VIEW_HESSIAN_MAX_CHANNELS == ECC_GRAM_CHANNELS_MAX, "header and kernels disagree");
static const int64_t VIEW_HESSIAN_KEEP_BYTES = (int64_t)64 << 20;  // 2 828 coefficients; 400 views of four channels are 20 MB

ECC_EXPORT int ecc_metric_evaluate_view_hessian(ecc_metric* m, int n_channels, double* hessian, double* pair_blocks)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!hessian && !pair_blocks) return fail(ECC_ERR_INVALID_ARGUMENT, "hessian and pair_blocks are both null");
    int rc = channel_form_check(m, n_channels, "n_channels must be in [1, ECC_VIEW_HESSIAN_MAX_CHANNELS]",
                                "the correlation cost is not a quadratic form of the coefficients");
    if (rc) return rc;
    const int K = n_channels, T2 = K * (K + 1) + K * K;
    const int64_t n = m->n_views, n_pairs = n * (n - 1) / 2, dim = n * K;
    if (hessian && dim > ECC_VIEW_HESSIAN_MAX_DIM)
        return fail(ECC_ERR_UNSUPPORTED, "n_views * n_channels exceeds ECC_VIEW_HESSIAN_MAX_DIM (ask for pair_blocks alone)");
    ecc_ctx* ctx = m->ctx;
    ColumnCall c;
    rc = column_call_begin(
        m, nullptr, n_pairs, 0, 0, &c,  // the sampling mode of an all-pairs evaluation; no float column
        [&]() -> int {
            const int e = m->view_moments_d.ensure((int64_t)T2 * c.col_stride, ctx->stream);
            return e || !hessian ? e : m->view_hessian_d.ensure(dim * dim, ctx->stream);
        },
        no_more);
    if (rc) return rc;
    EccViewMomentParams g;
    set_channel_strides(m, &g);
    g.values = m->view_moments_d.ptr;
    g.col_stride = c.col_stride;
    HIP_TRY(launch_timed(ctx, [&](hipStream_t s) { return ecc_launch_pairs_moments(&c.p, &g, K, s); }));
    rc = column_call_finish(m, c, 0, nullptr, T2, m->view_moments_d.ptr, pair_blocks, [&]() -> int {
        if (!hessian) return ECC_OK;  // the one large copy goes straight to the caller's array (20 MB at 400 views and four channels)
        HIP_TRY(ecc_launch_assemble_view_hessian(m->view_moments_d.ptr, c.col_stride, (int)n, K, m->view_hessian_d.ptr, ctx->stream));
        HIP_TRY(hipMemcpyAsync(hessian, m->view_hessian_d.ptr, sizeof(double) * (size_t)(dim * dim), hipMemcpyDeviceToHost, ctx->stream));
        return ECC_OK;
    });
    if (rc) return rc;
    // the matrix on the device is scratch of this call: kept for the next call while it is small (the copy dominates a repeated call
    // anyway), given back when it is not -- up to 512 MB would otherwise stay with the metric for its lifetime
    if (hessian && dim * dim * (int64_t)sizeof(double) > VIEW_HESSIAN_KEEP_BYTES) m->view_hessian_d.reset();
    return ECC_OK;
}
