// ecc_view_hessian.hip -- ecc_metric_evaluate_view_hessian: the quadratic form of per-view channel coefficients as a matrix (host
// code; include/ecc_hip.h states the contract, view_hessian_kernel.hip has the kernels).  The caller needs the form itself and not
// its products: a direct constrained solve, a regularisation sweep, many gauge or constraint choices on one data set, an
// eigen-analysis of what the data do not determine.  One call, then every coefficient vector in closed form on the host -- what
// ecc_metric_evaluate_gram gives the shared case.  Nothing in the reference corresponds to it.
//
// The launches: E1 (if the device geometry is behind the matrices), k01_kernel over all pairs into the Gram call's records (scratch
// of these calls alone), pairs_moments_kernel into float64 columns of this call's own, assemble_view_hessian_kernel, the copies.
// The metric's kept records, kept values and pose-batch scratch are not touched.
#include "ecc_capi_internal.h"

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
    if (n_channels < 1 || n_channels > ECC_VIEW_HESSIAN_MAX_CHANNELS)
        return fail(ECC_ERR_INVALID_ARGUMENT, "n_channels must be in [1, ECC_VIEW_HESSIAN_MAX_CHANNELS]");
    if (m->n_views < 1) return fail(ECC_ERR_INVALID_ARGUMENT, "projection matrices have not been set");
    if (m->n_views < 2) return fail(ECC_ERR_INVALID_ARGUMENT, "need at least two views (the reference divides 0/0 here)");
    if ((int64_t)m->dtrs.size() != (int64_t)n_channels * m->n_views)
        return fail(ECC_ERR_INVALID_ARGUMENT, "the metric must hold n_channels * n_views Radon intermediates, channel-major");
    if (m->use_corr) return fail(ECC_ERR_UNSUPPORTED, "the correlation cost is not a quadratic form of the coefficients");
    const int K = n_channels, T2 = K * (K + 1) + K * K;
    const int64_t n = m->n_views, n_pairs = n * (n - 1) / 2, dim = n * K;
    if (hessian && dim > ECC_VIEW_HESSIAN_MAX_DIM)
        return fail(ECC_ERR_UNSUPPORTED, "n_views * n_channels exceeds ECC_VIEW_HESSIAN_MAX_DIM (ask for pair_blocks alone)");
    ecc_ctx* ctx = m->ctx;
    int rc = set_device(ctx);
    if (rc) return rc;
    const int64_t col_stride = (n_pairs + 3) & ~(int64_t)3;

    // (as the first large all-pairs evaluation does: whether this scan's pairs would read row-quad copies; the same bits either way)
    if (!m->quads_decided && n_pairs >= 32768) decide_quad_copies(m);
    EccPairParams p;
    rc = fill_pair_params(m, &p, n_pairs, /*need_e1=*/false);  // the sampling mode of an all-pairs evaluation
    if (rc) return rc;
    rc = m->gram_records_d.ensure(n_pairs, ctx->stream);
    if (!rc) rc = m->view_moments_d.ensure((int64_t)T2 * col_stride, ctx->stream);
    if (!rc && hessian) rc = m->view_hessian_d.ensure(dim * dim, ctx->stream);
    if (rc) return rc;
    ecc_mark_busy(m);
    rc = ensure_e1(m);  // (see ecc_metric_evaluate_gram)
    if (rc) return rc;
    p.first = 0;
    p.count = n_pairs;
    p.records = m->gram_records_d.ptr;
    HIP_TRY(ecc_launch_k01(&p, ctx->stream));
    const int64_t paired_bytes = (int64_t)(m->n_alpha + 1) * m->pitch * 2 * (int64_t)sizeof(float);
    EccViewMomentParams g;
    g.paired_channel_bytes = n * paired_bytes;
    g.quad_channel_bytes = n * m->quad_floats * (int64_t)sizeof(float);
    g.values = m->view_moments_d.ptr;
    g.col_stride = col_stride;
    if (ctx->timing) HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
    HIP_TRY(ecc_launch_pairs_moments(&p, &g, K, ctx->stream));
    if (ctx->timing) {
        HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
        ctx->ev_valid[0] = true;
    }
    std::vector<double> cols;
    if (hessian) {  // the one large copy goes straight to the caller's array (20 MB at 400 views and four channels)
        HIP_TRY(ecc_launch_assemble_view_hessian(m->view_moments_d.ptr, col_stride, (int)n, K, m->view_hessian_d.ptr, ctx->stream));
        HIP_TRY(hipMemcpyAsync(hessian, m->view_hessian_d.ptr, sizeof(double) * (size_t)(dim * dim), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (pair_blocks) {
        cols.resize((size_t)T2 * (size_t)col_stride);
        HIP_TRY(hipMemcpyAsync(cols.data(), m->view_moments_d.ptr, sizeof(double) * cols.size(), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(wait_stream_spin(ctx->stream));
    m->done_generation = m->set_generation;
    m->quiet = true;  // the copies are the last thing this call queued, and they have landed
    // the matrix on the device is scratch of this call: kept for the next call while it is small (the copy dominates a repeated call
    // anyway), given back when it is not -- up to 512 MB would otherwise stay with the metric for its lifetime
    if (hessian && dim * dim * (int64_t)sizeof(double) > VIEW_HESSIAN_KEEP_BYTES) m->view_hessian_d.reset();
    if (pair_blocks)
        for (int64_t q = 0; q < n_pairs; ++q)
            for (int u = 0; u < T2; ++u) pair_blocks[(size_t)q * T2 + u] = cols[(size_t)u * col_stride + q];
    return ECC_OK;
}
