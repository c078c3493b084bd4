// ecc_gram.hip -- ecc_metric_evaluate_gram: the metric as a quadratic form of channel coefficients (host code; include/ecc_hip.h
// states the contract, gram_kernel.hip has the kernels).  The caller is an image-domain correction loop -- beam-hardening
// linearisation, scatter or offset correction: corrected image of view i = sum_c a_c I_c,i -- that moves the images and leaves
// the matrices alone; one call gives it the metric for every coefficient vector.  Nothing in the reference corresponds to it.
//
// The launches: E1 (if the device geometry is behind the matrices), k01_kernel over all pairs into records of this call's own,
// pairs_gram_kernel (one channel: the pair launch of an all-pairs evaluation), sum_gram_kernel, one copy of the slice sums.
// The metric's kept records, kept values and pose-batch scratch are not touched.
#include "ecc_capi_internal.h"
#include "ecc_sum_order.h"

using namespace ecc_internal;

extern "C" hipError_t ecc_launch_pairs_gram(const EccPairParams* p, const EccGramParams* g, int n_channels, hipStream_t stream);
extern "C" hipError_t ecc_launch_sum_gram(const float* values_d, long long col_stride, long long count, int n_columns, int n_slices,
                                          double* partial_d, hipStream_t stream);

static_assert(ECC_GRAM_MAX_CHANNELS == ECC_GRAM_CHANNELS_MAX, "header and kernels disagree");

ECC_EXPORT int ecc_metric_evaluate_gram(ecc_metric* m, int n_channels, float* pair_grams, double* gram)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!gram) return fail(ECC_ERR_INVALID_ARGUMENT, "gram is null");
    if (n_channels < 1 || n_channels > ECC_GRAM_MAX_CHANNELS)
        return fail(ECC_ERR_INVALID_ARGUMENT, "n_channels must be in [1, ECC_GRAM_MAX_CHANNELS]");
    if (m->n_views < 1) return fail(ECC_ERR_INVALID_ARGUMENT, "projection matrices have not been set");
    if (m->n_views < 2) return fail(ECC_ERR_INVALID_ARGUMENT, "need at least two views (the reference divides 0/0 here)");
    if ((int64_t)m->dtrs.size() != (int64_t)n_channels * m->n_views)
        return fail(ECC_ERR_INVALID_ARGUMENT, "the metric must hold n_channels * n_views Radon intermediates, channel-major");
    if (m->use_corr) return fail(ECC_ERR_UNSUPPORTED, "the correlation cost is not a quadratic form of the channel coefficients");
    ecc_ctx* ctx = m->ctx;
    int rc = set_device(ctx);
    if (rc) return rc;
    const int K = n_channels, T = K * (K + 1) / 2;
    const int64_t n = m->n_views, n_pairs = n * (n - 1) / 2;
    const int64_t col_stride = (n_pairs + 3) & ~(int64_t)3;

    // (as the first large all-pairs evaluation does: whether this scan's pairs would read row-quad copies; the same bits either way)
    if (!m->quads_decided && n_pairs >= 32768) decide_quad_copies(m);
    EccPairParams p;
    rc = fill_pair_params(m, &p, n_pairs, /*need_e1=*/false);  // the sampling mode of an all-pairs evaluation
    if (rc) return rc;
    rc = m->gram_records_d.ensure(n_pairs, ctx->stream);
    if (!rc) rc = m->gram_values_d.ensure((int64_t)T * col_stride, ctx->stream);
    if (!rc) rc = m->gram_partial_d.ensure((int64_t)T * ecc_sum::SLICES, ctx->stream);
    if (rc) return rc;
    ecc_mark_busy(m);
    // the device geometry of the current matrices (a no-op unless a view is behind its matrix; ensure_e1 keeps the books the
    // other paths read: the kept records are declared stale exactly when the geometry under them changes)
    rc = ensure_e1(m);
    if (rc) return rc;
    p.first = 0;
    p.count = n_pairs;
    p.records = m->gram_records_d.ptr;
    HIP_TRY(ecc_launch_k01(&p, ctx->stream));
    if (K == 1) {  // the pair launch of ecc_metric_evaluate_all
        p.pair_values = m->gram_values_d.ptr;
        HIP_TRY(launch_pairs_timed(ctx, &p));
    } else {
        const int64_t paired_bytes = (int64_t)(m->n_alpha + 1) * m->pitch * 2 * (int64_t)sizeof(float);
        EccGramParams g;
        g.paired_channel_bytes = n * paired_bytes;
        g.quad_channel_bytes = n * m->quad_floats * (int64_t)sizeof(float);
        g.values = m->gram_values_d.ptr;
        g.col_stride = col_stride;
        if (ctx->timing) HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
        HIP_TRY(ecc_launch_pairs_gram(&p, &g, K, ctx->stream));
        if (ctx->timing) {
            HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
            ctx->ev_valid[0] = true;
        }
    }
    // the column sums in the order an all-pairs evaluation of n_pairs values is added in (ecc_sum_order.h)
    const int n_slices = ecc_sum::slices(n_pairs, m->sum_scratch_d.ptr != nullptr);
    HIP_TRY(ecc_launch_sum_gram(m->gram_values_d.ptr, col_stride, n_pairs, T, n_slices, m->gram_partial_d.ptr, ctx->stream));
    std::vector<double> partial((size_t)T * ecc_sum::SLICES);
    HIP_TRY(hipMemcpyAsync(partial.data(), m->gram_partial_d.ptr, sizeof(double) * partial.size(), hipMemcpyDeviceToHost, ctx->stream));
    std::vector<float> cols;
    if (pair_grams) {
        cols.resize((size_t)T * (size_t)col_stride);
        HIP_TRY(hipMemcpyAsync(cols.data(), m->gram_values_d.ptr, sizeof(float) * cols.size(), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(wait_stream_spin(ctx->stream));
    m->done_generation = m->set_generation;
    m->quiet = true;  // the copies are the last thing this call queued, and they have landed
    int t = 0;
    for (int c = 0; c < K; ++c)
        for (int d = c; d < K; ++d, ++t) {
            double tot = 0.0;
            for (int s = 0; s < n_slices; ++s) tot += partial[(size_t)t * ecc_sum::SLICES + s];
            const double mean = tot / (double)n_pairs;  // ref: ...RadonIntermediate.cpp:224 (all weights are 1)
            gram[(size_t)c * K + d] = mean;
            gram[(size_t)d * K + c] = mean;  // symmetric by construction: only c <= d is computed
        }
    if (pair_grams)
        for (int64_t q = 0; q < n_pairs; ++q)
            for (int u = 0; u < T; ++u) pair_grams[(size_t)q * T + u] = cols[(size_t)u * col_stride + q];
    return ECC_OK;
}
