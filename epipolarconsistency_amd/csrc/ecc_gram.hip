// ecc_gram.hip -- ecc_metric_evaluate_gram: the metric as a quadratic form of channel coefficients (host code; include/ecc_hip.h
// states the contract, gram_kernel.hip has the kernels).  The caller is an image-domain correction loop -- beam-hardening
// linearisation, scatter or offset correction: corrected image of view i = sum_c a_c I_c,i -- that moves the images and leaves
// the matrices alone; one call gives it the metric for every coefficient vector.  Nothing in the reference corresponds to it.
//
// The launches: E1 (if the device geometry is behind the matrices), k01_kernel over all pairs into records of this call's own
// (column_call_begin, ecc_column_call.h), pairs_gram_kernel (one channel: the pair launch of an all-pairs evaluation),
// sum_gram_kernel, one copy of the slice sums (column_call_finish).
// The metric's kept records, kept values and pose-batch scratch are not touched.
#include "ecc_column_call.h"

using namespace ecc_internal;

extern "C" hipError_t ecc_launch_pairs_gram(const EccPairParams* p, const EccGramParams* g, int n_channels, hipStream_t stream);

static_assert(ECC_GRAM_MAX_CHANNELS == ECC_GRAM_CHANNELS_MAX, "header and kernels disagree");

namespace ecc_internal {
int channel_form_check(const ecc_metric* m, int n_channels, const char* range_text, const char* corr_text)
{
    if (n_channels < 1 || n_channels > ECC_GRAM_CHANNELS_MAX) return fail(ECC_ERR_INVALID_ARGUMENT, range_text);
    if (m->n_views < 1) return fail(ECC_ERR_INVALID_ARGUMENT, "projection matrices have not been set");
    if (m->n_views < 2) return fail(ECC_ERR_INVALID_ARGUMENT, "need at least two views (the reference divides 0/0 here)");
    if ((int64_t)m->dtrs.size() != (int64_t)n_channels * m->n_views)
        return fail(ECC_ERR_INVALID_ARGUMENT, "the metric must hold n_channels * n_views Radon intermediates, channel-major");
    if (m->use_corr) return fail(ECC_ERR_UNSUPPORTED, corr_text);
    return ECC_OK;
}
}  // namespace ecc_internal

ECC_EXPORT int ecc_metric_evaluate_gram(ecc_metric* m, int n_channels, float* pair_grams, double* gram)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!gram) return fail(ECC_ERR_INVALID_ARGUMENT, "gram is null");
    int rc = channel_form_check(m, n_channels, "n_channels must be in [1, ECC_GRAM_MAX_CHANNELS]",
                                "the correlation cost is not a quadratic form of the channel coefficients");
    if (rc) return rc;
    const int K = n_channels, T = K * (K + 1) / 2;
    const int64_t n = m->n_views, n_pairs = n * (n - 1) / 2;
    ColumnCall c;
    rc = column_call_begin(m, nullptr, n_pairs, T, T, &c);  // the sampling mode of an all-pairs evaluation
    if (rc) return rc;
    if (K == 1) {  // the pair launch of ecc_metric_evaluate_all
        c.p.pair_values = m->gram_values_d.ptr;
        HIP_TRY(launch_pairs_timed(m->ctx, &c.p));
    } else {
        EccGramParams g;
        set_channel_strides(m, &g);
        g.values = m->gram_values_d.ptr;
        g.col_stride = c.col_stride;
        HIP_TRY(launch_timed(m->ctx, [&](hipStream_t s) { return ecc_launch_pairs_gram(&c.p, &g, K, s); }));
    }
    std::vector<double> totals((size_t)T);
    rc = column_call_finish(m, c, T, totals.data(), T, m->gram_values_d.ptr, pair_grams);
    if (rc) return rc;
    int t = 0;
    for (int c0 = 0; c0 < K; ++c0)
        for (int d = c0; d < K; ++d, ++t) {
            const double mean = totals[(size_t)t] / (double)n_pairs;  // ref: ...RadonIntermediate.cpp:224 (all weights are 1)
            gram[(size_t)c0 * K + d] = mean;
            gram[(size_t)d * K + c0] = mean;  // symmetric by construction: only c <= d is computed
        }
    return ECC_OK;
}
