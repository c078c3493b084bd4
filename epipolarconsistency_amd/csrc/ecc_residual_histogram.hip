// ecc_residual_histogram.hip -- ecc_metric_evaluate_residual_histogram[_pairs], ecc_metric_evaluate_variance_residual_histogram[_pairs],
// ecc_host_histogram_quantile: the distribution of the per-sample residual, per view (host code; include/ecc_hip.h states the
// contract, residual_histogram_kernel.hip has the kernels, DESIGN.md 4.34 the reasons).  Every robust call takes a scale delta, and
// the library could only propose one from per-pair figures -- a pair's RMS is pulled up by exactly the outliers the loss is meant to
// reject.  These calls return, from one pair launch, how many samples of every view fall into each bin of |d| (or of |z| = |d| / sigma
// on a metric with variance fields): delta from sample quantiles, a per-view tail share that names the view with the instrument before
// any delta exists, and the calibration check of a variance model.
//
// The launch sequence is a column-form call's (ecc_column_call.h) without value columns, T = S = 0: the checks, column_call_begin --
// the table's room as its more_scratch, the table's memset as its upload_more --, the pair launch between the timing events,
// column_call_finish with the table's copy as its queue_more, the one wait.  It is written once, over the launch (histogram_call).
// Not here: pose-delta and transform batches; the form under line weights (counts would not be integers); range, group and RCCL
// forms; use_corr.
#include "ecc_form_call.h"
#include "ecc_histogram_host.h"
#include "ecc_residual_histogram.h"

using namespace ecc_internal;

namespace {

// What the four calls need of counts, width and n_bins (after the null check of m and the list's own checks), before the device is
// touched; *inv_width = (float)(1.0 / (double)width), formed here, on the host, in float64.
int histogram_check(const uint64_t* counts, float width, int n_bins, float* inv_width)
{
    if (!counts) return fail(ECC_ERR_INVALID_ARGUMENT, "counts is null");
    if (!(width > 0.0f) || !std::isfinite(width)) return fail(ECC_ERR_INVALID_ARGUMENT, "the bin width must be finite and > 0");
    *inv_width = (float)(1.0 / (double)width);
    if (!(*inv_width > 0.0f) || !std::isfinite(*inv_width))
        return fail(ECC_ERR_INVALID_ARGUMENT, "the bin width's reciprocal must be finite and > 0 in float32");
    if (n_bins < ECC_HISTOGRAM_MIN_BINS || n_bins > ECC_HISTOGRAM_MAX_BINS || (n_bins & 63))
        return fail(ECC_ERR_INVALID_ARGUMENT, "n_bins must be a multiple of 64 in [64, 1024]");
    return ECC_OK;
}

// the raw form's conditions on the metric: ecc_metric_evaluate_robust's
int raw_metric_check(const ecc_metric* m)
{
    if (m->n_views < 1) return fail(ECC_ERR_INVALID_ARGUMENT, "projection matrices have not been set");
    if (m->n_views < 2) return fail(ECC_ERR_INVALID_ARGUMENT, "need at least two views (the reference divides 0/0 here)");
    if (m->use_corr) return fail(ECC_ERR_UNSUPPORTED, "the residual histogram is not defined for the correlation cost");
    if ((int64_t)m->dtrs.size() < (int64_t)m->n_views) return fail(ECC_ERR_INVALID_ARGUMENT, "fewer Radon intermediates than projection matrices");
    return ECC_OK;
}

// Everything of a call behind its checks: the table of `count` pairs -- all pairs (idx4 null) or the list -- into counts
// (n_views x n_bins, written completely).  launch(p, table): the form's pair launch.
int histogram_call(ecc_metric* m, const int32_t* idx4, int64_t count, int n_bins, uint64_t* counts,
                   const std::function<hipError_t(const EccPairParams&, unsigned long long*, hipStream_t)>& launch)
{
    const size_t cells = (size_t)m->n_views * (size_t)n_bins;
    if (count == 0) {  // an empty list: nothing was sampled
        std::fill(counts, counts + cells, (uint64_t)0);
        return ECC_OK;
    }
    ecc_ctx* ctx = m->ctx;
    ColumnCall c;
    int rc = column_call_begin(
        m, idx4, count, /*T=*/0, /*S=*/0, &c, [&]() -> int { return m->histogram_d.ensure((int64_t)cells, ctx->stream); },
        [&]() -> int {
            HIP_TRY(hipMemsetAsync(m->histogram_d.ptr, 0, sizeof(unsigned long long) * cells, ctx->stream));
            return ECC_OK;
        });
    if (rc) return rc;
    HIP_TRY(launch_timed(ctx, [&](hipStream_t s) { return launch(c.p, m->histogram_d.ptr, s); }));
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the table's cells are the caller's");
    return column_call_finish(m, c, /*S=*/0, (double*)nullptr, /*T=*/0, (const float*)nullptr, (float*)nullptr, [&]() -> int {
        HIP_TRY(hipMemcpyAsync(counts, m->histogram_d.ptr, sizeof(uint64_t) * cells, hipMemcpyDeviceToHost, ctx->stream));
        return ECC_OK;
    });
}

int raw_call(ecc_metric* m, const int32_t* idx4, int64_t count, float inv_width, int n_bins, uint64_t* counts)
{
    return histogram_call(m, idx4, count, n_bins, counts, [=](const EccPairParams& p, unsigned long long* table, hipStream_t s) {
        EccResidualHistogramParams g;
        g.counts = table;
        g.n_bins = n_bins;
        g.inv_width = inv_width;
        return ecc_launch_pairs_residual_histogram(&p, &g, s);
    });
}

int variance_call(ecc_metric* m, const int32_t* idx4, int64_t count, float floor, float inv_width, int n_bins, uint64_t* counts)
{
    return histogram_call(m, idx4, count, n_bins, counts, [=](const EccPairParams& p, unsigned long long* table, hipStream_t s) {
        EccVarianceResidualHistogramParams g;
        set_channel_strides(m, &g);  // the data channel and, one channel behind it, the variance fields
        g.counts = table;
        g.n_bins = n_bins;
        g.inv_width = inv_width;
        g.floor = floor;
        return ecc_launch_pairs_variance_residual_histogram(&p, &g, s);
    });
}

// the lists of both forms: P index the current matrices, D the DATA intermediates, which are the table's rows
int list_check(const ecc_metric* m, const int32_t* idx4, int n_pairs)
{
    return check_index_list(idx4, n_pairs, m->n_views, m->n_views,
                            "index array contains invalid indices (matrices and data intermediates lie in [0, n_views): the rows of counts)");
}

}  // namespace

ECC_EXPORT int ecc_metric_evaluate_residual_histogram(ecc_metric* m, float width, int n_bins, uint64_t* counts)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    float inv_width = 0.0f;
    int rc = histogram_check(counts, width, n_bins, &inv_width);
    if (!rc) rc = raw_metric_check(m);
    if (rc) return rc;
    const int64_t n = m->n_views;
    return raw_call(m, nullptr, n * (n - 1) / 2, inv_width, n_bins, counts);
}

ECC_EXPORT int ecc_metric_evaluate_residual_histogram_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, float width, int n_bins,
                                                            uint64_t* counts)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    float inv_width = 0.0f;
    int rc = histogram_check(counts, width, n_bins, &inv_width);
    if (rc) return rc;
    if (n_pairs < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "negative list length");
    if (n_pairs > 0 && !idx4) return fail(ECC_ERR_INVALID_ARGUMENT, "index list is null");
    rc = raw_metric_check(m);
    if (!rc) rc = list_check(m, idx4, n_pairs);
    if (rc) return rc;
    return raw_call(m, idx4, n_pairs, inv_width, n_bins, counts);
}

ECC_EXPORT int ecc_metric_evaluate_variance_residual_histogram(ecc_metric* m, float floor, float width, int n_bins, uint64_t* counts)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    float inv_width = 0.0f;
    int rc = histogram_check(counts, width, n_bins, &inv_width);
    if (!rc) rc = variance_check(m, floor);
    if (rc) return rc;
    const int64_t n = m->n_views;
    return variance_call(m, nullptr, n * (n - 1) / 2, floor, inv_width, n_bins, counts);
}

ECC_EXPORT int ecc_metric_evaluate_variance_residual_histogram_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, float floor, float width,
                                                                     int n_bins, uint64_t* counts)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    float inv_width = 0.0f;
    int rc = histogram_check(counts, width, n_bins, &inv_width);
    if (rc) return rc;
    if (n_pairs < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "negative list length");
    if (n_pairs > 0 && !idx4) return fail(ECC_ERR_INVALID_ARGUMENT, "index list is null");
    rc = variance_check(m, floor);
    if (!rc) rc = list_check(m, idx4, n_pairs);
    if (rc) return rc;
    return variance_call(m, idx4, n_pairs, floor, inv_width, n_bins, counts);
}

// Host only, no device (ecc_histogram_host.h).
ECC_EXPORT double ecc_host_histogram_quantile(const uint64_t* counts, int n_bins, double width, double q)
{
    return ecc_histogram_host::histogram_quantile(counts, n_bins, width, q);
}
