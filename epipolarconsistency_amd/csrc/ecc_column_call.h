// ecc_column_call.h -- the host side of a column-form call, once.  A column-form call evaluates `count` pairs --
// all pairs of the current matrices, or an index list -- with a pair kernel that stores T columns per pair, col_stride apart, and
// returns the float64 totals of the leading S columns and, on request, the columns as rows.  ecc_metric_evaluate_gram,
// _view_coefficients, _view_hessian, _weighted, _weighted_pairs, _robust[_pairs] and _weighted_robust[_pairs] are such calls (the
// weighted and robust families through ecc_form_call.h, which states their four steps once):
//   its checks                 every one returns before the device is touched
//   column_call_begin          everything up to and including the record launch
//   its own parameter struct and pair launch, between the timing events (launch_timed)
//   column_call_finish         sum_gram_kernel over the S columns, the copies, the wait, the totals, the rows
// The records, the float columns and the slice sums are the Gram family's scratch (gram_records_d, gram_values_d, gram_partial_d):
// the metric's kept records, kept values and pose-batch values are not touched.
#ifndef ECC_COLUMN_CALL_H
#define ECC_COLUMN_CALL_H

#include "ecc_capi_internal.h"
#include "ecc_sum_order.h"

extern "C" hipError_t ecc_launch_sum_gram(const float* values_d, long long col_stride, long long count, int n_columns, int n_slices,
                                          double* partial_d, hipStream_t stream);

namespace ecc_internal {

struct ColumnCall {
    EccPairParams p;                    // the record launch as it was made: first 0, `count` pairs, records in gram_records_d
    int64_t count = 0, col_stride = 0;  // the pairs; the distance of two columns (count rounded up to whole float4)
};

inline int no_more() { return ECC_OK; }

// `count` pairs -- all pairs (idx4 null) or the list -- under the sampling mode of that many values: the device, the quad-copy
// decision of a first large all-pairs evaluation, the launch parameters, room for the records, T float columns and S x SLICES
// slice sums (and the list), more_scratch() for what else the form needs room for, E1 if the device geometry is behind the
// matrices, the list's upload and upload_more() for what else the form's pair kernel reads, k01_kernel.  Nothing is queued before
// more_scratch has returned; c->count and c->col_stride are set before either hook runs.
template <class MoreScratch, class UploadMore>
int column_call_begin(ecc_metric* m, const int32_t* idx4, int64_t count, int T, int S, ColumnCall* c, MoreScratch&& more_scratch,
                      UploadMore&& upload_more)
{
    ecc_ctx* ctx = m->ctx;
    int rc = set_device(ctx);
    if (rc) return rc;
    c->count = count;
    c->col_stride = (count + 3) & ~(int64_t)3;
    // (as the first large all-pairs evaluation does: whether this scan's pairs would read row-quad copies; the same bits either way)
    if (!idx4 && !m->quads_decided && count >= 32768) decide_quad_copies(m);
    EccPairParams& p = c->p;
    rc = fill_pair_params(m, &p, count, /*need_e1=*/false);
    if (rc) return rc;
    rc = m->gram_records_d.ensure(count, ctx->stream);
    if (!rc && T > 0) rc = m->gram_values_d.ensure((int64_t)T * c->col_stride, ctx->stream);
    if (!rc && S > 0) rc = m->gram_partial_d.ensure((int64_t)S * ecc_sum::SLICES, ctx->stream);
    if (!rc && idx4) rc = m->pose_idx_d.ensure(4 * count, ctx->stream);  // (the pose batch's index scratch)
    if (!rc) rc = more_scratch();
    if (rc) return rc;
    ecc_mark_busy(m);
    // the device geometry of the current matrices (a no-op unless a view is behind its matrix; ensure_e1 keeps the books the
    // other paths read: the kept records are declared stale exactly when the geometry under them changes)
    rc = ensure_e1(m);
    if (rc) return rc;
    if (idx4) {
        HIP_TRY(hipMemcpyAsync(m->pose_idx_d.ptr, idx4, sizeof(int32_t) * 4 * (size_t)count, hipMemcpyHostToDevice, ctx->stream));
        p.indices = m->pose_idx_d.ptr;
    }
    rc = upload_more();
    if (rc) return rc;
    p.first = 0;
    p.count = count;
    p.records = m->gram_records_d.ptr;
    HIP_TRY(ecc_launch_k01(&p, ctx->stream));
    return ECC_OK;
}
inline int column_call_begin(ecc_metric* m, const int32_t* idx4, int64_t count, int T, int S, ColumnCall* c)
{
    return column_call_begin(m, idx4, count, T, S, c, no_more, no_more);
}

// rows[q * T + u] = cols[u * col_stride + q]: what the device keeps as columns, as the caller's rows.
template <class V>
void columns_to_rows(const V* cols, int64_t col_stride, int64_t count, int T, V* rows)
{
    for (int64_t q = 0; q < count; ++q)
        for (int u = 0; u < T; ++u) rows[(size_t)q * T + u] = cols[(size_t)u * col_stride + q];
}

// Behind the pair launch.  totals[0 .. S): the leading S float columns of gram_values_d, each summed in the order an evaluation of
// `count` values is added in (ecc_sum_order.h: sum_gram_kernel's slice sums, added here in slice order).  rows (nullable, host):
// the T columns of cols_d -- float or double -- as count x T.  queue_more() queues what else the call wants done before the one wait.
// When it returns, everything the call queued has landed and the metric is quiet.
template <class V, class QueueMore>
int column_call_finish(ecc_metric* m, const ColumnCall& c, int S, double* totals, int T, const V* cols_d, V* rows, QueueMore&& queue_more)
{
    ecc_ctx* ctx = m->ctx;
    const int n_slices = ecc_sum::slices(c.count, m->sum_scratch_d.ptr != nullptr);
    std::vector<double> partial((size_t)S * ecc_sum::SLICES);
    if (S > 0) {
        HIP_TRY(ecc_launch_sum_gram(m->gram_values_d.ptr, c.col_stride, c.count, S, n_slices, m->gram_partial_d.ptr, ctx->stream));
        HIP_TRY(hipMemcpyAsync(partial.data(), m->gram_partial_d.ptr, sizeof(double) * partial.size(), hipMemcpyDeviceToHost, ctx->stream));
    }
    const int rc = queue_more();
    if (rc) return rc;
    std::vector<V> cols;
    if (rows) {
        cols.resize((size_t)T * (size_t)c.col_stride);
        HIP_TRY(hipMemcpyAsync(cols.data(), cols_d, sizeof(V) * cols.size(), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(wait_stream_spin(ctx->stream));
    m->done_generation = m->set_generation;
    m->quiet = true;  // the copies are the last thing this call queued, and they have landed
    for (int t = 0; t < S; ++t) {
        double tot = 0.0;
        for (int s = 0; s < n_slices; ++s) tot += partial[(size_t)t * ecc_sum::SLICES + s];
        totals[t] = tot;
    }
    if (rows) columns_to_rows(cols.data(), c.col_stride, c.count, T, rows);
    return ECC_OK;
}
template <class V>
int column_call_finish(ecc_metric* m, const ColumnCall& c, int S, double* totals, int T, const V* cols_d, V* rows)
{
    return column_call_finish(m, c, S, totals, T, cols_d, rows, no_more);
}

}  // namespace ecc_internal

#endif
