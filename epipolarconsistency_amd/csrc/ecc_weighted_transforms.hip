// ecc_weighted_transforms.hip -- the metric with per-line weights (ecc_weighted.hip, weighted_kernel.hip) for the registration of two
// scans (ecc_transforms.hip; ref: tools/Registration/Registration3D3D.hxx:56-62, :91-110).  Host code; include/ecc_hip.h states the
// contract.  A truncated second scan, a table edge that one scan sees, an instrument present in one acquisition break exactly the
// lines that cross them, in every cross pair of that view; the caller flags those lines in the view's weight intermediate.
//
// ecc_metric_evaluate_weighted_transforms, per batch of K transforms:
//   transform_list  ecc_transforms.hip's launch, unchanged: P_i T_k and E1 of the n + K n_source extended matrices, the index grid
//                   pair-major and transform-minor (ecc_transform_grid.h), entry (n + k n_source + i, n_source + j, i, n_source + j):
//                   the DATA indices stay i and n_source + j, so the weights of a sample come from dtr n_views + D whatever the
//                   extended matrix index is (its value slots are written and not read: the weighted pair launch has none)
//   k01_kernel      over the grid into the pose batch's records -- k01_radii_kernel under the automatic object radius
//   weighted pairs  ecc_launch_pairs_weighted over it, EccPairParams::n_views staying n; column col of entry e at col * stride + e
//   sum             sum_weighted_transforms_kernel: per transform both column sums in the order of ecc_sum_order.h for `count`
//                   values, read K floats apart -> 2 K pinned result words the host polls
//   host            values[k] = sum c / sum u, coverages[k] = sum u / count; the pair terms: one copy of both columns and the
//                   transposition to transform-major rows
// Every value, coverage and pair term has the bits of ecc_metric_set_projections(composed matrices) +
// ecc_metric_evaluate_weighted_pairs(the cross list) (tests/test_gpu_weighted_transforms.py).  What the batch does not take is
// evaluated that way inside the call.  Nothing of the metric's own state is written; the scratch is the pose batch's.
// Not here: the full-matrices and strided pose forms of the weighted metric; kept base columns; range, group and RCCL forms.
#include "ecc_capi_internal.h"
#include "ecc_sum_order.h"
#include "ecc_transform_grid.h"

using namespace ecc_internal;

namespace {

// transforms per batch: they are the y dimension of the sum's grid
constexpr int64_t WEIGHTED_TRANSFORM_BATCH_MAX = 32768;
static_assert(WEIGHTED_TRANSFORM_BATCH_MAX < 65536, "transforms are the y dimension of sum_weighted_transforms_kernel's grid");

// One batch: K transforms Ts (16 doubles each) of the base matrices (n x 12).  sums[2 k], sums[2 k + 1]: sum c and sum u of
// transform k over its cross list; pair_terms (nullable, host): K x count rows {c, u}.
int run_batch(ecc_metric* m, const double* base, int n_source, int K, const double* Ts, double* sums, float* pair_terms)
{
    ecc_ctx* ctx = m->ctx;
    const int64_t n = m->n_views, count = (int64_t)n_source * (n - n_source), entries = count * K;
    const int64_t vals_stride = (entries + 3) & ~(int64_t)3;
    volatile uint64_t* out = nullptr;
    double* out_dev = nullptr;
    int rc = stage_transform_grid(m, base, n_source, K, Ts, 2 * K, &out, &out_dev);
    if (!rc) rc = m->pose_values_d.ensure(2 * vals_stride, ctx->stream);
    if (!rc) rc = m->pose_partial_d.ensure((int64_t)2 * K * ecc_sum::SLICES, ctx->stream);
    if (rc) return rc;
    EccPairParams p;
    rc = fill_pair_params(m, &p, count, /*need_e1=*/false);  // the sampling mode of a list of `count` tuples
    if (rc) return rc;
    HIP_TRY(launch_transform_list(m, n_source, K, (long long)((count + 3) & ~(int64_t)3), 2 * K));
    p.PinvTs = m->pose_PinvTs_d.ptr;
    p.Cs = m->pose_Cs_d.ptr;
    p.indices = m->pose_idx_d.ptr;
    p.records = m->pose_records_d.ptr;
    p.first = 0;
    p.count = entries;
    if (m->object_radius_mm > 0) HIP_TRY(ecc_launch_k01(&p, ctx->stream));
    else HIP_TRY(ecc_launch_k01_radii(&p, m->transform_radii_d.ptr, K, ctx->stream));  // every transform the radius of its composed view 0
    EccWeightedParams g;  // (p.n_views stays n: the weight copy of data copy D is n copies behind it)
    set_channel_strides(m, &g);
    g.values = m->pose_values_d.ptr;
    g.col_stride = vals_stride;
    HIP_TRY(launch_weighted_timed(ctx, &p, &g));
    arm_pose_results(out, 2 * K);
    const int slices = ecc_sum::slices(count, m->sum_scratch_d.ptr != nullptr);  // ecc_metric_evaluate_weighted_pairs' choice
    HIP_TRY(ecc_launch_sum_weighted_transforms(m->pose_values_d.ptr, vals_stride, count, K, slices, m->pose_partial_d.ptr, out_dev, ctx->stream));
    std::vector<float> cols;
    if (pair_terms) {
        cols.resize(2 * (size_t)vals_stride);
        HIP_TRY(hipMemcpyAsync(cols.data(), m->pose_values_d.ptr, sizeof(float) * cols.size(), hipMemcpyDeviceToHost, ctx->stream));
    }
    rc = wait_pose_results(ctx, out, 2 * K, sums);
    if (rc || !pair_terms) return rc;
    HIP_TRY(wait_stream_spin(ctx->stream));  // the copy behind the sums
    for (int k = 0; k < K; ++k)
        for (int64_t q = 0; q < count; ++q)
            for (int u = 0; u < 2; ++u)
                pair_terms[2 * ((size_t)k * count + q) + u] = ecc_transform_grid::value(cols.data() + (size_t)u * vals_stride, q, k, K);
    return ECC_OK;
}

}  // namespace

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
    m->last_batched_transforms = 0;
    if (n_transforms == 0) return ECC_OK;
    rc = set_device(m->ctx);
    if (rc) return rc;
    const int64_t n = m->n_views, count = (int64_t)n_source * (n - n_source);
    const double* Pcur = m->Ps_h[m->set_generation & 1].host;
    const std::vector<double> base(Pcur, Pcur + 12 * n);
    if (!m->pose_batching || count > ECC_POSE_BATCH_MAX_ENTRIES)
        return transforms_sequential(m, base, n_source, n_transforms, Ts, [&](int k, const int32_t* idx, int len) {
            return ecc_metric_evaluate_weighted_pairs(m, idx, len, &values[k], coverages ? &coverages[k] : nullptr,
                                                      pair_terms ? pair_terms + 2 * (size_t)k * count : nullptr);
        });
    std::vector<double> sums;
    return transforms_batched(m, count, n_transforms, WEIGHTED_TRANSFORM_BATCH_MAX, [&](int64_t k0, int K) -> int {
        sums.resize(2 * (size_t)K);
        const int e = run_batch(m, base.data(), n_source, K, Ts + 16 * (size_t)k0, sums.data(), pair_terms ? pair_terms + 2 * (size_t)k0 * count : nullptr);
        if (e) return e;
        for (int k = 0; k < K; ++k) finish_weighted(sums[2 * k], sums[2 * k + 1], count, &values[k0 + k], coverages ? &coverages[k0 + k] : nullptr);
        return ECC_OK;
    });
}
