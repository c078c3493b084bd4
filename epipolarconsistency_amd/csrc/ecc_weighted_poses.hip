// ecc_weighted_poses.hip -- the metric with per-line weights (ecc_weighted.hip, weighted_kernel.hip) for the callers that have such
// data: pose optimisers.  Host code; include/ecc_hip.h states the contracts.
//
// ecc_metric_evaluate_weighted_pairs        an index list of (P0, P1, D0, D1) tuples: k01_kernel with the list into the Gram family's
//                                           records (column_call_begin, ecc_column_call.h), the weighted pair launch, sum_gram_kernel
//                                           over the two columns, the copies (column_call_finish).
// ecc_metric_evaluate_weighted_pose_deltas  K poses that each replace a few views of the current matrices (the lists of
//                                           ecc_metric_evaluate_pose_deltas, ecc_poses.hip):
//   base columns   {c, u} of all pairs at the current matrices (weighted_base_columns: ecc_metric_evaluate_weighted's own launches),
//                  recomputed on every call
//   per batch      (which poses: ecc_pose_batches.h) pose_list_kernel (index grid, E1 of the extended matrices), k01_kernel over
//                  the n x Q grid into the pose batch's records, the weighted pair launch over it (EccPairParams::n_views stays n:
//                  the weight copy of data copy iD is n copies behind it), sum_weighted_poses_kernel: per pose both column sums over all pairs, the pose's own entries
//                  substituted, in the order of ecc_sum_order.h -> 2 K pinned result words the host polls
//   host           values[k] = sum c / sum u, coverages[k] = sum u / n_pairs
// Every value and coverage has the bits of ecc_metric_set_projections + ecc_metric_evaluate_weighted for that pose
// (tests/test_gpu_weighted_poses.py).  What the batch does not take is evaluated that way inside the call.
// Not here: base columns kept between calls (a stale column is a silently wrong result; keeping them needs change tracking over
// matrices, parameters, sampling mode, quad copies and ecc_metric_refresh_dtrs); the full-matrices, strided, group and RCCL forms;
// an incremental mode for the weighted value; a one-launch small path for weighted lists.
#include "ecc_column_call.h"
#include "ecc_pose_batches.h"

using namespace ecc_internal;

namespace {

// poses per batch: the sum's grid is slices x poses x 2 columns, half a million workgroups at most
constexpr size_t WEIGHTED_BATCH_MAX_POSES = (1 << 19) / (2 * ecc_sum::SLICES);
static_assert(WEIGHTED_BATCH_MAX_POSES < 65536, "poses are the y dimension of sum_weighted_poses_kernel's grid");

// One batch: poses with off[0] = 0 ... off[K] = Q columns over the base matrices `base`, whose two columns are in m->gram_values_d
// (base_g).  sums[2 k], sums[2 k + 1]: sum c and sum u of pose k over all pairs.
int run_weighted_batch(ecc_metric* m, const double* base, const EccPairParams& base_p, const EccWeightedParams& base_g, int K, const int32_t* off,
                       const int32_t* views, const double* moved_Ps, double* sums)
{
    ecc_ctx* ctx = m->ctx;
    const int64_t n = m->n_views, n_pairs = n * (n - 1) / 2;
    const int Q = off[K];
    const int64_t entries = n * (int64_t)Q;
    const int64_t vals_stride = (std::max<int64_t>(entries, 1) + 3) & ~(int64_t)3;
    volatile uint64_t* out = nullptr;
    double* out_dev = nullptr;
    int rc = stage_pose_grid(m, base, K, off, views, moved_Ps, 2 * K, &out, &out_dev);
    if (!rc) rc = m->pose_values_d.ensure(2 * vals_stride, ctx->stream);
    if (!rc) rc = m->pose_partial_d.ensure((int64_t)2 * K * ecc_sum::SLICES, ctx->stream);
    if (rc) return rc;
    HIP_TRY(launch_pose_list(m, K, Q, 2 * K));
    if (entries > 0) {
        EccPairParams p = base_p;  // the sampling mode of an all-pairs evaluation; n_views stays n
        p.PinvTs = m->pose_PinvTs_d.ptr;
        p.Cs = m->pose_Cs_d.ptr;
        p.indices = m->pose_idx_d.ptr;
        p.records = m->pose_records_d.ptr;
        p.first = 0;
        p.count = entries;
        HIP_TRY(ecc_launch_k01(&p, ctx->stream));
        EccWeightedParams g = base_g;
        g.values = m->pose_values_d.ptr;
        g.col_stride = vals_stride;
        HIP_TRY(launch_weighted_timed(ctx, &p, &g));
    }
    arm_pose_results(out, 2 * K);
    const int slices = ecc_sum::slices(n_pairs, m->sum_scratch_d.ptr != nullptr);  // ecc_metric_evaluate_weighted's choice
    HIP_TRY(ecc_launch_sum_weighted_poses(base_g.values, base_g.col_stride, n_pairs, (int)n, Q, m->pose_lists_d.ptr, K, m->pose_values_d.ptr,
                                          vals_stride, slices, m->pose_partial_d.ptr, out_dev, ctx->stream));
    return wait_pose_results(ctx, out, 2 * K, sums);
}

// The batched poses of a call; what the batch does not take goes into not_batched.
int weighted_deltas(ecc_metric* m, int n_poses, const int32_t* off, const int32_t* views, const double* moved_Ps, double* values,
                    double* coverages, std::vector<int>* not_batched)
{
    ecc_ctx* ctx = m->ctx;
    const int64_t n = m->n_views, n_pairs = n * (n - 1) / 2;
    ecc_mark_busy(m);
    const double* Pcur = m->Ps_h[m->set_generation & 1].host;
    const std::vector<double> base(Pcur, Pcur + 12 * n);
    double base_radius = 0.0;
    ecc_metric_get_object_radius(m, &base_radius);
    ColumnCall base_c;
    EccWeightedParams base_g;
    int rc = weighted_base_columns(m, &base_c, &base_g);  // once per call
    if (rc) return rc;
    std::vector<double> sums;
    const int64_t max_cols = std::max<int64_t>(ECC_POSE_BATCH_MAX_ENTRIES / n, ECC_POSE_BATCH_MAX_MOVED);
    rc = ecc_pose_batches::pack(
        n_poses, off, views, moved_Ps, max_cols, WEIGHTED_BATCH_MAX_POSES,
        [&](int c, const int32_t* vk, const double* Pk) { return pose_keeps_radius(m, base_radius, c, vk, Pk); },
        [&](const ecc_pose_batches::Batch& b) -> int {
            sums.resize(2 * b.pose.size());
            const int e = run_weighted_batch(m, base.data(), base_c.p, base_g, (int)b.pose.size(), b.off.data(), b.views.data(), b.Ps.data(), sums.data());
            if (e) return e;
            for (size_t q = 0; q < b.pose.size(); ++q)
                finish_weighted(sums[2 * q], sums[2 * q + 1], n_pairs, &values[b.pose[q]], coverages ? &coverages[b.pose[q]] : nullptr);
            m->last_batched_poses += (int64_t)b.pose.size();
            return ECC_OK;
        },
        not_batched);
    if (rc) return rc;
    HIP_TRY(wait_stream_spin(ctx->stream));  // (the results were seen before the stream's own completion; the scratch is reused)
    m->done_generation = m->set_generation;
    m->quiet = true;
    return ECC_OK;
}

}  // namespace

ECC_EXPORT int ecc_metric_evaluate_weighted_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, double* value, double* coverage, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!value) return fail(ECC_ERR_INVALID_ARGUMENT, "value is null");
    if (n_pairs < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "negative list length");
    if (n_pairs == 0) return ECC_OK;
    if (!idx4) return fail(ECC_ERR_INVALID_ARGUMENT, "index list is null");
    int rc = weighted_check(m);
    if (rc) return rc;
    // P index the current matrices, D the DATA intermediates: the weights of a sample come from dtr n_views + D
    const int nP = m->n_views;
    for (int q = 0; q < n_pairs; ++q) {
        const int32_t* t = idx4 + 4 * (size_t)q;
        if (t[0] < 0 || t[0] >= nP || t[1] < 0 || t[1] >= nP || t[2] < 0 || t[2] >= nP || t[3] < 0 || t[3] >= nP)
            return fail(ECC_ERR_INVALID_ARGUMENT, "index array contains invalid indices (matrices and data intermediates lie in [0, n_views))");
    }
    ColumnCall c;
    rc = column_call_begin(m, idx4, n_pairs, 2, 2, &c);  // columns: c, u; the sampling mode of a list of n_pairs tuples, as ecc_metric_evaluate_pairs
    if (rc) return rc;
    EccWeightedParams g;
    set_channel_strides(m, &g);
    g.values = m->gram_values_d.ptr;
    g.col_stride = c.col_stride;
    HIP_TRY(launch_weighted_timed(m->ctx, &c.p, &g));
    double totals[2];  // both columns in the order a list of n_pairs values is added in (ecc_sum_order.h)
    rc = column_call_finish(m, c, 2, totals, 2, m->gram_values_d.ptr, pair_terms);
    if (rc) return rc;
    finish_weighted(totals[0], totals[1], n_pairs, value, coverage);
    return ECC_OK;
}

ECC_EXPORT int ecc_metric_evaluate_weighted_pose_deltas(ecc_metric* m, int n_poses, const int32_t* moved_offsets, const int32_t* moved_views,
                                                        const double* moved_Ps, double* values, double* coverages)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!moved_offsets || !values) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    if (n_poses < 1) return ECC_OK;
    if (moved_offsets[n_poses] > 0 && (!moved_views || !moved_Ps)) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    int rc = weighted_check(m);
    if (!rc) rc = check_lists(m, n_poses, moved_offsets, moved_views);
    if (rc) return rc;
    rc = set_device(m->ctx);
    if (rc) return rc;
    m->last_batched_poses = 0;
    std::vector<int> rest;
    if (m->pose_batching) {
        rc = weighted_deltas(m, n_poses, moved_offsets, moved_views, moved_Ps, values, coverages, &rest);
        if (rc) return rc;
    } else {
        for (int k = 0; k < n_poses; ++k) rest.push_back(k);
    }
    return pose_deltas_sequential(m, rest, moved_offsets, moved_views, moved_Ps, [&](int k) {
        return ecc_metric_evaluate_weighted(m, &values[k], coverages ? &coverages[k] : nullptr, nullptr);
    });
}
