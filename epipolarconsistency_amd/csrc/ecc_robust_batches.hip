// ecc_robust_batches.hip -- the metric under a per-sample robust loss (ecc_robust.hip, robust_kernel.hip) for the callers that sit
// in optimiser loops: a population of poses or of source-to-target transforms per call.  Host code only; include/ecc_hip.h states the
// contracts, DESIGN.md 4.22 the launch sequence.  Nothing here is a kernel of its own: the pair launch is ecc_launch_pairs_robust as
// it stands, the segmented sums are those of the weighted siblings (they read columns 0 and 1 of a column-form buffer and know
// nothing of line weights), the grids are ecc_poses.hip's and ecc_transforms.hip's.
//
// ecc_metric_evaluate_robust_pose_deltas  K poses that each replace a few views of the current matrices (the lists of
//                                         ecc_metric_evaluate_pose_deltas):
//   base columns   {c, u, r} of all pairs at the current matrices (robust_base_columns: ecc_metric_evaluate_robust's own launches),
//                  recomputed on every call
//   per batch      (which poses: ecc_pose_batches.h) pose_list_kernel (index grid, E1 of the extended matrices), k01_kernel over
//                  the n x Q grid into the pose batch's records, the robust pair launch over it with the base's parameters (the
//                  sampling mode and wave split of an all-pairs evaluation) into three columns of pose_values_d,
//                  sum_weighted_poses_kernel over columns 0 and 1 -> 2 K pinned result words the host polls
//   host           values[k] = sum c / n_pairs, inlier_masses[k] = sum u / n_pairs
// ecc_metric_evaluate_robust_transforms   K transforms of the source views (ecc_metric_evaluate_transforms' views and cross list), per batch:
//   transform_list ecc_transforms.hip's launch; k01_kernel (k01_radii_kernel under the automatic object radius) over the pair-major,
//                  transform-minor grid; the robust pair launch under the mode of a list of `count` tuples;
//                  sum_weighted_transforms_kernel over columns 0 and 1; the pair terms: one copy of the three columns and the
//                  transposition to transform-major rows
//   host           values[k] = sum c / count, inlier_masses[k] = sum u / count
// Every result has the bits of the sequential calls (tests/test_gpu_robust_poses.py, tests/test_gpu_robust_transforms.py); what a
// batch does not take is evaluated that way inside the call.
// Not here: base columns kept between calls; the full-matrices and strided pose forms; range, group and RCCL forms; these batches
// for the loss combined with line weights (ecc_weighted_robust.hip has its all-pairs and list forms); the loss under use_corr.
#include "ecc_column_call.h"
#include "ecc_pose_batches.h"
#include "ecc_transform_grid.h"

using namespace ecc_internal;

namespace {

constexpr int T = 3;  // columns of the pair launch: c, u, r; the sums read c and u
// poses / transforms per batch: the y dimension of the sums' grids (the bounds ecc_launch_sum_weighted_poses / _transforms check)
constexpr size_t ROBUST_BATCH_MAX_POSES = (1 << 19) / (2 * ecc_sum::SLICES);
constexpr int64_t ROBUST_TRANSFORM_BATCH_MAX = 32768;

// a mean over the pairs, as ecc_metric_evaluate_robust forms it -- NOT divided by the inlier mass
void finish_robust(double sum_c, double sum_u, int64_t count, double* value, double* inlier_mass)
{
    *value = sum_c / (double)count;
    if (inlier_mass) *inlier_mass = sum_u / (double)count;
}

// One batch: poses with off[0] = 0 ... off[K] = Q columns over the base matrices `base`, whose columns are in m->gram_values_d
// (base_g).  sums[2 k], sums[2 k + 1]: sum c and sum u of pose k over all pairs.
int run_pose_batch(ecc_metric* m, const double* base, const EccPairParams& base_p, const EccRobustParams& base_g, int K, const int32_t* off,
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
    if (!rc) rc = m->pose_values_d.ensure(T * vals_stride, ctx->stream);
    if (!rc) rc = m->pose_partial_d.ensure((int64_t)2 * K * ecc_sum::SLICES, ctx->stream);
    if (rc) return rc;
    HIP_TRY(launch_pose_list(m, K, Q, 2 * K));
    if (entries > 0) {
        EccPairParams p = base_p;  // the sampling mode of an all-pairs evaluation
        p.PinvTs = m->pose_PinvTs_d.ptr;
        p.Cs = m->pose_Cs_d.ptr;
        p.indices = m->pose_idx_d.ptr;
        p.records = m->pose_records_d.ptr;
        p.first = 0;
        p.count = entries;
        HIP_TRY(ecc_launch_k01(&p, ctx->stream));
        EccRobustParams g = base_g;
        g.values = m->pose_values_d.ptr;
        g.col_stride = vals_stride;
        HIP_TRY(launch_robust_timed(ctx, &p, &g));
    }
    arm_pose_results(out, 2 * K);
    const int slices = ecc_sum::slices(n_pairs, m->sum_scratch_d.ptr != nullptr);  // ecc_metric_evaluate_robust's choice
    HIP_TRY(ecc_launch_sum_weighted_poses(base_g.values, base_g.col_stride, n_pairs, (int)n, Q, m->pose_lists_d.ptr, K, m->pose_values_d.ptr,
                                          vals_stride, slices, m->pose_partial_d.ptr, out_dev, ctx->stream));
    return wait_pose_results(ctx, out, 2 * K, sums);
}

// The batched poses of a call; what the batch does not take goes into not_batched.
int robust_deltas(ecc_metric* m, int n_poses, const int32_t* off, const int32_t* views, const double* moved_Ps, int loss, float delta,
                  double* values, double* inlier_masses, std::vector<int>* not_batched)
{
    ecc_ctx* ctx = m->ctx;
    const int64_t n = m->n_views, n_pairs = n * (n - 1) / 2;
    ecc_mark_busy(m);
    const double* Pcur = m->Ps_h[m->set_generation & 1].host;
    const std::vector<double> base(Pcur, Pcur + 12 * n);
    double base_radius = 0.0;
    ecc_metric_get_object_radius(m, &base_radius);
    ColumnCall base_c;
    EccRobustParams base_g;
    int rc = robust_base_columns(m, loss, delta, &base_c, &base_g);  // once per call
    if (rc) return rc;
    std::vector<double> sums;
    const int64_t max_cols = std::max<int64_t>(ECC_POSE_BATCH_MAX_ENTRIES / n, ECC_POSE_BATCH_MAX_MOVED);
    rc = ecc_pose_batches::pack(
        n_poses, off, views, moved_Ps, max_cols, ROBUST_BATCH_MAX_POSES,
        [&](int c, const int32_t* vk, const double* Pk) { return pose_keeps_radius(m, base_radius, c, vk, Pk); },
        [&](const ecc_pose_batches::Batch& b) -> int {
            sums.resize(2 * b.pose.size());
            const int e = run_pose_batch(m, base.data(), base_c.p, base_g, (int)b.pose.size(), b.off.data(), b.views.data(), b.Ps.data(), sums.data());
            if (e) return e;
            for (size_t q = 0; q < b.pose.size(); ++q)
                finish_robust(sums[2 * q], sums[2 * q + 1], n_pairs, &values[b.pose[q]], inlier_masses ? &inlier_masses[b.pose[q]] : nullptr);
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

// One batch: K transforms Ts (16 doubles each) of the base matrices (n x 12).  sums[2 k], sums[2 k + 1]: sum c and sum u of
// transform k over its cross list; pair_terms (nullable, host): K x count rows {c, u, r}.
int run_transform_batch(ecc_metric* m, const double* base, int n_source, int K, const double* Ts, int loss, float delta, double* sums,
                        float* pair_terms)
{
    ecc_ctx* ctx = m->ctx;
    const int64_t n = m->n_views, count = (int64_t)n_source * (n - n_source), entries = count * K;
    const int64_t vals_stride = (entries + 3) & ~(int64_t)3;
    volatile uint64_t* out = nullptr;
    double* out_dev = nullptr;
    int rc = stage_transform_grid(m, base, n_source, K, Ts, 2 * K, &out, &out_dev);
    if (!rc) rc = m->pose_values_d.ensure(T * vals_stride, ctx->stream);
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
    EccRobustParams g;  // (the grid's value slots are written and not read: the robust pair launch has none)
    fill_robust_params(&g, m->pose_values_d.ptr, vals_stride, loss, delta);
    HIP_TRY(launch_robust_timed(ctx, &p, &g));
    arm_pose_results(out, 2 * K);
    const int slices = ecc_sum::slices(count, m->sum_scratch_d.ptr != nullptr);  // ecc_metric_evaluate_robust_pairs' choice
    HIP_TRY(ecc_launch_sum_weighted_transforms(m->pose_values_d.ptr, vals_stride, count, K, slices, m->pose_partial_d.ptr, out_dev, ctx->stream));
    std::vector<float> cols;
    if (pair_terms) {
        cols.resize(T * (size_t)vals_stride);
        HIP_TRY(hipMemcpyAsync(cols.data(), m->pose_values_d.ptr, sizeof(float) * cols.size(), hipMemcpyDeviceToHost, ctx->stream));
    }
    rc = wait_pose_results(ctx, out, 2 * K, sums, "transform");
    if (rc || !pair_terms) return rc;
    HIP_TRY(wait_stream_spin(ctx->stream));  // the copy behind the sums
    for (int k = 0; k < K; ++k)
        for (int64_t q = 0; q < count; ++q)
            for (int u = 0; u < T; ++u)
                pair_terms[T * ((size_t)k * count + q) + u] = ecc_transform_grid::value(cols.data() + (size_t)u * vals_stride, q, k, K);
    return ECC_OK;
}

}  // namespace

ECC_EXPORT int ecc_metric_evaluate_robust_pose_deltas(ecc_metric* m, int n_poses, const int32_t* moved_offsets, const int32_t* moved_views,
                                                      const double* moved_Ps, int loss, float delta, double* values, double* inlier_masses)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!moved_offsets || !values) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    if (n_poses < 1) return ECC_OK;
    if (moved_offsets[n_poses] > 0 && (!moved_views || !moved_Ps)) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    int rc = robust_check(m, values, loss, delta);
    if (rc) return rc;
    if ((int64_t)m->dtrs.size() < (int64_t)m->n_views) return fail(ECC_ERR_INVALID_ARGUMENT, "fewer Radon intermediates than projection matrices");
    rc = check_lists(m, n_poses, moved_offsets, moved_views);
    if (rc) return rc;
    rc = set_device(m->ctx);
    if (rc) return rc;
    m->last_batched_poses = 0;
    std::vector<int> rest;
    if (m->pose_batching) {
        rc = robust_deltas(m, n_poses, moved_offsets, moved_views, moved_Ps, loss, delta, values, inlier_masses, &rest);
        if (rc) return rc;
    } else {
        for (int k = 0; k < n_poses; ++k) rest.push_back(k);
    }
    return pose_deltas_sequential(m, rest, moved_offsets, moved_views, moved_Ps, [&](int k) {
        return ecc_metric_evaluate_robust(m, loss, delta, &values[k], inlier_masses ? &inlier_masses[k] : nullptr, nullptr);
    });
}

ECC_EXPORT int ecc_metric_evaluate_robust_transforms(ecc_metric* m, int n_source, int n_transforms, const double* Ts, int loss, float delta,
                                                     double* values, double* inlier_masses, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (n_transforms < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "n_transforms must not be negative");
    if (n_transforms > 0 && (!Ts || !values)) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    double unused = 0.0;  // (n_transforms == 0: values may be null, and nothing is written)
    int rc = robust_check(m, values ? values : &unused, loss, delta);
    if (rc) return rc;
    if ((int64_t)m->dtrs.size() < (int64_t)m->n_views) return fail(ECC_ERR_INVALID_ARGUMENT, "fewer Radon intermediates than projection matrices");
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
            return ecc_metric_evaluate_robust_pairs(m, idx, len, loss, delta, &values[k], inlier_masses ? &inlier_masses[k] : nullptr,
                                                    pair_terms ? pair_terms + T * (size_t)k * count : nullptr);
        });
    std::vector<double> sums;
    return transforms_batched(m, count, n_transforms, ROBUST_TRANSFORM_BATCH_MAX, [&](int64_t k0, int K) -> int {
        sums.resize(2 * (size_t)K);
        const int e = run_transform_batch(m, base.data(), n_source, K, Ts + 16 * (size_t)k0, loss, delta, sums.data(),
                                          pair_terms ? pair_terms + T * (size_t)k0 * count : nullptr);
        if (e) return e;
        for (int k = 0; k < K; ++k) finish_robust(sums[2 * k], sums[2 * k + 1], count, &values[k0 + k], inlier_masses ? &inlier_masses[k0 + k] : nullptr);
        return ECC_OK;
    });
}
