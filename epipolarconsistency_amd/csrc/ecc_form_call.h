// ecc_form_call.h -- the host side of the weighted, robust and weighted-robust call families, once.  The three
// forms are column-form calls (ecc_column_call.h) whose pair kernels differ in what they store per pair; what a call does around
// its pair launch does not depend on the form.  A PairForm says what does: how many columns the pair launch stores, how many of
// them are summed, how to launch the pair kernel into a column buffer, how totals become the caller's results.  weighted_form
// (ecc_weighted.hip), robust_form (ecc_robust.hip), weighted_robust_form (ecc_weighted_robust.hip), variance_form
// (ecc_variance.hip) and variance_robust_form (ecc_variance_robust.hip) build one from a call's arguments; the drivers below are
// written over it and never ask which form it is.
//
// form_call          all pairs of the current matrices, or an index list: E1 (if the device geometry is behind the matrices),
//                    k01_kernel into the Gram family's records (column_call_begin), the form's pair launch (form_columns),
//                    sum_gram_kernel over the S leading columns, the copies, the one wait (column_call_finish), the form's division.
//                    The metric's kept records, kept values and pose-batch values are not touched (a list stages its tuples in the
//                    pose batch's index scratch).
// form_pose_deltas   K poses that each replace a few views of the current matrices (the lists of ecc_metric_evaluate_pose_deltas):
//   base columns     all pairs at the current matrices (form_columns: the all-pairs call's own launches), once per call -- or, under
//                    ecc_metric_set_form_incremental, kept between calls in the metric's own buffer and refreshed for the pairs of the
//                    views that changed since (form_base_kept, ecc_form_base.h)
//   per batch        (which poses: ecc_pose_batches.h) pose_list_kernel (index grid, E1 of the extended matrices), k01_kernel over
//                    the n x Q grid into the pose batch's records, the form's pair launch over it with the base's parameters (the
//                    sampling mode and wave split of an all-pairs evaluation; EccPairParams::n_views stays n: the weight copy of data
//                    copy iD is n copies behind it) into T columns of pose_values_d, sum_weighted_poses_kernel: per pose the sums of
//                    columns 0 and 1 over all pairs, the pose's own entries substituted, in the order of ecc_sum_order.h -> 2 K
//                    pinned result words the host polls; the form's division per pose
//   the rest         what the batch does not take: the pose's matrices, the form's all-pairs call, the matrices back
// form_transforms    K transforms of the source views (ecc_metric_evaluate_transforms' views and cross list), per batch:
//                    transform_list_kernel (ecc_transforms.hip's launch, unchanged: the DATA indices of an entry stay i and
//                    n_source + j whatever its extended matrix index is; its value slots are written and not read: these pair
//                    launches have none), k01_kernel (k01_radii_kernel under the automatic object radius) over the pair-major,
//                    transform-minor grid (ecc_transform_grid.h), the form's pair launch under the mode of a list of `count` tuples,
//                    sum_weighted_transforms_kernel over columns 0 and 1 -> 2 K result words; the pair terms: one copy of the T
//                    columns and the transposition to transform-major rows; with batching off or a list longer than a batch the
//                    transforms one at a time through the form's list call
// The segmented sums read the S leading columns of a column-form buffer and know nothing of what the columns mean: S == 2 goes
// through sum_weighted_poses_kernel / sum_weighted_transforms_kernel as above, whatever the form's T; S == 3 (the weighted-robust
// and the variance-robust form) through sum_form_poses_kernel / sum_form_transforms_kernel (form_sums_kernel.hip), which take all S columns in one walk ->
// S K result words, word S k + col.
#ifndef ECC_FORM_CALL_H
#define ECC_FORM_CALL_H

#include "ecc_column_call.h"
#include "ecc_pose_batches.h"
#include "ecc_transform_grid.h"

namespace ecc_internal {

struct PairForm {
    int T;  // columns the pair launch stores per pair
    int S;  // leading columns that are summed
    // the form's pair kernel over p into T columns at `values`, col_stride apart, between the context's timing events
    std::function<hipError_t(ecc_metric* m, const EccPairParams& p, float* values, int64_t col_stride)> launch;
    // result k of the call from the totals of the summed columns over `count` pairs
    std::function<void(const double* totals, int64_t count, int64_t k)> finish;
    // which form it is and the parameters its columns depend on, for the key of kept base columns alone (ecc_form_base.h): the
    // drivers still never ask
    int kind = ecc_form_base::NONE;
    int loss = 0;
    float delta = 0.f, floor = 0.f;
};

// ecc_weighted.hip: T = S = 2, columns {c, u}; values[k] = sum c / sum u, coverages[k] (coverages nullable) = sum u / count
PairForm weighted_form(double* values, double* coverages);
// ecc_robust.hip: T = 3, S = 2, columns {c, u, r}; values[k] = sum c / count, inlier_masses[k] (nullable) = sum u / count
PairForm robust_form(int loss, float delta, double* values, double* inlier_masses);
// ecc_weighted_robust.hip: T = 4, S = 3, columns {c, u, k, r}; values[k] = sum c / sum u, coverages[k] (nullable) = sum u / count,
// inlier_masses[k] (nullable) = sum k / sum u
PairForm weighted_robust_form(int loss, float delta, double* values, double* coverages, double* inlier_masses);
// ecc_variance.hip: T = S = 2, columns {c, u}; values[k] = sum c / sum u, mean_weights[k] (nullable) = sum u / count
PairForm variance_form(float floor, double* values, double* mean_weights);
// ecc_variance_robust.hip: T = 4, S = 3, columns {c, u, k, r}; values[k] = sum c / sum u, mean_weights[k] (nullable) = sum u / count,
// inlier_masses[k] (nullable) = sum k / sum u
PairForm variance_robust_form(int loss, float delta, float floor, double* values, double* mean_weights, double* inlier_masses);

// poses per batch: the two-column sum's grid is slices x poses x 2 columns, half a million workgroups at most (the S-column sum has
// no z dimension and takes the same limit)
constexpr size_t FORM_BATCH_MAX_POSES = (1 << 19) / (2 * ecc_sum::SLICES);
static_assert(FORM_BATCH_MAX_POSES < 65536, "poses are the y dimension of sum_weighted_poses_kernel's grid");
// transforms per batch: they are the y dimension of the sum's grid
constexpr int64_t FORM_TRANSFORM_BATCH_MAX = 32768;
static_assert(FORM_TRANSFORM_BATCH_MAX < 65536, "transforms are the y dimension of sum_weighted_transforms_kernel's grid");

// The (P0, P1, D0, D1) tuples of an index list: P index the current matrices, in [0, nP), D the intermediates, in [0, nD).
inline int check_index_list(const int32_t* idx4, int n_pairs, int nP, int nD, const char* message)
{
    for (int q = 0; q < n_pairs; ++q) {
        const int32_t* t = idx4 + 4 * (size_t)q;
        if (t[0] < 0 || t[0] >= nP || t[1] < 0 || t[1] >= nP || t[2] < 0 || t[2] >= nD || t[3] < 0 || t[3] >= nD)
            return fail(ECC_ERR_INVALID_ARGUMENT, message);
    }
    return ECC_OK;
}

// k x the median of rms (even count: the mean of the two middle values); 0.0 with no entry.
inline double scaled_median(std::vector<double>& rms, double k)
{
    if (rms.empty()) return 0.0;
    std::sort(rms.begin(), rms.end());
    const size_t h = rms.size() / 2;
    return k * (rms.size() & 1 ? rms[h] : (rms[h - 1] + rms[h]) / 2.0);
}

// The form's columns of `count` pairs -- all pairs (idx4 null) or the list -- under the sampling mode of that many values: a call
// up to and including its pair launch.  The T columns are in m->gram_values_d, c->col_stride apart, once the stream gets there;
// c->p is the record launch as it was made (the pose batches launch their grids with the same parameters).
inline int form_columns(ecc_metric* m, const PairForm& f, const int32_t* idx4, int64_t count, ColumnCall* c)
{
    const int rc = column_call_begin(m, idx4, count, f.T, f.S, c);
    if (rc) return rc;
    HIP_TRY(f.launch(m, c->p, m->gram_values_d.ptr, c->col_stride));
    return ECC_OK;
}

// Everything behind the checks: result 0 of the form over `count` pairs; pair_terms (nullable, host): count x T rows.
inline int form_call(ecc_metric* m, const PairForm& f, const int32_t* idx4, int64_t count, float* pair_terms)
{
    ColumnCall c;
    int rc = form_columns(m, f, idx4, count, &c);
    if (rc) return rc;
    std::vector<double> totals((size_t)f.S);  // in the order an evaluation of `count` values is added in (ecc_sum_order.h)
    rc = column_call_finish(m, c, f.S, totals.data(), f.T, m->gram_values_d.ptr, pair_terms);
    if (rc) return rc;
    f.finish(totals.data(), count, 0);
    return ECC_OK;
}
inline int form_call_all_pairs(ecc_metric* m, const PairForm& f, float* pair_terms)
{
    const int64_t n = m->n_views;
    return form_call(m, f, nullptr, n * (n - 1) / 2, pair_terms);
}

// A pose grid up to and including its pair launch: poses with off[0] = 0 ... off[K] = Q columns over the base matrices `base`, under
// the parameters base_p of the base's record launch.  The grid's T columns are in m->pose_values_d, *vals_stride apart, once the
// stream gets there; `words` result words (none: 0) are reserved in the pinned block, *out / *out_dev their addresses.
inline int form_pose_grid(ecc_metric* m, const PairForm& f, const double* base, const EccPairParams& base_p, int K, const int32_t* off,
                          const int32_t* views, const double* moved_Ps, int words, volatile uint64_t** out, double** out_dev,
                          int64_t* vals_stride)
{
    ecc_ctx* ctx = m->ctx;
    const int64_t n = m->n_views;
    const int Q = off[K];
    const int64_t entries = n * (int64_t)Q;
    *vals_stride = (std::max<int64_t>(entries, 1) + 3) & ~(int64_t)3;
    int rc = stage_pose_grid(m, base, K, off, views, moved_Ps, words, out, out_dev);
    if (!rc) rc = m->pose_values_d.ensure(f.T * *vals_stride, ctx->stream);
    if (!rc && words > 0) rc = m->pose_partial_d.ensure((int64_t)words * ecc_sum::SLICES, ctx->stream);
    if (rc) return rc;
    HIP_TRY(launch_pose_list(m, K, Q, words));
    if (entries > 0) {
        EccPairParams p = base_p;  // the sampling mode of an all-pairs evaluation; n_views stays n
        p.PinvTs = m->pose_PinvTs_d.ptr;
        p.Cs = m->pose_Cs_d.ptr;
        p.indices = m->pose_idx_d.ptr;
        p.records = m->pose_records_d.ptr;
        p.first = 0;
        p.count = entries;
        HIP_TRY(ecc_launch_k01(&p, ctx->stream));
        HIP_TRY(f.launch(m, p, m->pose_values_d.ptr, *vals_stride));
    }
    return ECC_OK;
}

// One batch: poses with off[0] = 0 ... off[K] = Q columns over the base matrices `base`, whose columns are at base_cols --
// m->gram_values_d, or the kept columns of ecc_metric_set_form_incremental -- base_c.col_stride apart.  sums[S k + col], S = f.S:
// the sum of column col of pose k over all pairs.
inline int form_pose_batch(ecc_metric* m, const PairForm& f, const double* base, const ColumnCall& base_c, const float* base_cols, int K,
                           const int32_t* off, const int32_t* views, const double* moved_Ps, double* sums)
{
    ecc_ctx* ctx = m->ctx;
    const int64_t n = m->n_views, n_pairs = n * (n - 1) / 2;
    const int Q = off[K];
    int64_t vals_stride = 0;
    volatile uint64_t* out = nullptr;
    double* out_dev = nullptr;
    const int words = f.S * K;
    const int rc = form_pose_grid(m, f, base, base_c.p, K, off, views, moved_Ps, words, &out, &out_dev, &vals_stride);
    if (rc) return rc;
    arm_pose_results(out, words);
    const int slices = ecc_sum::slices(n_pairs, m->sum_scratch_d.ptr != nullptr);  // the all-pairs call's choice
    if (f.S == 2)
        HIP_TRY(ecc_launch_sum_weighted_poses(base_cols, base_c.col_stride, n_pairs, (int)n, Q, m->pose_lists_d.ptr, K,
                                              m->pose_values_d.ptr, vals_stride, slices, m->pose_partial_d.ptr, out_dev, ctx->stream));
    else  // all f.S columns in one walk of the pose's entries
        HIP_TRY(ecc_launch_sum_form_poses(base_cols, base_c.col_stride, n_pairs, (int)n, Q, m->pose_lists_d.ptr, K,
                                          m->pose_values_d.ptr, vals_stride, f.S, slices, m->pose_partial_d.ptr, out_dev, ctx->stream));
    return wait_pose_results(ctx, out, words, sums);
}

// What kept base columns of form f under the record launch p belong to, beside the matrices.
inline ecc_form_base::Key form_base_key(const ecc_metric* m, const PairForm& f, const EccPairParams& p)
{
    using ecc_form_base::bits_of;
    ecc_form_base::Key k;
    k.kind = f.kind;
    k.T = f.T;
    k.S = f.S;
    k.loss = f.loss;
    k.delta = bits_of(f.delta);
    k.floor = bits_of(f.floor);
    k.mode = p.reference_arithmetic ? ECC_SAMPLING_REFERENCE : (p.poly ? ECC_SAMPLING_POLYNOMIAL : ECC_SAMPLING_PER_SAMPLE);
    k.radius = bits_of(p.object_radius_mm);  // the radius the launch resolved: the automatic one follows view 0
    k.dkappa = bits_of(p.dkappa_user);
    k.tol = bits_of(p.economise_tol);
    k.use_corr = p.use_corr;
    k.n_views = m->n_views;
    k.n_dtrs = (int)m->dtrs.size();
    return k;
}

// The base columns of a pose-delta call under ecc_metric_set_form_incremental: in m->form_base_d, c->col_stride
// apart, once the stream gets there; c->p as form_columns leaves it.  ecc_form_base::decide says what is evaluated:
//   miss      form_columns' launches, into the kept buffer; the key and the matrices are taken (never under ECC_SAMPLING_REFERENCE)
//   hit       nothing; E1 if the device geometry is behind the matrices, as every column call makes sure
//   refresh   ONE pose grid -- the changed views at their current matrices over the current matrices, form_pose_grid -- and
//             form_base_scatter_kernel from its T columns into the kept ones; the changed views' matrices are taken
// The kept columns are invalid while they are rewritten and valid once everything is queued, as evaluate_cached keeps cache.valid.
inline int form_base_kept(ecc_metric* m, const PairForm& f, const double* Pcur, ColumnCall* c)
{
    namespace fb = ecc_form_base;
    ecc_ctx* ctx = m->ctx;
    const int64_t n = m->n_views, n_pairs = n * (n - 1) / 2;
    int rc = set_device(ctx);
    if (rc) return rc;
    c->count = n_pairs;
    c->col_stride = (n_pairs + 3) & ~(int64_t)3;
    if (!m->quads_decided && n_pairs >= 32768) decide_quad_copies(m);  // (as column_call_begin: in front of the parameters)
    rc = fill_pair_params(m, &c->p, n_pairs, /*need_e1=*/false);
    if (rc) return rc;
    const fb::Key key = form_base_key(m, f, c->p);
    std::vector<int> changed;
    std::vector<int32_t> views;
    std::vector<double> moved;
    const fb::Decision d = fb::decide(
        m->form_base.valid, m->form_base.key, m->form_base.Ps.data(), key, Pcur, fb::limit(n),
        [&](const std::vector<int>& ch) {
            views.assign(ch.begin(), ch.end());
            moved.resize(12 * ch.size());
            for (size_t a = 0; a < ch.size(); ++a) std::memcpy(&moved[12 * a], Pcur + 12 * (size_t)ch[a], sizeof(double) * 12);
            float kept_radius;
            std::memcpy(&kept_radius, &m->form_base.key.radius, sizeof(kept_radius));
            return pose_keeps_radius(m, (double)kept_radius, (int)ch.size(), views.data(), moved.data());
        },
        &changed);
    m->form_base.valid = false;  // until everything below is queued
    m->last_form_base_pairs = fb::base_pairs(d, n, (int64_t)changed.size());
    if (d == fb::MISS) {
        rc = column_call_begin(m, nullptr, n_pairs, /*T=*/0, f.S, c, [&] { return m->form_base_d.ensure((int64_t)f.T * c->col_stride, ctx->stream); }, no_more);
        if (rc) return rc;
        HIP_TRY(f.launch(m, c->p, m->form_base_d.ptr, c->col_stride));
        if (fb::may_keep(key)) {
            m->form_base.take(0, n_pairs, (int)n, key, Pcur);
            m->form_base.valid = true;
        }
        return ECC_OK;
    }
    c->p.first = 0;
    c->p.count = n_pairs;
    rc = ensure_e1(m);
    if (rc) return rc;
    if (d == fb::REFRESH) {
        const int cv = (int)changed.size();
        const int32_t off[2] = {0, cv};
        int64_t vals_stride = 0;
        volatile uint64_t* out = nullptr;
        double* out_dev = nullptr;
        rc = form_pose_grid(m, f, Pcur, c->p, 1, off, views.data(), moved.data(), /*words=*/0, &out, &out_dev, &vals_stride);
        if (rc) return rc;
        // (the changed views on the device: pose_list_kernel's copy of the lists, behind the two offsets of the one pose)
        HIP_TRY(ecc_launch_form_base_scatter(m->pose_values_d.ptr, vals_stride, (int)n, cv, m->pose_lists_d.ptr + 2, f.T, m->form_base_d.ptr,
                                             c->col_stride, ctx->stream));
        HIP_TRY(wait_stream_spin(ctx->stream));  // the call's first batch writes its own grid into the pinned block this one was read from
        m->form_base.update(changed, Pcur);
    }
    m->form_base.valid = true;
    return ECC_OK;
}

// The batched poses of a call; what the batch does not take goes into not_batched.
inline int form_pose_deltas_batched(ecc_metric* m, const PairForm& f, int n_poses, const int32_t* off, const int32_t* views,
                                    const double* moved_Ps, std::vector<int>* not_batched)
{
    ecc_ctx* ctx = m->ctx;
    const int64_t n = m->n_views, n_pairs = n * (n - 1) / 2;
    ecc_mark_busy(m);
    const double* Pcur = m->Ps_h[m->set_generation & 1].host;
    const std::vector<double> base(Pcur, Pcur + 12 * n);
    double base_radius = 0.0;
    ecc_metric_get_object_radius(m, &base_radius);
    ColumnCall base_c;
    int rc;
    if (m->form_incremental) rc = form_base_kept(m, f, base.data(), &base_c);
    else {
        rc = form_columns(m, f, nullptr, n_pairs, &base_c);  // once per call
        m->last_form_base_pairs = n_pairs;
    }
    if (rc) return rc;
    const float* base_cols = m->form_incremental ? m->form_base_d.ptr : m->gram_values_d.ptr;
    std::vector<double> sums;
    const int64_t max_cols = std::max<int64_t>(ECC_POSE_BATCH_MAX_ENTRIES / n, ECC_POSE_BATCH_MAX_MOVED);
    rc = ecc_pose_batches::pack(
        n_poses, off, views, moved_Ps, max_cols, FORM_BATCH_MAX_POSES,
        [&](int c, const int32_t* vk, const double* Pk) { return pose_keeps_radius(m, base_radius, c, vk, Pk); },
        [&](const ecc_pose_batches::Batch& b) -> int {
            sums.resize(f.S * b.pose.size());
            const int e = form_pose_batch(m, f, base.data(), base_c, base_cols, (int)b.pose.size(), b.off.data(), b.views.data(), b.Ps.data(),
                                          sums.data());
            if (e) return e;
            for (size_t q = 0; q < b.pose.size(); ++q) f.finish(&sums[f.S * q], n_pairs, b.pose[q]);
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

// Everything of a pose-delta call behind its checks.  evaluate_pose(k): the form's all-pairs call for result k, at the current
// matrices.
inline int form_pose_deltas(ecc_metric* m, const PairForm& f, int n_poses, const int32_t* off, const int32_t* views, const double* moved_Ps,
                            const std::function<int(int)>& evaluate_pose)
{
    int rc = set_device(m->ctx);
    if (rc) return rc;
    m->last_batched_poses = 0;
    m->last_form_base_pairs = 0;  // (with batching off the call computes no base columns)
    std::vector<int> rest;
    if (m->pose_batching) {
        rc = form_pose_deltas_batched(m, f, n_poses, off, views, moved_Ps, &rest);
        if (rc) return rc;
    } else {
        for (int k = 0; k < n_poses; ++k) rest.push_back(k);
    }
    return pose_deltas_sequential(m, rest, off, views, moved_Ps, evaluate_pose);
}

// One batch: K transforms Ts (16 doubles each) of the base matrices (n x 12).  sums[S k + col], S = f.S: the sum of column col of
// transform k over its cross list; pair_terms (nullable, host): K x count rows of T.  batch_noun: wait_pose_results' word for the
// batch.
inline int form_transform_batch(ecc_metric* m, const PairForm& f, const double* base, int n_source, int K, const double* Ts,
                                const char* batch_noun, double* sums, float* pair_terms)
{
    ecc_ctx* ctx = m->ctx;
    const int T = f.T, words = f.S * K;
    const int64_t n = m->n_views, count = (int64_t)n_source * (n - n_source), entries = count * K;
    const int64_t vals_stride = (entries + 3) & ~(int64_t)3;
    volatile uint64_t* out = nullptr;
    double* out_dev = nullptr;
    int rc = stage_transform_grid(m, base, n_source, K, Ts, words, &out, &out_dev);
    if (!rc) rc = m->pose_values_d.ensure(T * vals_stride, ctx->stream);
    if (!rc) rc = m->pose_partial_d.ensure((int64_t)words * ecc_sum::SLICES, ctx->stream);
    if (rc) return rc;
    EccPairParams p;
    rc = fill_pair_params(m, &p, count, /*need_e1=*/false);  // the sampling mode of a list of `count` tuples
    if (rc) return rc;
    HIP_TRY(launch_transform_list(m, n_source, K, (long long)((count + 3) & ~(int64_t)3), words));
    p.PinvTs = m->pose_PinvTs_d.ptr;
    p.Cs = m->pose_Cs_d.ptr;
    p.indices = m->pose_idx_d.ptr;
    p.records = m->pose_records_d.ptr;
    p.first = 0;
    p.count = entries;
    if (m->object_radius_mm > 0) HIP_TRY(ecc_launch_k01(&p, ctx->stream));
    else HIP_TRY(ecc_launch_k01_radii(&p, m->transform_radii_d.ptr, K, ctx->stream));  // every transform the radius of its composed view 0
    HIP_TRY(f.launch(m, p, m->pose_values_d.ptr, vals_stride));  // (p.n_views stays n: the weight copy of data copy D is n copies behind it)
    arm_pose_results(out, words);
    const int slices = ecc_sum::slices(count, m->sum_scratch_d.ptr != nullptr);  // the list call's choice
    if (f.S == 2)
        HIP_TRY(ecc_launch_sum_weighted_transforms(m->pose_values_d.ptr, vals_stride, count, K, slices, m->pose_partial_d.ptr, out_dev, ctx->stream));
    else  // all f.S columns from one set of strided addresses
        HIP_TRY(ecc_launch_sum_form_transforms(m->pose_values_d.ptr, vals_stride, count, K, f.S, slices, m->pose_partial_d.ptr, out_dev, ctx->stream));
    std::vector<float> cols;
    if (pair_terms) {
        cols.resize(T * (size_t)vals_stride);
        HIP_TRY(hipMemcpyAsync(cols.data(), m->pose_values_d.ptr, sizeof(float) * cols.size(), hipMemcpyDeviceToHost, ctx->stream));
    }
    rc = wait_pose_results(ctx, out, words, sums, batch_noun);
    if (rc || !pair_terms) return rc;
    HIP_TRY(wait_stream_spin(ctx->stream));  // the copy behind the sums
    for (int k = 0; k < K; ++k)
        for (int64_t q = 0; q < count; ++q)
            for (int u = 0; u < T; ++u)
                pair_terms[T * ((size_t)k * count + q) + u] = ecc_transform_grid::value(cols.data() + (size_t)u * vals_stride, q, k, K);
    return ECC_OK;
}

// Everything of a transforms call behind its checks.  evaluate_list(k, the cross list, its length, the rows of transform k or
// null): the form's list call for result k, at the current matrices.
inline int form_transforms(ecc_metric* m, const PairForm& f, int n_source, int n_transforms, const double* Ts, float* pair_terms,
                           const char* batch_noun, const std::function<int(int, const int32_t*, int, float*)>& evaluate_list)
{
    m->last_batched_transforms = 0;
    if (n_transforms == 0) return ECC_OK;
    const int rc = set_device(m->ctx);
    if (rc) return rc;
    const int64_t n = m->n_views, count = (int64_t)n_source * (n - n_source);
    const double* Pcur = m->Ps_h[m->set_generation & 1].host;
    const std::vector<double> base(Pcur, Pcur + 12 * n);
    auto rows_of = [&](int64_t k) -> float* { return pair_terms ? pair_terms + f.T * (size_t)k * count : nullptr; };
    if (!m->pose_batching || count > ECC_POSE_BATCH_MAX_ENTRIES)
        return transforms_sequential(m, base, n_source, n_transforms, Ts,
                                     [&](int k, const int32_t* idx, int len) { return evaluate_list(k, idx, len, rows_of(k)); });
    std::vector<double> sums;
    return transforms_batched(m, count, n_transforms, FORM_TRANSFORM_BATCH_MAX, [&](int64_t k0, int K) -> int {
        sums.resize(f.S * (size_t)K);
        const int e = form_transform_batch(m, f, base.data(), n_source, K, Ts + 16 * (size_t)k0, batch_noun, sums.data(), rows_of(k0));
        if (e) return e;
        for (int k = 0; k < K; ++k) f.finish(&sums[f.S * k], count, k0 + k);
        return ECC_OK;
    });
}

}  // namespace ecc_internal

#endif
