// ecc_gradient.hip -- the metric and the probes of its central-difference gradient over the pose parameters of ONE view, in one
// call (host code; include/ecc_hip.h states the contract).  ref for the caller: Gui/SingleImageMotion.h:84-90 -- the objective of
// an optimiser that moves one view; its 2 p probes per iterate are p = 6 parameters of the "3D Rigid" model.
//
// The probes are poses of ecc_metric_evaluate_pose_deltas (ecc_poses.hip) that replace the same view: that call is the reference
// for every bit this one returns, and the way everything goes that the launch below does not take.  What is new is the launch
// shape of a batch this small: the batch's pose_list_kernel -> k01_kernel -> pairs_kernel become ONE kernel
// (small_poses_kernel.hip) whose probe geometry travels in the kernel arguments; the batch's own segmented sum follows.
// That launch is opt-in (ecc_debug_set_gradient_launch): it measured no faster than the batch, which is the default.
#include "ecc_capi_internal.h"
#include "ecc_sum_order.h"

using namespace ecc_internal;

namespace {

// The Q probes of `view` (moved_Ps: Q x 12) and one pose that moves nothing through small_poses_kernel + the batch's sum:
// means[0 .. Q) the probes, means[Q] the current matrices.  *taken = false: the launch declines (include/ecc_hip.h lists when) and
// nothing was launched.
int gradient_one_launch(ecc_metric* m, int view, int Q, const double* moved_Ps, double* means, bool* taken)
{
    *taken = false;
    ecc_ctx* ctx = m->ctx;
    const int64_t n = m->n_views, n_pairs = n * (n - 1) / 2;
    if (Q > ECC_SMALL_PATCH_MAX) return ECC_OK;
    double base_radius = 0.0;
    ecc_metric_get_object_radius(m, &base_radius);
    const int32_t moved = view;
    for (int q = 0; q < Q; ++q)
        if (!pose_keeps_radius(m, base_radius, 1, &moved, moved_Ps + 12 * (size_t)q)) return ECC_OK;
    EccPairParams p;
    int rc = fill_pair_params(m, &p, n_pairs, /*need_e1=*/false);  // the sampling mode of an all-pairs evaluation
    if (rc) return rc;
    int wpp = 0;
    size_t lds = 0;
    if (!ecc_small_poses_plan(&p, Q, &wpp, &lds)) return ECC_OK;
    // the probes' entries are stored behind the views' (ecc_metric_set_projections leaves the room)
    if (m->PinvTs_d.cap < 12 * (n + ECC_SMALL_PATCH_MAX) || m->Cs_d.cap < 4 * (n + ECC_SMALL_PATCH_MAX)) return ECC_OK;

    ecc_mark_busy(m);
    // the base's pair values: kept between calls, only the pairs of views that changed since are redone (as the pose batch does)
    float* base_vals_d = nullptr;
    rc = evaluate_cached(m, 0, n_pairs, /*sum_d=*/nullptr, &base_vals_d);
    if (rc) return rc;
    rc = ensure_e1(m);  // the partners' geometry is read from the device arrays (a no-op unless a view is behind its matrix)
    if (rc) return rc;
    const int K = Q + 1;  // the pose behind the probes moves nothing: the metric at the current matrices
    const int64_t entries = n * (int64_t)Q;
    rc = m->pose_h.ensure((int64_t)sizeof(double) * K, 1 << 16, ctx->stream);
    if (!rc) rc = m->pose_values_d.ensure(entries, ctx->stream);
    if (!rc) rc = m->pose_partial_d.ensure((int64_t)K * ecc_sum::SLICES, ctx->stream);
    if (!rc) rc = m->pose_lists_d.ensure((int64_t)K + 1 + Q, ctx->stream);
    if (rc) return rc;

    EccSmallEval x;
    std::memset(&x, 0, sizeof(x));
    x.patch_count = Q;
    for (int q = 0; q < Q; ++q) {  // E1 of the probe matrices with the code e1_kernel compiles (bit-identical)
        ecc_host::pinv_transpose(moved_Ps + 12 * (size_t)q, &x.patch_geo[q][0]);
        ecc_host::source_position(moved_Ps + 12 * (size_t)q, &x.patch_geo[q][12]);
        x.patch_views[q] = (int)n + q;
    }
    EccSmallPoses y = {view, Q, K, m->pose_lists_d.ptr};
    p.PinvTs = m->PinvTs_d.ptr;
    p.Cs = m->Cs_d.ptr;
    p.pair_values = m->pose_values_d.ptr;
    HIP_TRY(launch_timed(ctx, [&](hipStream_t s) { return ecc_launch_small_poses(&p, &x, &y, s); }));
    std::vector<double> sums((size_t)K);
    rc = sum_poses(m, base_vals_d, K, Q, reinterpret_cast<volatile uint64_t*>(m->pose_h.host), reinterpret_cast<double*>(m->pose_h.dev),
                   sums.data());
    if (rc) return rc;
    for (int k = 0; k < K; ++k) means[k] = sums[k] / (double)n_pairs;  // ref: ...RadonIntermediate.cpp:224
    HIP_TRY(wait_stream_spin(ctx->stream));  // (the results were seen before the stream's own completion; the scratch is reused)
    m->quiet = true;
    *taken = true;
    return ECC_OK;
}

}  // namespace

ECC_EXPORT int ecc_metric_evaluate_gradient(ecc_metric* m, int view, int n_params, const double* Ps_plus, const double* Ps_minus,
                                            const double* h, double* value, double* grad, double* probes)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!Ps_plus || !Ps_minus || !h || !grad) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    if (n_params < 1 || n_params > (1 << 20)) return fail(ECC_ERR_INVALID_ARGUMENT, "n_params must be in [1, 2^20]");
    if (m->n_views < 1) return fail(ECC_ERR_INVALID_ARGUMENT, "projection matrices have not been set");
    if (m->n_views < 2) return fail(ECC_ERR_INVALID_ARGUMENT, "need at least two views (the reference divides 0/0 here)");
    if ((int)m->dtrs.size() < m->n_views) return fail(ECC_ERR_INVALID_ARGUMENT, "fewer Radon intermediates than projection matrices");
    if (view < 0 || view >= m->n_views) return fail(ECC_ERR_INVALID_ARGUMENT, "view outside [0, n_views)");
    for (int p = 0; p < n_params; ++p)
        if (!std::isfinite(h[p]) || h[p] == 0.0) return fail(ECC_ERR_INVALID_ARGUMENT, "every step length must be finite and not zero");
    int rc = set_device(m->ctx);
    if (rc) return rc;
    const int Q = 2 * n_params;
    std::vector<double> moved(12 * (size_t)Q), means((size_t)Q + 1);
    for (int p = 0; p < n_params; ++p) {  // plus_0, minus_0, plus_1, ...
        std::memcpy(moved.data() + 12 * (size_t)(2 * p), Ps_plus + 12 * (size_t)p, sizeof(double) * 12);
        std::memcpy(moved.data() + 12 * (size_t)(2 * p + 1), Ps_minus + 12 * (size_t)p, sizeof(double) * 12);
    }
    m->last_batched_poses = 0;
    bool taken = false;
    if (m->pose_batching && m->gradient_launch) {
        rc = gradient_one_launch(m, view, Q, moved.data(), means.data(), &taken);
        if (rc) return rc;
    }
    m->last_gradient_path = taken ? 2 : (m->pose_batching ? 1 : 0);
    if (!taken) {  // the probes as poses of one moved view each, then one that moves nothing
        std::vector<int32_t> off((size_t)Q + 2), views((size_t)Q, view);
        for (int k = 0; k <= Q; ++k) off[k] = k;
        off[(size_t)Q + 1] = Q;
        rc = ecc_metric_evaluate_pose_deltas(m, Q + 1, off.data(), views.data(), moved.data(), means.data());
        if (rc) return rc;
    }
    if (value) *value = means[(size_t)Q];
    if (probes) std::memcpy(probes, means.data(), sizeof(double) * (size_t)Q);
    for (int p = 0; p < n_params; ++p) grad[p] = (means[2 * (size_t)p] - means[2 * (size_t)p + 1]) / (2.0 * h[p]);
    return ECC_OK;
}

ECC_EXPORT int ecc_metric_last_gradient_path(const ecc_metric* m, int* path)
{
    if (!m || !path) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    *path = m->last_gradient_path;
    return ECC_OK;
}

ECC_EXPORT int ecc_debug_set_gradient_launch(ecc_metric* m, int on)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    m->gradient_launch = on ? 1 : 0;
    return ECC_OK;
}
