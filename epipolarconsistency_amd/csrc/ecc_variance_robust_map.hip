// ecc_variance_robust_map.hip -- ecc_metric_evaluate_variance_robust_map[_pairs], ecc_metric_variance_robust_map_variances: where the
// robust loss rejects in sigma units (host code; include/ecc_hip.h states the contract, variance_robust_map_kernel.hip has the
// kernels, DESIGN.md 4.31 the reasons).  ecc_metric_evaluate_variance_robust applies the loss to z = d / sigma with known variances,
// so a line that is merely noisy, and known to be, is not rejected; a map of the raw-residual loss would point at exactly that
// line.  These calls map the studentised loss -- REJ / HITS is the share of a bin's samples with |z| > delta -- and turn the held
// map into the next pass's variance fields, V / mu with mu the mean loss weight that reached the bin: what the loss distrusts once
// is known to be noisy afterwards, and ecc_metric_evaluate_variance alone is then robust (api.py: refine_variances).
//
// The launch sequence is the map call's (robust_map_call, ecc_robust_map.hip) with variance_robust_form's columns and division
// (ecc_variance_robust.hip) and the map kernels behind its launch.
// Not here: pose-delta and transform batches of any map; range, group and RCCL forms; use_corr; a third plane of squared
// residuals; an IRLS loop.
#include "ecc_form_call.h"
#include "ecc_robust_map.h"

using namespace ecc_internal;

namespace {

// variance_robust_form with the map kernels behind its launch
PairForm variance_robust_map_form(int loss, float delta, float floor, double* value, double* mean_weight, double* inlier_mass)
{
    PairForm f = variance_robust_form(loss, delta, floor, value, mean_weight, inlier_mass);
    f.launch = [=](ecc_metric* m, const EccPairParams& p, float* cols, int64_t col_stride) {
        EccVarianceRobustMapParams g;
        set_channel_strides(m, &g);  // the data channel and, one channel behind it, the variance fields
        g.values = cols;
        g.col_stride = col_stride;
        g.floor = floor;
        g.loss = loss;
        g.delta = delta;
        g.inv_delta = (float)(1.0 / (double)delta);  // formed here, on the host, in float64 (as variance_robust_form does)
        set_map_planes(m, &g);
        return launch_timed(m->ctx, [&](hipStream_t s) { return ecc_launch_pairs_variance_robust_map(&p, &g, s); });
    };
    return f;
}

}  // namespace

ECC_EXPORT int ecc_metric_evaluate_variance_robust_map(ecc_metric* m, int loss, float delta, float floor, const int32_t* views, int n_mapped,
                                                       float* hits, float* rejected, double* value, double* mean_weight, double* inlier_mass,
                                                       float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    const int rc = variance_robust_check(m, value, loss, delta, floor);
    if (rc) return rc;
    const int64_t n = m->n_views;
    return robust_map_call(m, variance_robust_map_form(loss, delta, floor, value, mean_weight, inlier_mass), ECC_MAP_VARIANCE, nullptr,
                           n * (n - 1) / 2, (int)n, views, n_mapped, hits, rejected, pair_terms);
}

ECC_EXPORT int ecc_metric_evaluate_variance_robust_map_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, int loss, float delta, float floor,
                                                             const int32_t* views, int n_mapped, float* hits, float* rejected, double* value,
                                                             double* mean_weight, double* inlier_mass, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (n_pairs < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "negative list length");
    if (n_pairs > 0 && !idx4) return fail(ECC_ERR_INVALID_ARGUMENT, "index list is null");
    int rc = variance_robust_check(m, value, loss, delta, floor);
    if (rc) return rc;
    // P index the current matrices, D the DATA intermediates: the variance of a sample comes from dtr n_views + D, its map is D's
    rc = check_index_list(idx4, n_pairs, m->n_views, m->n_views,
                          "index array contains invalid indices (matrices and data intermediates lie in [0, n_views))");
    if (rc) return rc;
    return robust_map_call(m, variance_robust_map_form(loss, delta, floor, value, mean_weight, inlier_mass), ECC_MAP_VARIANCE, idx4, n_pairs,
                           m->n_views, views, n_mapped, hits, rejected, pair_terms);
}

ECC_EXPORT int ecc_metric_variance_robust_map_variances(ecc_metric* m, float floor, float min_hits, float gain, float max_factor, ecc_dtr** out)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!out) return fail(ECC_ERR_INVALID_ARGUMENT, "the output is null");
    if (!(floor > 0.0f) || !std::isfinite(floor)) return fail(ECC_ERR_INVALID_ARGUMENT, "floor must be finite and positive");
    if (!(min_hits >= 0.0f) || !std::isfinite(min_hits)) return fail(ECC_ERR_INVALID_ARGUMENT, "min_hits must be finite and not negative");
    if (!(gain >= 0.0f) || !std::isfinite(gain)) return fail(ECC_ERR_INVALID_ARGUMENT, "gain must be finite and not negative");
    if (!(max_factor >= 1.0f) || !std::isfinite(max_factor)) return fail(ECC_ERR_INVALID_ARGUMENT, "max_factor must be finite and at least 1");
    if (!m->map_valid || m->map_kind != ECC_MAP_VARIANCE || m->map_n_mapped < 1 || !m->map_planes_d.ptr || m->map_n_slots != m->n_views ||
        (int64_t)m->dtrs.size() != 2 * (int64_t)m->n_views)
        return fail(ECC_ERR_INVALID_ARGUMENT,
                    "no variance robust map held: call ecc_metric_evaluate_variance_robust_map first (refresh_dtrs and set_params drop it)");
    // V_v: the slab of dtr n_views + v, the handle's own; the mapped views: behind the plane table
    return robust_map_feedback(m, [&](const float* h, const float* r, float* slabs, int n_map) {
        return ecc_launch_variance_robust_map_variances(h, r, m->dtr_table_d.ptr + m->n_views, m->map_slot_d.ptr + m->map_n_slots, slabs, n_map,
                                                        m->n_alpha, m->n_t, m->pitch, floor, min_hits, gain, max_factor, m->ctx->stream);
    }, out);
}
