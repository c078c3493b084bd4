// ecc_weighted_robust_map.hip -- ecc_metric_evaluate_weighted_robust_map[_pairs], ecc_metric_weighted_robust_map_weights: where the
// robust loss rejects on a metric that already carries line weights (host code; include/ecc_hip.h states the contract,
// weighted_robust_map_kernel.hip has the kernels, DESIGN.md 4.25 the reasons).  ecc_metric_evaluate_robust_map maps an n-metric
// and its weights feed a 2 n metric; there the loop stopped, because a metric with weights could not be mapped.  These calls map
// it -- whatever its weights are: an earlier pass's, a collimator flag, both -- and multiply the map's factor into the weights it
// was made under, so the loss and the line weights can be iterated (api.py: refine_line_weights).
//
// The launch sequence is the map call's (robust_map_call, ecc_robust_map.hip) with weighted_robust_form's columns and division
// (ecc_weighted_robust.hip) and the weighted map kernels behind its launch.
// Not here: pose-delta and transform batches of either map; range, group and RCCL forms; use_corr; Tukey's biweight; an IRLS loop.
#include "ecc_form_call.h"
#include "ecc_robust_map.h"

using namespace ecc_internal;

namespace {

// weighted_robust_form with the map kernels behind its launch
PairForm weighted_robust_map_form(int loss, float delta, double* value, double* coverage, double* inlier_mass)
{
    PairForm f = weighted_robust_form(loss, delta, value, coverage, inlier_mass);
    f.launch = [=](ecc_metric* m, const EccPairParams& p, float* cols, int64_t col_stride) {
        EccWeightedRobustMapParams g;
        set_channel_strides(m, &g);  // the data channel and, one channel behind it, the weights
        g.values = cols;
        g.col_stride = col_stride;
        g.loss = loss;
        g.delta = delta;
        g.inv_delta = (float)(1.0 / (double)delta);  // formed here, on the host, in float64 (as weighted_robust_form does)
        set_map_planes(m, &g);
        return launch_timed(m->ctx, [&](hipStream_t s) { return ecc_launch_pairs_weighted_robust_map(&p, &g, s); });
    };
    return f;
}

}  // namespace

ECC_EXPORT int ecc_metric_evaluate_weighted_robust_map(ecc_metric* m, int loss, float delta, const int32_t* views, int n_mapped, float* hits,
                                                       float* rejected, double* value, double* coverage, double* inlier_mass,
                                                       float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    const int rc = weighted_robust_check(m, value, loss, delta);
    if (rc) return rc;
    const int64_t n = m->n_views;
    return robust_map_call(m, weighted_robust_map_form(loss, delta, value, coverage, inlier_mass), ECC_MAP_WEIGHTED, nullptr, n * (n - 1) / 2,
                           (int)n, views, n_mapped, hits, rejected, pair_terms);
}

ECC_EXPORT int ecc_metric_evaluate_weighted_robust_map_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, int loss, float delta,
                                                             const int32_t* views, int n_mapped, float* hits, float* rejected, double* value,
                                                             double* coverage, double* inlier_mass, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (n_pairs < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "negative list length");
    if (n_pairs > 0 && !idx4) return fail(ECC_ERR_INVALID_ARGUMENT, "index list is null");
    int rc = weighted_robust_check(m, value, loss, delta);
    if (rc) return rc;
    // P index the current matrices, D the DATA intermediates: the weights of a sample come from dtr n_views + D, its map is D's
    rc = check_index_list(idx4, n_pairs, m->n_views, m->n_views,
                          "index array contains invalid indices (matrices and data intermediates lie in [0, n_views))");
    if (rc) return rc;
    return robust_map_call(m, weighted_robust_map_form(loss, delta, value, coverage, inlier_mass), ECC_MAP_WEIGHTED, idx4, n_pairs, m->n_views,
                           views, n_mapped, hits, rejected, pair_terms);
}

ECC_EXPORT int ecc_metric_weighted_robust_map_weights(ecc_metric* m, float min_hits, float gain, ecc_dtr** out)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!out) return fail(ECC_ERR_INVALID_ARGUMENT, "the output is null");
    if (!(min_hits >= 0.0f) || !std::isfinite(min_hits)) return fail(ECC_ERR_INVALID_ARGUMENT, "min_hits must be finite and not negative");
    if (!(gain >= 0.0f) || !std::isfinite(gain)) return fail(ECC_ERR_INVALID_ARGUMENT, "gain must be finite and not negative");
    if (!m->map_valid || m->map_kind != ECC_MAP_WEIGHTED || m->map_n_mapped < 1 || !m->map_planes_d.ptr || m->map_n_slots != m->n_views ||
        (int64_t)m->dtrs.size() != 2 * (int64_t)m->n_views)
        return fail(ECC_ERR_INVALID_ARGUMENT,
                    "no weighted robust map held: call ecc_metric_evaluate_weighted_robust_map first (refresh_dtrs and set_params drop it)");
    // W_v: the slab of dtr n_views + v, the handle's own; the mapped views: behind the plane table
    return robust_map_feedback(m, [&](const float* h, const float* r, float* slabs, int n_map) {
        return ecc_launch_weighted_robust_map_weights(h, r, m->dtr_table_d.ptr + m->n_views, m->map_slot_d.ptr + m->map_n_slots, slabs, n_map,
                                                      m->n_alpha, m->n_t, m->pitch, min_hits, gain, m->ctx->stream);
    }, out);
}
