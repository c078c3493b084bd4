// ecc_robust_map.hip -- ecc_metric_evaluate_robust_map[_pairs], ecc_metric_robust_map_weights: where the robust loss rejects (host
// code; include/ecc_hip.h states the contract, robust_map_kernel.hip has the kernels, DESIGN.md 4.24 the reasons).  The robust calls
// answer "how consistent is the scan if I distrust outliers" with one number per pair; these answer "which lines of which view were
// distrusted" with two planes per view, and turn them into line weights on the device: the loss finds the bad lines, the line
// weights (ecc_weighted.hip) remove them for good, nobody flags pixels by hand.
//
// The launch sequence is a column-form call's (ecc_column_call.h) with robust_form's columns and division (ecc_robust.hip): the
// checks, column_call_begin -- the planes' room as its more_scratch, the plane table's upload and the planes' memset as its
// upload_more --, the map form's pair launch between the timing events, column_call_finish with the finishing kernel and the
// planes' copies as its queue_more, the one wait.  It is written once, over the form (robust_map_call): the map under line weights
// (ecc_weighted_robust_map.hip) runs it with weighted_robust_form's columns, the map in sigma units (ecc_variance_robust_map.hip)
// with variance_robust_form's.
#include "ecc_form_call.h"
#include "ecc_robust_map.h"

using namespace ecc_internal;

namespace {

// robust_form with the map kernels behind its launch
PairForm robust_map_form(int loss, float delta, double* value, double* inlier_mass)
{
    PairForm f = robust_form(loss, delta, value, inlier_mass);
    f.launch = [=](ecc_metric* m, const EccPairParams& p, float* cols, int64_t col_stride) {
        EccRobustMapParams g;
        g.values = cols;
        g.col_stride = col_stride;
        g.loss = loss;
        g.delta = delta;
        g.inv_delta = (float)(1.0 / (double)delta);  // formed here, on the host, in float64 (as robust_form does)
        set_map_planes(m, &g);
        return launch_timed(m->ctx, [&](hipStream_t s) { return ecc_launch_pairs_robust_map(&p, &g, s); });  // (robust_map_kernel.hip)
    };
    return f;
}

// room for `need` elements, at least twice what there was: a caller that maps more views call after call reallocates rarely
template <class T>
int ensure_geometric(ecc_internal::DeviceArray<T>& a, int64_t need, hipStream_t stream)
{
    if (a.ptr && a.cap >= need) return ECC_OK;
    return a.ensure(std::max<int64_t>(need, 2 * a.cap), stream);
}

// The list of mapped intermediates: views[0 .. n_mapped), or every one of the nD (n_mapped == 0) -> slot_of (nD entries, -1: not mapped).
int map_slots(const int32_t* views, int n_mapped, int nD, std::vector<int32_t>* slot_of, int* n_out)
{
    if (n_mapped < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "negative number of mapped views");
    if (n_mapped > 0 && !views) return fail(ECC_ERR_INVALID_ARGUMENT, "the list of mapped views is null");
    slot_of->assign((size_t)nD, -1);
    if (n_mapped == 0) {
        for (int v = 0; v < nD; ++v) (*slot_of)[v] = v;
        *n_out = nD;
        return ECC_OK;
    }
    for (int k = 0; k < n_mapped; ++k) {
        if (views[k] < 0 || views[k] >= nD) return fail(ECC_ERR_INVALID_ARGUMENT, "a mapped view is out of range");
        if ((*slot_of)[views[k]] >= 0) return fail(ECC_ERR_INVALID_ARGUMENT, "a mapped view is listed twice");
        (*slot_of)[views[k]] = k;
    }
    *n_out = n_mapped;
    return ECC_OK;
}

}  // namespace

// Everything of a map call behind the checks of its evaluation (ecc_robust_map.h); ecc_weighted_robust_map.hip calls it with the
// weighted form, ecc_variance_robust_map.hip with the variance-robust form.  The plane table is followed by the list of mapped
// intermediates, slot by slot, which the weighted map's weights kernel and the variance map's variances kernel read.
int ecc_internal::robust_map_call(ecc_metric* m, const PairForm& f, EccMapKind kind, const int32_t* idx4, int64_t count, int nD,
                                  const int32_t* views, int n_mapped, float* hits, float* rejected, float* pair_terms)
{
    std::vector<int32_t> slot_of;
    int n_map = 0;
    int rc = map_slots(views, n_mapped, nD, &slot_of, &n_map);
    if (rc) return rc;
    if (2 * (int64_t)n_map > 65535) return fail(ECC_ERR_INVALID_ARGUMENT, "more than 32767 mapped views");
    slot_of.resize((size_t)nD + (size_t)n_map);
    for (int v = 0; v < nD; ++v)
        if (slot_of[v] >= 0) slot_of[(size_t)nD + slot_of[v]] = v;
    const int64_t bins = (int64_t)m->n_alpha * m->n_t, cells = ecc_robust_map_plane_cells(m->n_alpha, m->n_t);
    m->map_valid = false;
    m->map_kind = kind;
    m->map_n_mapped = n_map;
    m->map_n_slots = nD;
    if (count == 0) {  // an empty list: nothing was sampled
        if (hits) std::fill(hits, hits + (size_t)n_map * bins, 0.0f);
        if (rejected) std::fill(rejected, rejected + (size_t)n_map * bins, 0.0f);
        return ECC_OK;
    }
    ecc_ctx* ctx = m->ctx;
    ColumnCall c;
    rc = column_call_begin(
        m, idx4, count, f.T, f.S, &c,
        [&]() -> int {
            int e = ensure_geometric(m->map_fixed_d, 2 * (int64_t)n_map * cells, ctx->stream);
            if (!e) e = ensure_geometric(m->map_planes_d, 2 * (int64_t)n_map * bins, ctx->stream);
            if (!e) e = ensure_geometric(m->map_slot_d, (int64_t)slot_of.size(), ctx->stream);
            return e;
        },
        [&]() -> int {
            HIP_TRY(hipMemcpyAsync(m->map_slot_d.ptr, slot_of.data(), sizeof(int32_t) * slot_of.size(), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(hipMemsetAsync(m->map_fixed_d.ptr, 0, sizeof(unsigned long long) * 2 * (size_t)n_map * (size_t)cells, ctx->stream));
            return ECC_OK;
        });
    if (rc) return rc;
    HIP_TRY(f.launch(m, c.p, m->gram_values_d.ptr, c.col_stride));
    std::vector<double> totals((size_t)f.S);  // in the order an evaluation of `count` values is added in (ecc_sum_order.h)
    rc = column_call_finish(m, c, f.S, totals.data(), f.T, m->gram_values_d.ptr, pair_terms, [&]() -> int {
        // the fixed-point block and the float block are both every HITS plane, then every REJ plane, as the caller's two arrays are
        HIP_TRY(ecc_launch_robust_map_finish(m->map_fixed_d.ptr, m->map_planes_d.ptr, 2 * n_map, m->n_alpha, m->n_t, m->pitch, ctx->stream));
        const size_t bytes = sizeof(float) * (size_t)n_map * (size_t)bins;
        if (hits) HIP_TRY(hipMemcpyAsync(hits, m->map_planes_d.ptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (rejected)
            HIP_TRY(hipMemcpyAsync(rejected, m->map_planes_d.ptr + (size_t)n_map * bins, bytes, hipMemcpyDeviceToHost, ctx->stream));
        return ECC_OK;
    });
    if (rc) return rc;
    f.finish(totals.data(), count, 0);
    m->map_valid = true;
    return ECC_OK;
}

ECC_EXPORT int ecc_metric_evaluate_robust_map(ecc_metric* m, int loss, float delta, const int32_t* views, int n_mapped, float* hits,
                                              float* rejected, double* value, double* inlier_mass, float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    int rc = robust_check(m, value, loss, delta);
    if (rc) return rc;
    if ((int64_t)m->dtrs.size() < (int64_t)m->n_views) return fail(ECC_ERR_INVALID_ARGUMENT, "fewer Radon intermediates than projection matrices");
    const int64_t n = m->n_views;
    return robust_map_call(m, robust_map_form(loss, delta, value, inlier_mass), ECC_MAP_PLAIN, nullptr, n * (n - 1) / 2, (int)n, views,
                           n_mapped, hits, rejected, pair_terms);
}

ECC_EXPORT int ecc_metric_evaluate_robust_map_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, int loss, float delta, const int32_t* views,
                                                    int n_mapped, float* hits, float* rejected, double* value, double* inlier_mass,
                                                    float* pair_terms)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (n_pairs < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "negative list length");
    if (n_pairs > 0 && !idx4) return fail(ECC_ERR_INVALID_ARGUMENT, "index list is null");
    int rc = robust_check(m, value, loss, delta);
    if (rc) return rc;
    rc = check_index_list(idx4, n_pairs, m->n_views, (int)m->dtrs.size(), "index array contains invalid indices");
    if (rc) return rc;
    return robust_map_call(m, robust_map_form(loss, delta, value, inlier_mass), ECC_MAP_PLAIN, idx4, n_pairs, (int)m->dtrs.size(), views,
                           n_mapped, hits, rejected, pair_terms);
}

ECC_EXPORT int ecc_metric_robust_map_weights(ecc_metric* m, float min_hits, float gain, ecc_dtr** out)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!out) return fail(ECC_ERR_INVALID_ARGUMENT, "the output is null");
    if (!(min_hits >= 0.0f) || !std::isfinite(min_hits)) return fail(ECC_ERR_INVALID_ARGUMENT, "min_hits must be finite and not negative");
    if (!(gain >= 0.0f) || !std::isfinite(gain)) return fail(ECC_ERR_INVALID_ARGUMENT, "gain must be finite and not negative");
    if (!m->map_valid || m->map_n_mapped < 1 || !m->map_planes_d.ptr)
        return fail(ECC_ERR_INVALID_ARGUMENT, "no robust map held: call ecc_metric_evaluate_robust_map first (refresh_dtrs and set_params drop it)");
    if (m->map_kind == ECC_MAP_WEIGHTED)
        return fail(ECC_ERR_INVALID_ARGUMENT, "the held map was made under line weights: its weights are ecc_metric_weighted_robust_map_weights'");
    if (m->map_kind != ECC_MAP_PLAIN)
        return fail(ECC_ERR_INVALID_ARGUMENT, "the held map was made in sigma units: it feeds ecc_metric_variance_robust_map_variances");
    return robust_map_feedback(m, [&](const float* h, const float* r, float* slabs, int n_map) {
        return ecc_launch_robust_map_weights(h, r, slabs, n_map, m->n_alpha, m->n_t, m->pitch, min_hits, gain, m->ctx->stream);
    }, out);
}

// Everything of a feedback call behind its checks (ecc_robust_map.h): the three kinds' calls differ in their checks and launches alone.
int ecc_internal::robust_map_feedback(ecc_metric* m, const std::function<hipError_t(const float*, const float*, float*, int)>& launch,
                                      ecc_dtr** out)
{
    ecc_ctx* ctx = m->ctx;
    const int rc = set_device(ctx);
    if (rc) return rc;
    const int n_map = m->map_n_mapped;
    const int64_t slab = ecc_layout_floats(m->n_alpha, m->n_t), bins = (int64_t)m->n_alpha * m->n_t;
    auto owner = std::make_shared<Slab>();
    owner->device = ctx->device;
    HIP_TRY(hipMalloc((void**)&owner->ptr, (size_t)slab * (size_t)n_map * sizeof(float)));
    ecc_mark_busy(m);
    HIP_TRY(launch(m->map_planes_d.ptr, m->map_planes_d.ptr + (size_t)n_map * bins, owner->ptr, n_map));
    return make_weight_handles(ctx, owner, n_map, m->n_alpha, m->n_t, m->n_u, m->n_v, out);
}

// Debug: the fixed-point planes of the held map, of any kind, as the kernel left them -- every HITS plane, then every REJ plane,
// (n_alpha + 2) x pitch cells each in the slab's padded geometry -- so that a test can add and compare the integer sums themselves.
ECC_EXPORT int ecc_debug_robust_map_fixed(ecc_metric* m, uint64_t* out, int64_t capacity)
{
    if (!m || !out) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    if (!m->map_valid) return fail(ECC_ERR_INVALID_ARGUMENT, "no robust map held");
    const int64_t cells = 2 * (int64_t)m->map_n_mapped * ecc_robust_map_plane_cells(m->n_alpha, m->n_t);
    if (capacity < cells) return fail(ECC_ERR_INVALID_ARGUMENT, "capacity too small for the held map");
    const int rc = set_device(m->ctx);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, m->map_fixed_d.ptr, sizeof(uint64_t) * (size_t)cells, hipMemcpyDeviceToHost, m->ctx->stream));
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));
    return ECC_OK;
}
