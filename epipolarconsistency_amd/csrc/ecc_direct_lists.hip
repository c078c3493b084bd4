// ecc_direct_lists.hip -- MetricDirect's index lists and pose batches behind the C ABI (host code only; the kernels are
// direct_list_kernel.hip).  ref: Metric::evaluate(indices, out) and Gui/SingleImageMotion.h, which builds the list
// (input_index, i, input_index, i) of the one view an optimiser moves.
//
// One call: everything the device needs (plane-angle ranges, candidate matrices, segment offsets, tuples) is laid out in one
// pinned block and copied once; the list runs in batches bounded as ecc_direct_evaluate's (256 MB of line integrals, 65535
// records), each batch writing its float64 values into a buffer that holds the whole list; one segmented sum; the outputs are
// copied back and the stream is waited for once.  All scratch grows geometrically and is kept with the metric.
#include "ecc_direct_internal.h"
#include "ecc_direct_lists_host.h"

#define ECC_EXPORT extern "C" __attribute__((visibility("default")))

using namespace ecc_internal;
namespace lists = ecc_direct_lists;

namespace {

// room for `need` elements, at least doubling what is there (DeviceArray::ensure alone grows to the exact size)
template <class T>
int grow(DeviceArray<T>& a, int64_t need, hipStream_t stream)
{
    if (need <= 0 || (a.cap >= need && a.ptr)) return ECC_OK;
    return a.ensure(std::max<int64_t>(need, 2 * a.cap), stream);
}

int64_t align8(int64_t bytes) { return (bytes + 7) & ~(int64_t)7; }

// The block a call hands to the device: [ranges: n float64][candidate matrices: 12 m float64][offsets: n_segments + 1 int64]
// [tuples: 4 n int32]
struct Stage {
    int64_t n = 0, m = 0, n_segments = 0;
    int64_t ranges_at() const { return 0; }
    int64_t Ps_at() const { return 8 * n; }
    int64_t offsets_at() const { return Ps_at() + 8 * 12 * m; }
    int64_t idx4_at() const { return offsets_at() + 8 * (n_segments + 1); }
    int64_t bytes() const { return align8(idx4_at() + 16 * n); }
};

int list_checks(const ecc_direct* d)
{
    if (d->n_views < 1) return fail(ECC_ERR_INVALID_ARGUMENT, "projection matrices have not been set");
    return ECC_OK;
}

// The staged list on the device -> pair values and segment sums.  The tuples' matrix indices are rows of the metric's view
// table; with candidates (st.m > 0) of a copy of it with the candidates' records behind it, so that the set matrices stay.
int run_list(ecc_direct* d, const Stage& st, double* pair_values, double* segment_sums)
{
    ecc_ctx* ctx = d->ctx;
    int n_max = 0;
    int rc = direct_n_max(d, &n_max);
    if (rc) return rc;
    // batches bounded by the grid's y extent and by 256 MB of line integrals in flight, as ecc_direct_evaluate's
    int64_t bound = (256ll << 20) / (8ll * n_max);
    if (bound < 1) bound = 1;
    if (bound > 65535) bound = 65535;
    if (d->list_batch_max > 0 && bound > d->list_batch_max) bound = d->list_batch_max;
    const int64_t batch = std::min(bound, st.n);
    if (d->batch_capacity < batch || d->n_max_capacity < n_max) {
        rc = direct_scratch(d, std::min(bound, std::max(batch, 2 * d->batch_capacity)), std::max(n_max, d->n_max_capacity));
        if (rc) return rc;
    }
    rc = grow(d->list_in, st.bytes(), ctx->stream);
    if (!rc) rc = grow(d->list_values, st.n, ctx->stream);
    if (!rc) rc = grow(d->list_sums, st.n_segments, ctx->stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(d->list_in.ptr, d->list_stage.host, (size_t)st.bytes(), hipMemcpyHostToDevice, ctx->stream));
    const char* in = d->list_in.ptr;
    const EccDirectView* views = d->views_d;
    if (st.m > 0) {
        rc = grow(d->list_views, d->n_views + st.m, ctx->stream);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(d->list_views.ptr, d->views_d, sizeof(EccDirectView) * (size_t)d->n_views, hipMemcpyDeviceToDevice,
                               ctx->stream));
        HIP_TRY(ecc_launch_direct_views(reinterpret_cast<const double*>(in + st.Ps_at()), (int)st.m, d->list_views.ptr + d->n_views,
                                        d->n_u, d->n_v, ctx->stream));
        views = d->list_views.ptr;
    }
    for (int64_t first = 0; first < st.n; first += batch) {
        EccDirectListParams q;
        std::memset(&q, 0, sizeof(q));
        EccDirectParams& p = q.b;
        p.images = d->images_d;
        p.imagesT = d->imagesT_d;
        p.image_stride = (int64_t)d->n_u * d->n_v;
        p.views = views;
        p.pairs = d->pairs_d;
        p.samples = d->samples_d;
        p.pair_metric = d->list_values.ptr + first;
        p.first = first;
        p.count = std::min<int64_t>(batch, st.n - first);
        p.n_views = d->n_images;
        p.n_u = d->n_u;
        p.n_v = d->n_v;
        p.n_max = d->n_max_capacity;
        p.object_radius_mm = direct_radius(d);
        p.dkappa = d->dkappa;
        p.use_fbcc = d->use_fbcc ? 1 : 0;
        p.k_second = reinterpret_cast<const double*>(in + st.ranges_at()) + first;
        q.idx4 = reinterpret_cast<const int32_t*>(in + st.idx4_at()) + 4 * first;
        HIP_TRY(ecc_launch_direct_list_batch(&q, ctx->stream));
    }
    if (segment_sums) {
        HIP_TRY(ecc_launch_direct_segment_sums(d->list_values.ptr, reinterpret_cast<const int64_t*>(in + st.offsets_at()),
                                               (int)st.n_segments, d->list_sums.ptr, ctx->stream));
        HIP_TRY(hipMemcpyAsync(segment_sums, d->list_sums.ptr, sizeof(double) * (size_t)st.n_segments, hipMemcpyDeviceToHost,
                               ctx->stream));
    }
    if (pair_values)
        HIP_TRY(hipMemcpyAsync(pair_values, d->list_values.ptr, sizeof(double) * (size_t)st.n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ECC_OK;
}

}  // namespace

ECC_EXPORT int ecc_direct_evaluate_pairs(ecc_direct* d, const int32_t* idx4, int64_t n_pairs, const int64_t* segment_offsets,
                                         int n_segments, double* pair_values, double* segment_sums)
{
    if (!d) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (!pair_values && !segment_sums) return fail(ECC_ERR_INVALID_ARGUMENT, "pair_values and segment_sums are both null");
    if (n_pairs < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "negative number of pairs");
    if (n_pairs > 0 && !idx4) return fail(ECC_ERR_INVALID_ARGUMENT, "idx4 is null");
    if (!segment_offsets) n_segments = 1;
    if (n_segments < 0 || n_segments > lists::MAX_PAIRS + 1) return fail(ECC_ERR_INVALID_ARGUMENT, "number of segments out of range");
    int rc = list_checks(d);
    if (rc) return rc;
    std::string e = lists::check_idx4(idx4, n_pairs, d->n_views, d->n_images);
    if (e.empty() && segment_offsets) e = lists::check_offsets(segment_offsets, n_segments, n_pairs, "segment");
    if (!e.empty()) return fail(ECC_ERR_INVALID_ARGUMENT, e);
    if (n_pairs == 0) {
        for (int s = 0; segment_sums && s < n_segments; ++s) segment_sums[s] = 0.0;
        return ECC_OK;
    }
    ecc_ctx* ctx = d->ctx;
    rc = set_device(ctx);
    if (rc) return rc;
    Stage st;
    st.n = n_pairs;
    st.n_segments = segment_sums ? n_segments : 0;
    rc = d->list_stage.ensure(st.bytes(), 4096, ctx->stream);
    if (rc) return rc;
    char* h = d->list_stage.host;
    double* ranges = reinterpret_cast<double*>(h + st.ranges_at());
    const double user_radius = direct_radius(d);
    for (int64_t q = 0; q < n_pairs; ++q) {
        const int i = idx4[4 * q], j = idx4[4 * q + 1];
        ranges[q] = direct_range(&d->centers[4 * (size_t)i], &d->centers[4 * (size_t)j], user_radius, d->radii[i], d->radii[j]);
    }
    if (segment_sums) {
        int64_t* off = reinterpret_cast<int64_t*>(h + st.offsets_at());
        if (segment_offsets) std::memcpy(off, segment_offsets, sizeof(int64_t) * ((size_t)n_segments + 1));
        else off[0] = 0, off[1] = n_pairs;
    }
    std::memcpy(h + st.idx4_at(), idx4, sizeof(int32_t) * 4 * (size_t)n_pairs);
    return run_list(d, st, pair_values, segment_sums);
}

ECC_EXPORT int ecc_direct_pose_pairs_bound(const ecc_direct* d, int n_poses, const int32_t* moved_offsets, int64_t* n_pairs)
{
    if (!d || !n_pairs) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    *n_pairs = 0;
    if (n_poses < 1) return ECC_OK;
    if (!moved_offsets) return fail(ECC_ERR_INVALID_ARGUMENT, "moved_offsets is null");
    const std::string e = lists::check_poses(n_poses, moved_offsets, nullptr, d->n_images, n_pairs);
    if (!e.empty()) return fail(ECC_ERR_INVALID_ARGUMENT, e);
    return ECC_OK;
}

ECC_EXPORT int ecc_direct_evaluate_pose_deltas(ecc_direct* d, int n_poses, const int32_t* moved_offsets, const int32_t* moved_views,
                                               const double* moved_Ps, double* sums, double* pair_values, int32_t* pair_idx4)
{
    if (!d) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (n_poses < 1) return ECC_OK;
    if (!moved_offsets || !sums) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    int rc = list_checks(d);
    if (rc) return rc;
    if (d->n_views < d->n_images) return fail(ECC_ERR_INVALID_ARGUMENT, "fewer projection matrices than images");
    if (moved_offsets[0] == 0 && moved_offsets[n_poses] > 0 && (!moved_views || !moved_Ps))
        return fail(ECC_ERR_INVALID_ARGUMENT, "moved_views or moved_Ps is null");
    int64_t n_pairs = 0;
    const std::string e = lists::check_poses(n_poses, moved_offsets, moved_views, d->n_images, &n_pairs);
    if (!e.empty()) return fail(ECC_ERR_INVALID_ARGUMENT, e);
    for (int k = 0; k < n_poses; ++k) sums[k] = 0.0;
    if (n_pairs == 0) return ECC_OK;
    ecc_ctx* ctx = d->ctx;
    rc = set_device(ctx);
    if (rc) return rc;
    const int n = d->n_images, base = d->n_views;  // candidate q is row base + q of the call's view table
    Stage st;
    st.n = n_pairs;
    st.m = moved_offsets[n_poses];
    st.n_segments = n_poses;
    rc = d->list_stage.ensure(st.bytes(), 4096, ctx->stream);
    if (rc) return rc;
    char* h = d->list_stage.host;
    double* ranges = reinterpret_cast<double*>(h + st.ranges_at());
    int64_t* off = reinterpret_cast<int64_t*>(h + st.offsets_at());
    int32_t* idx4 = reinterpret_cast<int32_t*>(h + st.idx4_at());
    std::memcpy(h + st.Ps_at(), moved_Ps, sizeof(double) * 12 * (size_t)st.m);
    // the candidates' source positions and radius estimates, as ecc_direct_set_projections keeps them for the set matrices
    std::vector<double> cC(4 * (size_t)st.m), cR((size_t)st.m);
    for (int64_t q = 0; q < st.m; ++q) {
        ecc_host::camera_center(moved_Ps + 12 * q, &cC[4 * (size_t)q]);
        cR[(size_t)q] = ecc_host::object_radius(moved_Ps + 12 * q, d->n_u, d->n_v);
    }
    std::vector<int> slot((size_t)n, -1), sorted;
    int64_t at = 0;
    off[0] = 0;
    for (int k = 0; k < n_poses; ++k) {
        const int32_t q0 = moved_offsets[k];
        // ref: Metric::getObjectRadius: the user's value or the estimate of the pose's FIRST view
        double radius = direct_radius(d);
        if (!(d->object_radius_mm > 0))
            for (int32_t q = q0; q < moved_offsets[k + 1]; ++q)
                if (moved_views[q] == 0) radius = cR[(size_t)q];
        lists::pose_pairs(n, moved_views + q0, moved_offsets[k + 1] - q0, slot, sorted, [&](int i, int j, int si, int sj) {
            const size_t ci = (size_t)q0 + (size_t)si, cj = (size_t)q0 + (size_t)sj;  // (used where the slot is not -1)
            ranges[at] = direct_range(si >= 0 ? &cC[4 * ci] : &d->centers[4 * (size_t)i], sj >= 0 ? &cC[4 * cj] : &d->centers[4 * (size_t)j],
                                      radius, si >= 0 ? cR[ci] : d->radii[(size_t)i], sj >= 0 ? cR[cj] : d->radii[(size_t)j]);
            int32_t* t = idx4 + 4 * at;
            t[0] = si >= 0 ? base + (int)ci : i;
            t[1] = sj >= 0 ? base + (int)cj : j;
            t[2] = i;
            t[3] = j;
            ++at;
        });
        off[k + 1] = at;
    }
    if (pair_idx4)
        for (int64_t q = 0; q < n_pairs; ++q) {
            pair_idx4[4 * q] = pair_idx4[4 * q + 2] = idx4[4 * q + 2];
            pair_idx4[4 * q + 1] = pair_idx4[4 * q + 3] = idx4[4 * q + 3];
        }
    return run_list(d, st, pair_values, sums);
}

ECC_EXPORT int ecc_debug_set_direct_batch(ecc_direct* d, int64_t max_pairs)
{
    if (!d || max_pairs < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null or the bound is negative");
    d->list_batch_max = max_pairs;
    return ECC_OK;
}
