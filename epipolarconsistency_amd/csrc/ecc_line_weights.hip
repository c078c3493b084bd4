// ecc_line_weights.hip -- line weights made on the device (host code only): ecc_line_weights_defaults, ecc_radon_line_weights,
// ecc_radon_line_weights_into and ecc_dtr_line_weights of include/ecc_hip.h.
//
// Per sub-batch of at most 64 images, all on the context's stream: [dilate_max_kernel: flagged -> scratch images,] the Radon
// launches of ecc_radon_api.hip (FILTER_NONE, POST_IDENTITY, the context's arithmetic) into scratch slabs, clip_min_kernel: scratch
// slabs -> destination slabs, written completely.  No memset, no border launch, no host round trip.
#include "ecc_capi_internal.h"
#include "ecc_extremum_tile.h"

using namespace ecc_internal;

namespace {

constexpr int SUB_BATCH = 64;  // radon_launch's sub-batch: the scratch holds the lengths (and dilated images) of this many views

void defaults(ecc_line_weights_config* cfg)
{
    cfg->dilate_px = 0;
    cfg->guard_bins = 1;
    cfg->zero_at_px = 1.0f;
}

// cfg (null: the defaults) into *use, or the error of the first cap it breaks
int check_config(const ecc_line_weights_config* cfg, ecc_line_weights_config* use)
{
    defaults(use);
    if (!cfg) return ECC_OK;
    if (cfg->dilate_px < 0 || cfg->dilate_px > ecc_extremum::DILATE_MAX)
        return fail(ECC_ERR_INVALID_ARGUMENT, "line weights: dilate_px must be in [0, 16]");
    if (cfg->guard_bins < 0 || cfg->guard_bins > ecc_extremum::GUARD_MAX)
        return fail(ECC_ERR_INVALID_ARGUMENT, "line weights: guard_bins must be in [0, 8]");
    if (!(cfg->zero_at_px > 0.0f) || !std::isfinite(cfg->zero_at_px))
        return fail(ECC_ERR_INVALID_ARGUMENT, "line weights: zero_at_px must be finite and positive");
    *use = *cfg;
    return ECC_OK;
}

int check_stack(ecc_ctx* ctx, const float* flagged, int n, int n_u, int n_v, int n_alpha, int n_t, const void* dst,
                const ecc_line_weights_config* cfg, ecc_line_weights_config* use)
{
    if (!ctx) return fail(ECC_ERR_INVALID_ARGUMENT, "line weights: context is null");
    if (!flagged) return fail(ECC_ERR_INVALID_ARGUMENT, "line weights: the flagged images are null");
    if (!dst) return fail(ECC_ERR_INVALID_ARGUMENT, "line weights: the output is null");
    ecc_dtr* dummy = nullptr;
    const int rc = radon_check_args(ctx, flagged, n, n_u, n_v, n_alpha, n_t, ECC_FILTER_NONE, ECC_POST_IDENTITY, &dummy);
    if (rc) return rc;
    return check_config(cfg, use);
}

int ensure_scratch(ecc_ctx* ctx, size_t floats)
{
    if (ctx->line_weights_scratch_cap >= floats) return ECC_OK;
    if (ctx->line_weights_scratch_d) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        HIP_TRY(hipFree(ctx->line_weights_scratch_d));
        ctx->line_weights_scratch_d = nullptr;
        ctx->line_weights_scratch_cap = 0;
    }
    HIP_TRY(hipMalloc((void**)&ctx->line_weights_scratch_d, sizeof(float) * floats));
    ctx->line_weights_scratch_cap = floats;
    return ECC_OK;
}

// flagged_d: n images on the device; slabs_d: n destination slabs, `slab` floats apart
int launch_stack(ecc_ctx* ctx, const float* flagged_d, int n, int n_u, int n_v, int n_alpha, int n_t,
                 const ecc_line_weights_config& cfg, float* slabs_d)
{
    const int64_t slab = ecc_layout_floats(n_alpha, n_t), img = (int64_t)n_u * n_v;
    const int pitch = ecc_layout_pitch(n_t);
    const int sub = std::min(n, SUB_BATCH);
    int rc = ensure_scratch(ctx, (size_t)sub * (size_t)(slab + (cfg.dilate_px > 0 ? img : 0)));
    if (rc) return rc;
    float* lengths_d = ctx->line_weights_scratch_d;
    float* dilated_d = lengths_d + slab * sub;  // slab is a multiple of 32 floats: the images start on a 128-byte line
    for (int first = 0; first < n; first += sub) {
        const int cnt = std::min(sub, n - first);
        const float* src = flagged_d + img * first;
        if (cfg.dilate_px > 0) {
            HIP_TRY(ecc_launch_dilate_max(src, dilated_d, img, cnt, n_u, n_v, cfg.dilate_px, ctx->stream));
            src = dilated_d;
        }
        rc = radon_launch_stack(ctx, src, cnt, n_u, n_v, n_alpha, n_t, ECC_FILTER_NONE, ECC_POST_IDENTITY, lengths_d, slab);
        if (rc) return rc;
        HIP_TRY(ecc_launch_clip_min(lengths_d, slab, slabs_d + slab * first, slab, cnt, n_alpha, n_t, pitch, cfg.guard_bins,
                                    cfg.zero_at_px, ctx->stream));
    }
    return ECC_OK;
}

}  // namespace

namespace ecc_internal {
// n line-weight handles over one slab stack (ecc_robust_map.hip makes its weights' handles here too)
int make_weight_handles(ecc_ctx* ctx, const std::shared_ptr<Slab>& owner, int n, int n_alpha, int n_t, int n_u, int n_v, ecc_dtr** out)
{
    const int64_t slab = ecc_layout_floats(n_alpha, n_t);
    std::vector<ecc_dtr*> made;
    for (int k = 0; k < n; ++k) {
        ecc_dtr* d = new (std::nothrow) ecc_dtr();
        if (!d) {
            (void)hipStreamSynchronize(ctx->stream);  // the launches write the stack the last handle frees
            for (ecc_dtr* q : made) delete q;
            return fail(ECC_ERR_OUT_OF_MEMORY, "host allocation failed");
        }
        d->ctx = ctx;
        d->owner = owner;
        d->base = owner->ptr + slab * k;
        d->n_alpha = n_alpha;
        d->n_t = n_t;
        d->n_u = n_u;
        d->n_v = n_v;
        d->filter = ECC_FILTER_NONE;
        d->pitch = ecc_layout_pitch(n_t);
        made.push_back(d);
    }
    for (int k = 0; k < n; ++k) out[k] = made[k];
    return ECC_OK;
}
}  // namespace ecc_internal

ECC_EXPORT void ecc_line_weights_defaults(ecc_line_weights_config* cfg)
{
    if (cfg) defaults(cfg);
}

ECC_EXPORT int ecc_radon_line_weights(ecc_ctx* ctx, const float* flagged, int on_device, int n, int n_u, int n_v, int n_alpha, int n_t,
                                      const ecc_line_weights_config* cfg, ecc_dtr** out)
{
    ecc_line_weights_config use;
    int rc = check_stack(ctx, flagged, n, n_u, n_v, n_alpha, n_t, out, cfg, &use);
    if (rc) return rc;
    rc = set_device(ctx);
    if (rc) return rc;
    const int64_t slab = ecc_layout_floats(n_alpha, n_t);
    auto owner = std::make_shared<Slab>();
    owner->device = ctx->device;
    HIP_TRY(hipMalloc((void**)&owner->ptr, (size_t)slab * n * sizeof(float)));
    const float* flagged_d = flagged;
    float* staging = nullptr;
    if (!on_device) {
        const size_t bytes = (size_t)n * n_u * n_v * sizeof(float);
        HIP_TRY(hipMalloc((void**)&staging, bytes));
        const hipError_t e = hipMemcpyAsync(staging, flagged, bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            (void)hipFree(staging);
            HIP_TRY(e);
        }
        flagged_d = staging;
    }
    rc = launch_stack(ctx, flagged_d, n, n_u, n_v, n_alpha, n_t, use, owner->ptr);
    if (staging || rc) (void)hipStreamSynchronize(ctx->stream);
    if (staging) (void)hipFree(staging);
    if (rc) return rc;
    return make_weight_handles(ctx, owner, n, n_alpha, n_t, n_u, n_v, out);
}

ECC_EXPORT int ecc_radon_line_weights_into(ecc_ctx* ctx, const float* flagged_d, int n, int n_u, int n_v, int n_alpha, int n_t,
                                           const ecc_line_weights_config* cfg, float* slabs_d)
{
    ecc_line_weights_config use;
    int rc = check_stack(ctx, flagged_d, n, n_u, n_v, n_alpha, n_t, slabs_d, cfg, &use);
    if (rc) return rc;
    rc = set_device(ctx);
    if (rc) return rc;
    return launch_stack(ctx, flagged_d, n, n_u, n_v, n_alpha, n_t, use, slabs_d);
}

ECC_EXPORT int ecc_dtr_line_weights(ecc_ctx* ctx, const ecc_dtr* lengths, const ecc_line_weights_config* cfg, ecc_dtr** out)
{
    if (!ctx) return fail(ECC_ERR_INVALID_ARGUMENT, "line weights: context is null");
    if (!lengths) return fail(ECC_ERR_INVALID_ARGUMENT, "line weights: the length intermediate is null");
    if (!out) return fail(ECC_ERR_INVALID_ARGUMENT, "line weights: the output is null");
    ecc_line_weights_config use;
    int rc = check_config(cfg, &use);
    if (rc) return rc;
    if (lengths->filter != ECC_FILTER_NONE)
        return fail(ECC_ERR_INVALID_ARGUMENT, "line weights: the length intermediate must have ECC_FILTER_NONE");
    if (!lengths->ctx || lengths->ctx->device != ctx->device)
        return fail(ECC_ERR_INVALID_ARGUMENT, "line weights: the length intermediate lives on another device");
    rc = set_device(ctx);
    if (rc) return rc;
    // lengths written on another stream of the device: wait for them
    if (lengths->ctx->stream != ctx->stream) HIP_TRY(hipStreamSynchronize(lengths->ctx->stream));
    const int64_t slab = ecc_layout_floats(lengths->n_alpha, lengths->n_t);
    auto owner = std::make_shared<Slab>();
    owner->device = ctx->device;
    HIP_TRY(hipMalloc((void**)&owner->ptr, (size_t)slab * sizeof(float)));
    HIP_TRY(ecc_launch_clip_min(lengths->base, slab, owner->ptr, slab, 1, lengths->n_alpha, lengths->n_t, lengths->pitch, use.guard_bins,
                                use.zero_at_px, ctx->stream));
    return make_weight_handles(ctx, owner, 1, lengths->n_alpha, lengths->n_t, lengths->n_u, lengths->n_v, out);
}
