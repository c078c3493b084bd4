// ecc_transforms.hip -- many rigid source-to-target transforms of ONE pair of scans per call (the registration of two scans;
// ref: tools/Registration/Registration3D3D.hxx:56-62, :91-110 -- the views of a SOURCE scan first, those of a TARGET scan
// behind them; a cost call multiplies every source matrix by one 4x4 transform, calls setProjectionMatrices and evaluates
// the index list of all source x target pairs).
//
// The reference -- and ecc_metric_set_projections + ecc_metric_evaluate_pairs here -- evaluates a transform at a time: host E1
// and an upload of n_source matrices, a list upload and the fixed cost of a list evaluation for every probe of a sweep, a
// finite-difference gradient or a population-based optimiser.  ecc_metric_evaluate_transforms does, for K transforms:
//   transform_list  ONE launch: P_i T_k (ecc_host::compose_transform, the host's bits) and E1 of the n base views followed by the
//                   K x n_source composed matrices (e1_kernel's code) -- the EXTENDED geometry, source view i under transform
//                   k at entry n + k n_source + i -- and, in the workgroups behind those, the index grid: entry e = q K + k
//                   (pair-major, transform-minor: neighbours in the launch sample the same two Radon intermediates under slightly
//                   different geometries) = pair q = j n_source + i of transform k, (n + k n_source + i, n_source + j, i,
//                   n_source + j), and its value slot k seg + q (seg = the list length rounded up to whole float4)
//   k01_kernel      ONE launch over the grid -- k01_radii_kernel under the automatic object radius: the radius follows the
//                   COMPOSED view 0 (ref: Metric::getObjectRadius), so every transform has its own; the host derives the K
//                   floats ecc_metric_set_projections would have passed and entry e takes radii[e % K]
//   pairs_kernel    ONE launch over it; the values go to their slots, i.e. transform-major, each transform's in list order
//   sum_transforms  ONE launch: per transform the float64 total of its values in the order of ecc_sum_order.h, the slice
//                   sums added in slice order by finish_transforms where there are sixteen -> pinned host memory
// A pair value depends on its two matrices, its two Radon intermediates and the parameters only, the sampling mode is the one a
// list of n_source n_target pairs resolves to, and the sum's order is reproduced: every mean and every pair value has the
// bits of ecc_metric_set_projections(composed matrices) + ecc_metric_evaluate_pairs(that list) (tests/test_gpu_transforms.py).
// Nothing of the metric's own state is written: current matrices, device geometry, kept records and values stay; the scratch
// is the pose batch's (pose_*), which every batch of either kind rewrites from scratch.
// The two drivers of a call, transforms_batched and transforms_sequential below, are ecc_form_call.h's as well
// (DESIGN.md 4.21); the result slots are armed and awaited through ecc_poses.hip's arm_pose_results / wait_pose_results.
#include "ecc_capi_internal.h"
#include "ecc_sum_order.h"

using namespace ecc_internal;

namespace {

constexpr int SUM_THREADS = ecc_sum::THREADS, SUM_SLICES = ecc_sum::SLICES;
// transforms per batch: they are the y dimension of the sum's grid
constexpr int64_t TRANSFORM_BATCH_MAX = 32768;
static_assert(TRANSFORM_BATCH_MAX < 65536, "transforms are the y dimension of sum_transforms_kernel's grid");

// Workgroups [0, e1_blocks): E1 of the extended matrices, 64 views each -- wave 0 (P^+)^T, wave 1 the source positions, as in
// e1_kernel (geometry_kernel.hip; the same code, ecc_host_geometry.h, the same bits).  View v < n is base matrix v; view
// n + k n_source + i is base matrix i times transform k.
// The workgroups behind them: 256 grid entries each (index tuple and value slot); the first K entries' threads also copy the
// radii from the pinned block into device memory for the record launch.
__global__ __launch_bounds__(256) void transform_list_kernel(const double* __restrict__ Ps, const double* __restrict__ Ts, int n,
                                                             int n_source, int n_target, int K, unsigned e1_blocks, long long seg,
                                                             int32_t* __restrict__ idx, int32_t* __restrict__ slots,
                                                             float* __restrict__ PinvTs, float* __restrict__ Cs,
                                                             const float* __restrict__ radii_h, float* __restrict__ radii_d)
{
    if (blockIdx.x < e1_blocks) {  // uniform over the workgroup
        const int role = threadIdx.x >> 6;
        const long long v = (long long)blockIdx.x * 64 + (threadIdx.x & 63);
        if (role > 1 || v >= n + (long long)K * n_source) return;
        double P[12];
        if (v < n) {
#pragma unroll
            for (int q = 0; q < 12; ++q) P[q] = Ps[12 * (size_t)v + q];
        } else {
            const int k = (int)((v - n) / n_source), i = (int)((v - n) - (long long)k * n_source);
            double B[12], T[16];
#pragma unroll
            for (int q = 0; q < 12; ++q) B[q] = Ps[12 * (size_t)i + q];
#pragma unroll
            for (int q = 0; q < 16; ++q) T[q] = Ts[16 * (size_t)k + q];
            ecc_host::compose_transform(B, T, P);
        }
        if (role == 0) {
            float pinvT[12];
            ecc_host::pinv_transpose(P, pinvT);
#pragma unroll
            for (int q = 0; q < 12; ++q) PinvTs[12 * (size_t)v + q] = pinvT[q];
        } else {
            float C[4];
            ecc_host::source_position(P, C);
#pragma unroll
            for (int q = 0; q < 4; ++q) Cs[4 * (size_t)v + q] = C[q];
        }
        return;
    }
    const long long e = (long long)(blockIdx.x - e1_blocks) * 256 + threadIdx.x;
    const long long entries = (long long)n_source * n_target * K;
    if (e >= entries) return;
    if (radii_h && e < K) radii_d[e] = radii_h[e];
    const long long q = e / K;
    const int k = (int)(e - q * K), j = (int)(q / n_source), i = (int)(q - (long long)j * n_source);
    reinterpret_cast<int4*>(idx)[e] = make_int4(n + k * n_source + i, n_source + j, i, n_source + j);
    slots[e] = (int32_t)(k * seg + q);
}

// Workgroup (slice, transform): the float64 sum of the slice of the transform's `count` values, vals[k seg ..], in the order
// of ecc_sum_order.h (seg is a multiple of 4 floats: every transform's values start on a float4).
template <int SLICES>
__global__ __launch_bounds__(SUM_THREADS) void sum_transforms_kernel(const float* __restrict__ vals, long long count, long long seg,
                                                                     double* __restrict__ partial, double* __restrict__ out_host)
{
    __shared__ double s[SUM_THREADS / 64];
    const int k = blockIdx.y, slice = blockIdx.x, t = threadIdx.x;
    const float* __restrict__ v = vals + (size_t)k * seg;
    const float4* __restrict__ v4 = reinterpret_cast<const float4*>(v);
    const long long n4 = count >> 2;
    long long lo, hi;
    ecc_sum::slice_bounds(n4, SLICES, slice, &lo, &hi);
    ecc_sum::Acc4 a;
    for (long long kk = lo + t; kk < hi; kk += SUM_THREADS) ecc_sum::add(a, v4[kk]);
    double acc = ecc_sum::combine(a);
    if (slice == SLICES - 1 && t == 0) ecc_sum::add_tail(acc, v + (n4 << 2), n4, count);
    ecc_sum::stage_wave_sums(acc, s);
    if (t == 0) {
        const double part = ecc_sum::waves_in_order(s);
        if (SLICES == 1)  // one slice: this IS the result (no finish_transforms_kernel launch)
            __hip_atomic_store(reinterpret_cast<unsigned long long*>(out_host) + k, (unsigned long long)__double_as_longlong(part),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        else partial[(size_t)k * SLICES + slice] = part;
    }
}

// Transform k's slice sums added in slice order (ecc_sum_order.h) -> the pinned result array (system-scope store: visible to
// the host before the stream is reported idle).
__global__ __launch_bounds__(256) void finish_transforms_kernel(const double* __restrict__ partial, int slices, int K,
                                                                double* __restrict__ out_host)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    double tot = 0.0;
    for (int b = 0; b < slices; ++b) tot += partial[(size_t)k * slices + b];
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(out_host) + k, (unsigned long long)__double_as_longlong(tot),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

size_t align64(size_t x) { return (x + 63) & ~(size_t)63; }

// the pinned block of a batch: base matrices | transforms | results | radii (byte offsets)
struct TransformBlock {
    size_t Ps, Ts, out, radii, end;
};
TransformBlock transform_block(int64_t n, int K, int result_words)
{
    TransformBlock b;
    b.Ps = 0;
    b.Ts = align64(sizeof(double) * 12 * (size_t)n);
    b.out = b.Ts + align64(sizeof(double) * 16 * (size_t)K);
    b.radii = b.out + align64(sizeof(double) * (size_t)result_words);
    b.end = b.radii + align64(sizeof(float) * (size_t)K);
    return b;
}

}  // namespace
namespace ecc_internal {
// The float the launches of ecc_metric_set_projections(composed matrices) would take for their object radius
// (fill_pair_params): the metric's fixed one, or the automatic one of the composed view 0.
float radius_of_transform(const ecc_metric* m, const double* base, const double* T)
{
    if (m->object_radius_mm > 0) return (float)m->object_radius_mm;
    double P0[12];
    ecc_host::compose_transform(base, T, P0);
    return (float)ecc_host::object_radius(P0, m->n_u, m->n_v);
}

// The host half of a batch's grid: the pinned block -- base matrices | the K transforms | result_words result slots | under the
// automatic object radius the K radii -- is filled, and the device arrays of the extended geometry, the index grid, its value slots
// and records (and the radii) have room.  *out / *out_dev: host and device address of the result slots, which the caller arms.
int stage_transform_grid(ecc_metric* m, const double* base, int n_source, int K, const double* Ts, int result_words,
                         volatile uint64_t** out, double** out_dev)
{
    ecc_ctx* ctx = m->ctx;
    const int64_t n = m->n_views, entries = (int64_t)n_source * (n - n_source) * K, ext = n + (int64_t)K * n_source;
    const bool per_transform_radius = !(m->object_radius_mm > 0);
    const TransformBlock b = transform_block(n, K, result_words);
    int rc = m->pose_h.ensure((int64_t)b.end, 1 << 16, ctx->stream);
    if (rc) return rc;
    char* const h = m->pose_h.host;
    float* radii_h = reinterpret_cast<float*>(h + b.radii);
    std::memcpy(h + b.Ps, base, sizeof(double) * 12 * (size_t)n);
    std::memcpy(h + b.Ts, Ts, sizeof(double) * 16 * (size_t)K);
    if (per_transform_radius)
        for (int k = 0; k < K; ++k) radii_h[k] = radius_of_transform(m, base, Ts + 16 * (size_t)k);
    std::atomic_thread_fence(std::memory_order_seq_cst);
    *out = reinterpret_cast<volatile uint64_t*>(h + b.out);
    *out_dev = reinterpret_cast<double*>(m->pose_h.dev + b.out);

    rc = m->pose_PinvTs_d.ensure(12 * ext, ctx->stream);
    if (!rc) rc = m->pose_Cs_d.ensure(4 * ext, ctx->stream);
    if (!rc) rc = m->pose_idx_d.ensure(4 * entries, ctx->stream);
    if (!rc) rc = m->pose_lists_d.ensure(entries, ctx->stream);  // the value slots
    if (!rc) rc = m->pose_records_d.ensure(entries, ctx->stream);
    if (!rc && per_transform_radius) rc = m->transform_radii_d.ensure(K, ctx->stream);
    return rc;
}

// transform_list_kernel over the block stage_transform_grid has just filled (the same n_source, K and result_words); seg: the
// distance of two transforms' value slots.
hipError_t launch_transform_list(ecc_metric* m, int n_source, int K, long long seg, int result_words)
{
    const int64_t n = m->n_views, n_target = n - n_source, entries = (int64_t)n_source * n_target * K, ext = n + (int64_t)K * n_source;
    const bool per_transform_radius = !(m->object_radius_mm > 0);
    const TransformBlock b = transform_block(n, K, result_words);
    const char* const h_dev = m->pose_h.dev;
    const unsigned e1_blocks = (unsigned)((ext + 63) / 64), idx_blocks = (unsigned)((entries + 255) / 256);
    hipLaunchKernelGGL(transform_list_kernel, dim3(e1_blocks + idx_blocks), dim3(256), 0, m->ctx->stream,
                       reinterpret_cast<const double*>(h_dev + b.Ps), reinterpret_cast<const double*>(h_dev + b.Ts), (int)n, n_source,
                       (int)n_target, K, e1_blocks, seg, m->pose_idx_d.ptr, m->pose_lists_d.ptr, m->pose_PinvTs_d.ptr,
                       m->pose_Cs_d.ptr, per_transform_radius ? reinterpret_cast<const float*>(h_dev + b.radii) : nullptr,
                       m->transform_radii_d.ptr);
    return hipGetLastError();
}
}  // namespace ecc_internal
namespace {

// One batch: K transforms Ts (16 doubles each) of the base matrices (n x 12).  sums[k]: the float64 total of transform k's
// n_source n_target values; values (nullable, host): K x count floats.
int run_batch(ecc_metric* m, const double* base, int n_source, int K, const double* Ts, double* sums, float* values)
{
    ecc_ctx* ctx = m->ctx;
    const int64_t n = m->n_views, n_target = n - n_source, count = (int64_t)n_source * n_target;
    const int64_t seg = (count + 3) & ~(int64_t)3, entries = count * K;
    const bool per_transform_radius = !(m->object_radius_mm > 0);
    volatile uint64_t* out = nullptr;
    double* out_dev = nullptr;
    int rc = stage_transform_grid(m, base, n_source, K, Ts, K, &out, &out_dev);
    if (rc) return rc;
    arm_pose_results(out, K);
    rc = m->pose_values_d.ensure(seg * K, ctx->stream);
    if (!rc) rc = m->pose_partial_d.ensure((int64_t)K * SUM_SLICES, ctx->stream);
    if (rc) return rc;

    EccPairParams p;
    rc = fill_pair_params(m, &p, count, /*need_e1=*/false);  // the sampling mode of a list of `count` pairs
    if (rc) return rc;
    HIP_TRY(launch_transform_list(m, n_source, K, (long long)seg, K));
    p.PinvTs = m->pose_PinvTs_d.ptr;
    p.Cs = m->pose_Cs_d.ptr;
    p.indices = m->pose_idx_d.ptr;
    p.records = m->pose_records_d.ptr;
    p.pair_values = m->pose_values_d.ptr;
    p.value_slots = m->pose_lists_d.ptr;
    p.first = 0;
    p.count = entries;
    if (per_transform_radius) HIP_TRY(ecc_launch_k01_radii(&p, m->transform_radii_d.ptr, K, ctx->stream));
    else HIP_TRY(ecc_launch_k01(&p, ctx->stream));
    HIP_TRY(launch_pairs_timed(ctx, &p));
    // ecc_metric_evaluate_pairs' choice for a list of `count` values (its one-launch path's host sum is the one-slice order)
    const int slices = ecc_sum::slices(count, m->sum_scratch_d.ptr != nullptr);
    hipLaunchKernelGGL(slices == 1 ? sum_transforms_kernel<1> : sum_transforms_kernel<SUM_SLICES>, dim3((unsigned)slices, (unsigned)K),
                       dim3(SUM_THREADS), 0, ctx->stream, m->pose_values_d.ptr, (long long)count, (long long)seg, m->pose_partial_d.ptr, out_dev);
    HIP_TRY(hipGetLastError());
    if (slices > 1) {
        hipLaunchKernelGGL(finish_transforms_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, ctx->stream, m->pose_partial_d.ptr,
                           slices, K, out_dev);
        HIP_TRY(hipGetLastError());
    }
    if (values)  // (transform-major on the device, seg floats apart)
        HIP_TRY(hipMemcpy2DAsync(values, sizeof(float) * (size_t)count, m->pose_values_d.ptr, sizeof(float) * (size_t)seg,
                                 sizeof(float) * (size_t)count, (size_t)K, hipMemcpyDeviceToHost, ctx->stream));
    rc = wait_pose_results(ctx, out, K, sums, "transform");
    if (rc) return rc;
    if (values) HIP_TRY(wait_stream_spin(ctx->stream));  // the copy behind the sums
    return ECC_OK;
}

}  // namespace
namespace ecc_internal {
// The transforms one at a time, the way a caller without these entry points does it -- the composed matrices, then
// evaluate_list(k, the cross list, its length): pair q = j n_source + i is (i, n_source + j, i, n_source + j) -- then the base again.
int transforms_sequential(ecc_metric* m, const std::vector<double>& base, int n_source, int n_transforms, const double* Ts,
                          const std::function<int(int, const int32_t*, int)>& evaluate_list)
{
    const int n = m->n_views, n_target = n - n_source;
    const int64_t count = (int64_t)n_source * n_target;
    if (count > std::numeric_limits<int>::max()) return fail(ECC_ERR_INVALID_ARGUMENT, "the index list of one transform is too long");
    std::vector<int32_t> idx(4 * (size_t)count);
    for (int j = 0; j < n_target; ++j)
        for (int i = 0; i < n_source; ++i) {
            int32_t* t = idx.data() + 4 * ((size_t)j * n_source + i);
            t[0] = t[2] = i;
            t[1] = t[3] = n_source + j;
        }
    std::vector<double> full(base);
    int rc = ECC_OK;
    for (int k = 0; k < n_transforms && !rc; ++k) {
        for (int i = 0; i < n_source; ++i)
            ecc_host::compose_transform(base.data() + 12 * (size_t)i, Ts + 16 * (size_t)k, full.data() + 12 * (size_t)i);
        rc = ecc_metric_set_projections(m, full.data(), n);
        if (!rc) rc = evaluate_list(k, idx.data(), (int)count);
    }
    const int rb = ecc_metric_set_projections(m, base.data(), n);
    return rc ? rc : rb;
}

// n_transforms transforms of `count` pairs each as batches of whole transforms within ECC_POSE_BATCH_MAX_ENTRIES grid entries, at
// most max_per_batch of them: run_batch(first transform, how many) each, which returns with the batch's results seen.
int transforms_batched(ecc_metric* m, int64_t count, int n_transforms, int64_t max_per_batch, const std::function<int(int64_t, int)>& run_batch)
{
    const bool was_quiet = m->quiet;
    ecc_mark_busy(m);
    const int64_t per_batch = std::min<int64_t>(std::max<int64_t>(ECC_POSE_BATCH_MAX_ENTRIES / count, 1), max_per_batch);
    for (int64_t k0 = 0; k0 < n_transforms; k0 += per_batch) {
        const int K = (int)std::min<int64_t>(per_batch, n_transforms - k0);
        const int rc = run_batch(k0, K);
        if (rc) return rc;
        m->last_batched_transforms += K;
    }
    HIP_TRY(wait_stream_spin(m->ctx->stream));  // (the results were seen before the stream's own completion; the scratch is reused)
    m->quiet = was_quiet;  // what was known to be complete before the call still is
    return ECC_OK;
}
}  // namespace ecc_internal

ECC_EXPORT void ecc_host_compose_transform(const double* P12, const double* T16, double* out12)
{
    double out[12];  // (out12 may be P12)
    ecc_host::compose_transform(P12, T16, out);
    std::memcpy(out12, out, sizeof(out));
}

ECC_EXPORT int ecc_metric_last_batched_transforms(const ecc_metric* m, int64_t* transforms)
{
    if (!m || !transforms) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    *transforms = m->last_batched_transforms;
    return ECC_OK;
}

ECC_EXPORT int ecc_metric_evaluate_transforms(ecc_metric* m, int n_source, int n_transforms, const double* Ts, double* means,
                                              float* pair_values)
{
    if (!m) return fail(ECC_ERR_INVALID_ARGUMENT, "metric is null");
    if (n_transforms < 0) return fail(ECC_ERR_INVALID_ARGUMENT, "n_transforms must not be negative");
    if (n_transforms > 0 && (!Ts || !means)) return fail(ECC_ERR_INVALID_ARGUMENT, "null argument");
    if (n_source < 1 || n_source >= m->n_views)
        return fail(ECC_ERR_INVALID_ARGUMENT, "n_source must be in [1, n_views): the views [0, n_source) are the source, the rest the target");
    if ((int)m->dtrs.size() != m->n_views)
        return fail(ECC_ERR_INVALID_ARGUMENT, "a registration needs one Radon intermediate per projection matrix");
    m->last_batched_transforms = 0;
    if (n_transforms == 0) return ECC_OK;
    int rc = set_device(m->ctx);
    if (rc) return rc;
    const int64_t n = m->n_views, count = (int64_t)n_source * (n - n_source);
    const double* Pcur = m->Ps_h[m->set_generation & 1].host;
    const std::vector<double> base(Pcur, Pcur + 12 * n);
    if (!m->pose_batching || count > ECC_POSE_BATCH_MAX_ENTRIES)
        return transforms_sequential(m, base, n_source, n_transforms, Ts, [&](int k, const int32_t* idx, int len) {
            return ecc_metric_evaluate_pairs(m, idx, len, pair_values ? pair_values + (size_t)k * count : nullptr, &means[k]);
        });
    std::vector<double> sums;
    return transforms_batched(m, count, n_transforms, TRANSFORM_BATCH_MAX, [&](int64_t k0, int K) -> int {
        sums.resize((size_t)K);
        const int e = run_batch(m, base.data(), n_source, K, Ts + 16 * (size_t)k0, sums.data(), pair_values ? pair_values + (size_t)k0 * count : nullptr);
        if (e) return e;
        for (int k = 0; k < K; ++k) means[k0 + k] = sums[k] / (double)count;  // ref: ...RadonIntermediate.cpp:224 (all weights are 1)
        return ECC_OK;
    });
}
