// ecc_capi_internal.h -- what the translation units of the C ABI share (ecc_capi.hip: errors, contexts; ecc_radon_api.hip: Radon
// intermediates; ecc_metric_api.hip: the metric's objects; ecc_evaluate.hip: its evaluation paths; ecc_preprocess_api.hip;
// ecc_direct_api.hip: MetricDirect): the object
// layouts behind the opaque handles, the kernel launchers, error handling and the helpers of namespace ecc_internal.
#ifndef ECC_CAPI_INTERNAL_H
#define ECC_CAPI_INTERNAL_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/ecc_hip.h"
#include "ecc_form_base.h"
#include "ecc_host_geometry.h"
#include "ecc_layout.h"
#include "ecc_view_changes.h"

extern "C" hipError_t ecc_launch_radon(const EccRadonParams* p, int derivative, hipStream_t stream);
extern "C" hipError_t ecc_launch_dtr_border(float* slabs, int64_t slab_stride, int n_img, int n_alpha, int n_t,
                                            int pitch, hipStream_t stream);
extern "C" hipError_t ecc_launch_ramp(float* slabs, int64_t slab_stride, int n_img, int n_alpha, int n_t, int pitch,
                                      const double* h2_d, hipStream_t stream);
extern "C" hipError_t ecc_launch_dtr_import(const float* src, float* slab, int n_alpha, int n_t, int pitch,
                                            hipStream_t stream);
extern "C" hipError_t ecc_launch_dtr_export(const float* slab, float* dst, int n_alpha, int n_t, int pitch,
                                            hipStream_t stream);
extern "C" hipError_t ecc_launch_build_paired(const float* const* slabs_tbl_d, float* paired_d, int64_t paired_stride, int n,
                                              int rows, int pitch, hipStream_t stream);
extern "C" hipError_t ecc_launch_build_quad(const float* const* slabs_tbl_d, float* quads_d, int64_t quad_stride_floats, int n,
                                            int rows, int pitch, hipStream_t stream);
extern "C" hipError_t ecc_launch_k01(const EccPairParams* p, hipStream_t stream);
extern "C" hipError_t ecc_launch_k01_radii(const EccPairParams* p, const float* radii_d, int period, hipStream_t stream);
extern "C" hipError_t ecc_launch_k01_patched(const EccPairParams* p, const EccSmallEval* x, hipStream_t stream);
extern "C" hipError_t ecc_launch_pairs(const EccPairParams* p, hipStream_t stream);
extern "C" int ecc_small_eval_plan(const EccPairParams* p, long long forced_bound, int* wpp, size_t* lds_bytes);
extern "C" hipError_t ecc_launch_small_eval(const EccPairParams* p, const EccSmallEval* x, hipStream_t stream);
extern "C" int ecc_small_poses_plan(const EccPairParams* p, int Q, int* wpp, size_t* lds_bytes);
extern "C" hipError_t ecc_launch_small_poses(const EccPairParams* p, const EccSmallEval* x, const EccSmallPoses* y, hipStream_t stream);
extern "C" hipError_t ecc_launch_preprocess(const EccPreprocessParams* p, hipStream_t stream);
extern "C" size_t ecc_preprocess_lds_bytes(int k);
extern "C" hipError_t ecc_launch_direct_views(const double* Ps_d, int n, EccDirectView* views, int n_u, int n_v,
                                              hipStream_t stream);
extern "C" hipError_t ecc_launch_direct_transpose(const float* src, float* dst, int n, int W, int H, hipStream_t stream);
extern "C" hipError_t ecc_launch_direct_batch(const EccDirectParams* p, double* total, hipStream_t stream);
extern "C" hipError_t ecc_launch_direct_list_batch(const EccDirectListParams* q, hipStream_t stream);
extern "C" hipError_t ecc_launch_direct_segment_sums(const double* vals, const int64_t* offsets, int n_segments, double* sums,
                                                     hipStream_t stream);
extern "C" hipError_t ecc_launch_pair_samples(const EccPairSamplesParams* p, hipStream_t stream);
extern "C" hipError_t ecc_launch_sum_pairs(const float* vals, long long count, double* out, void* scratch, hipStream_t stream);
extern "C" hipError_t ecc_launch_sum_pairs_to_host(const float* vals, long long count, double* out, float* values_host, hipStream_t stream);
extern "C" hipError_t ecc_launch_publish_scalar(const double* value_d, double* host_slot_dev, hipStream_t stream);
extern "C" size_t ecc_sum_scratch_bytes();
extern "C" hipError_t ecc_launch_pairs_weighted(const EccPairParams* p, const EccWeightedParams* g, hipStream_t stream);
extern "C" hipError_t ecc_launch_pairs_robust(const EccPairParams* p, const EccRobustParams* g, hipStream_t stream);
extern "C" hipError_t ecc_launch_pairs_weighted_robust(const EccPairParams* p, const EccWeightedRobustParams* g, hipStream_t stream);
extern "C" hipError_t ecc_launch_pairs_variance(const EccPairParams* p, const EccVarianceParams* g, hipStream_t stream);
extern "C" hipError_t ecc_launch_pairs_variance_robust(const EccPairParams* p, const EccVarianceRobustParams* g, hipStream_t stream);
// the segmented sums of columns 0 and 1 of a column-form buffer: per pose over all pairs with the pose's own entries substituted
// (weighted_poses_kernel.hip), per transform over its cross list (weighted_transforms_kernel.hip)
extern "C" hipError_t ecc_launch_sum_weighted_poses(const float* base_cols, long long base_stride, long long count, int n, int Q,
                                                    const int32_t* lists_d, int K, const float* val_cols, long long vals_stride, int slices,
                                                    double* partial_d, double* out_host_dev, hipStream_t stream);
extern "C" hipError_t ecc_launch_sum_weighted_transforms(const float* val_cols, long long col_stride, long long count, int K, int slices,
                                                         double* partial_d, double* out_host_dev, hipStream_t stream);
// the same sums over the S leading columns in one walk, results at word S k + col (form_sums_kernel.hip; S == 3, anything else is
// hipErrorInvalidValue)
extern "C" hipError_t ecc_launch_sum_form_poses(const float* base_cols, long long base_stride, long long count, int n, int Q,
                                                const int32_t* lists_d, int K, const float* val_cols, long long vals_stride, int S, int slices,
                                                double* partial_d, double* out_host_dev, hipStream_t stream);
extern "C" hipError_t ecc_launch_sum_form_transforms(const float* val_cols, long long col_stride, long long count, int K, int S, int slices,
                                                     double* partial_d, double* out_host_dev, hipStream_t stream);
// the T columns of a pose grid of c changed views (M_d: device, ascending) to the all-pairs positions of kept base columns
// (form_base_scatter_kernel.hip)
extern "C" hipError_t ecc_launch_form_base_scatter(const float* vals, long long vals_stride, int n, int c, const int32_t* M_d, int T,
                                                   float* base_cols, long long base_stride, hipStream_t stream);
extern "C" hipError_t ecc_launch_dilate_max(const float* src, float* dst, int64_t stride, int n_img, int n_u, int n_v, int radius,
                                            hipStream_t stream);
extern "C" hipError_t ecc_launch_clip_min(const float* lengths, int64_t lengths_stride, float* dst, int64_t dst_stride, int n_img,
                                          int n_alpha, int n_t, int pitch, int radius, float zero_at_px, hipStream_t stream);
extern "C" hipError_t ecc_launch_e1(const double* Ps_d, int n, float* PinvTs_d, float* Cs_d, hipStream_t stream);

#ifndef ECC_POSE_BATCH_MAX_ENTRIES
// grid entries (records of 296 bytes) per batch of ecc_poses.hip / ecc_transforms.hip: longer lists go in several batches
#define ECC_POSE_BATCH_MAX_ENTRIES (1 << 20)
#endif

#define ECC_EXPORT extern "C" __attribute__((visibility("default")))

// Thread-local message of the last failing call (ecc_last_error); defined in ecc_capi.hip.
extern "C" int ecc_set_error(int code, const char* msg);
namespace {
inline int fail(int code, const std::string& msg) { return ecc_set_error(code, msg.c_str()); }
}  // namespace

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            (void)hipGetLastError();                                                              \
            return fail(_e == hipErrorOutOfMemory ? ECC_ERR_OUT_OF_MEMORY : ECC_ERR_HIP,          \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                       \
        }                                                                                         \
    } while (0)

// Device slab shared by the dtrs of one batch; freed when the last handle goes away.
struct EccSlab {
    float* ptr = nullptr;
    int device = 0;
    ~EccSlab()
    {
        if (ptr) {
            (void)hipSetDevice(device);
            (void)hipFree(ptr);
        }
    }
};
typedef EccSlab Slab;

struct ecc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool timing = false;
    int radon_arithmetic = ECC_RADON_EXACT;  // ecc_radon_set_arithmetic
    int quad_copies = ECC_QUAD_COPIES_AUTO;  // ecc_ctx_set_quad_copies: whether metrics created from this context build row-quad copies
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // pair, radon, preprocess start/stop
    bool ev_valid[3] = {false, false, false};
    // trig table cache for the Radon kernel
    float* trig_d = nullptr;
    int trig_n_alpha = 0;
    // circular-convolution kernel of Filter::Ramp (2*n_t doubles), cached per n_t
    double* ramp_d = nullptr;
    int ramp_n_t = 0;
    // constant tables of the pair kernel's polynomial path
    EccPolyTables* poly_d = nullptr;
    // arena of ecc_preprocess, reused between calls and freed with the context: device tables + their pinned host
    // image (uploaded asynchronously; pre_ev marks the last upload, so the host image is not rewritten under a copy
    // in flight) and the scratch stack of the host-input / in-place forms
    char* pre_tables_d = nullptr;
    char* pre_tables_h = nullptr;
    size_t pre_tables_cap = 0;
    hipEvent_t pre_ev = nullptr;
    bool pre_ev_recorded = false;
    float* pre_scratch_d[2] = {nullptr, nullptr};
    size_t pre_scratch_cap[2] = {0, 0};
    // transposed copy of (a sub-batch of) the projection images for the Radon kernel's transposed tiles
    float* radon_T_d = nullptr;
    size_t radon_T_cap = 0;  // floats
    // one slab of scratch for ecc_radon_compute_linear
    float* linear_scratch_d = nullptr;
    size_t linear_scratch_cap = 0;  // floats
    // scratch of ecc_radon_line_weights*: the lengths of one sub-batch (at most 64 slabs), then its dilated images (dilate_px > 0)
    float* line_weights_scratch_d = nullptr;
    size_t line_weights_scratch_cap = 0;  // floats
};

struct ecc_dtr {
    ecc_ctx* ctx = nullptr;
    std::shared_ptr<Slab> owner;  // null when wrapping caller memory
    float* base = nullptr;
    int n_alpha = 0, n_t = 0, n_u = 0, n_v = 0, filter = 0, pitch = 0;
};

namespace ecc_internal {
hipError_t wait_stream_spin(hipStream_t stream);

// A device array the metric owns: grown on demand, freed with the metric (ecc_metric_destroy makes its device current first).
template <class T>
struct DeviceArray {
    T* ptr = nullptr;
    int64_t cap = 0;  // elements
    DeviceArray() = default;
    DeviceArray(const DeviceArray&) = delete;
    DeviceArray& operator=(const DeviceArray&) = delete;
    ~DeviceArray() { reset(); }
    void reset()
    {
        if (ptr) (void)hipFree((void*)ptr);
        ptr = nullptr;
        cap = 0;
    }
    // room for `need` elements: exactly that many, after the stream has drained when a smaller array is replaced
    int ensure(int64_t need, hipStream_t stream)
    {
        if (cap >= need && ptr) return ECC_OK;
        if (ptr) {
            HIP_TRY(hipStreamSynchronize(stream));
            HIP_TRY(hipFree((void*)ptr));
            ptr = nullptr;
            cap = 0;
        }
        HIP_TRY(alloc(need));
        return ECC_OK;
    }
    // the first allocation, for callers that report a failure themselves
    hipError_t alloc(int64_t n)
    {
        const hipError_t e = hipMalloc((void**)&ptr, (size_t)n * sizeof(T));
        if (e != hipSuccess) ptr = nullptr;
        cap = e == hipSuccess ? n : 0;
        return e;
    }
    int64_t bytes() const { return cap * (int64_t)sizeof(T); }
};

// A pinned host array mapped into the device's address space (zero-copy staging): host and device address of the same memory.
template <class T>
struct PinnedArray {
    T* host = nullptr;
    T* dev = nullptr;
    int64_t cap = 0;  // elements
    unsigned flags;
    explicit PinnedArray(unsigned alloc_flags = hipHostMallocMapped) : flags(alloc_flags) {}
    PinnedArray(const PinnedArray&) = delete;
    PinnedArray& operator=(const PinnedArray&) = delete;
    ~PinnedArray()
    {
        if (host) (void)hipHostFree(host);
    }
    // room for `need` elements: max(2 need, floor) of them, after the stream has drained when a smaller array is replaced
    // (a launch may still be reading it)
    int ensure(int64_t need, int64_t floor, hipStream_t stream)
    {
        if (cap >= need) return ECC_OK;
        if (host) {
            HIP_TRY(wait_stream_spin(stream));
            HIP_TRY(hipHostFree(host));
            host = dev = nullptr;
            cap = 0;
        }
        HIP_TRY(alloc(std::max<int64_t>(2 * need, floor)));
        return ECC_OK;
    }
    // the first allocation, for callers that report a failure themselves
    hipError_t alloc(int64_t n)
    {
        hipError_t e = hipHostMalloc((void**)&host, sizeof(T) * (size_t)n, flags);
        if (e != hipSuccess) host = nullptr;
        else e = hipHostGetDevicePointer((void**)&dev, host, 0);
        if (e == hipSuccess) cap = n;
        return e;
    }
};

// What an evaluation keeps for the next one of the same pair range: the range, the parameters it depends on (Key) and the
// matrices it was made from.  `valid` is set by the caller once everything that made it is enqueued.
template <class Key>
struct Kept {
    bool valid = false;
    int64_t first = 0, count = 0;
    int n_views = 0;
    Key key{};
    std::vector<double> Ps;
    bool matches(int64_t f, int64_t c, int n, const Key& k) const
    {
        return valid && first == f && count == c && n_views == n && key == k && (int64_t)Ps.size() == 12 * (int64_t)n;
    }
    void take(int64_t f, int64_t c, int n, const Key& k, const double* Pcur)
    {
        Ps.assign(Pcur, Pcur + 12 * (size_t)n);
        first = f;
        count = c;
        n_views = n;
        key = k;
    }
    void update(const std::vector<int>& views, const double* Pcur)
    {
        for (int v : views) std::memcpy(Ps.data() + 12 * (size_t)v, Pcur + 12 * (size_t)v, sizeof(double) * 12);
    }
};
// the kept records: the resolved sampling mode and the launch's float parameters
struct RecordKey {
    int mode;
    float radius, dkappa, tol;
    bool operator==(const RecordKey& o) const { return mode == o.mode && radius == o.radius && dkappa == o.dkappa && tol == o.tol; }
};
// the kept pair values: the metric's settings
struct ValueKey {
    int use_corr, sampling;
    double radius, dkappa;
    bool operator==(const ValueKey& o) const
    {
        return use_corr == o.use_corr && sampling == o.sampling && radius == o.radius && dkappa == o.dkappa;
    }
};
}  // namespace ecc_internal

// the kinds of robust map a metric can hold (ecc_robust_map.h); each kind's *_map_weights / *_map_variances call refuses the others
enum EccMapKind { ECC_MAP_PLAIN, ECC_MAP_WEIGHTED, ECC_MAP_VARIANCE };

struct ecc_metric {
    template <class T>
    using DeviceArray = ecc_internal::DeviceArray<T>;
    template <class T>
    using PinnedArray = ecc_internal::PinnedArray<T>;
    ecc_ctx* ctx = nullptr;
    std::vector<ecc_dtr*> dtrs;
    int n_alpha = 0, n_t = 0, n_u = 0, n_v = 0, pitch = 0;
    bool is_derivative = true;
    float step_alpha = 0, step_t = 0;
    // parameters
    double object_radius_mm = 0, dkappa = 0;
    int use_corr = 0;
    int sampling = ECC_SAMPLING_AUTO;  // ecc_metric_set_sampling
    // projections
    int n_views = 0;
    std::vector<double> P_first;  // first projection matrix (object radius estimate)
    // device state
    DeviceArray<const float*> dtr_table_d;     // the dtrs' slabs (borrowed)
    DeviceArray<float> paired_d;               // row-paired copies of all dtrs (owned; what the pair kernel samples)
    DeviceArray<const float*> paired_table_d;  // per dtr: base of its paired copy
    DeviceArray<float> quads_d;                // row-quad copies of all dtrs (owned; sampled by the pairs with kappa_max > pi/4), or none
    DeviceArray<const float*> quads_table_d;
    int64_t quad_floats = 0;                 // floats per row-quad copy
    std::vector<const float*> quads_table_h; // host image of quads_table_d
    bool quads_possible = false;             // offsets into a row-quad copy fit 32 bits
    bool quads_decided = true;               // ECC_QUAD_COPIES_AUTO: false until the first large evaluation has looked at the matrices
    DeviceArray<float> Cs_d;                 // 4 per view
    DeviceArray<float> PinvTs_d;             // 12 per view
    int geom_capacity = 0;                   // views Cs_d, PinvTs_d and Ps_h have room for
    DeviceArray<float> pair_values_d;
    DeviceArray<float> cost_d;
    DeviceArray<int32_t> indices_d;
    DeviceArray<float> K01_d;
    DeviceArray<EccPairRecord> records_d;  // per-pair geometry between k01_kernel and pairs_kernel
    DeviceArray<double> sum_d;
    DeviceArray<char> sum_scratch_d;  // partials + ticket of the multi-workgroup sum (zeroed; sum_kernel.hip)
    // pinned host staging, mapped into the device's address space (zero-copy: the 38 KB of matrices and the 8-byte
    // result cross PCIe inside the kernels, no copy commands).  Two matrix buffers, used alternately: an evaluate
    // call returns only after the stream has executed everything up to its result, so the buffer of the call before
    // the previous one is free without asking the stream (set_generation / done_generation below).
    PinnedArray<double> Ps_h[2];
    uint64_t set_generation = 0;   // number of e1 launches so far; launch g reads Ps_h[g & 1]
    uint64_t done_generation = 0;  // every e1 launch up to this one is known to have completed
    // 64-byte slot; [0] = the result, written by sum_pairs_kernel with a system-scope store
    PinnedArray<double> sum_h{hipHostMallocMapped | hipHostMallocCoherent};
    // ecc_metric_set_incremental: the pair values of the last evaluation of one pair range, the matrices and parameters
    // they belong to, and a pinned, device-mapped list buffer (4 indices + 1 slot per re-evaluated pair)
    int incremental = 0;
    ecc_internal::Kept<ecc_internal::ValueKey> cache;
    DeviceArray<float> cache_values_d;
    PinnedArray<int32_t> list_h;
    std::vector<int> scratch_changed;        // reused between evaluations (no heap traffic on the optimiser's path)
    ecc_view_changes::PairList scratch_pairs;
    int64_t last_evaluated_pairs = 0;
    // ecc_metric_set_record_reuse: the per-pair records (k01_kernel's output) of the last all-pairs / range evaluation
    // stay in records_d together with the matrices and parameters they belong to; the next evaluation of the same range
    // refits only the pairs with a changed matrix.  E1 is deferred to the evaluation for the same reason.
    int record_reuse = 1;
    bool e1_pending = false;   // matrices were staged since PinvTs_d / Cs_d were last known to be current (ensure_e1 finds out)
    // the matrices PinvTs_d / Cs_d on the device were made from, view by view (e1_kernel: all views; the patch lists of the
    // reuse path and of the one-launch path: the listed views)
    std::vector<double> dev_Ps;
    bool dev_valid = false;
    // automatic object radius (a function of the first matrix and the image size), kept until the first matrix changes
    mutable double radius_cache = 0.0;
    mutable double radius_cache_P[12] = {0};
    mutable bool radius_cache_valid = false;
    bool eager_e1 = false;     // the last range was too small for record reuse: set_projections launches e1_kernel itself
    ecc_internal::Kept<ecc_internal::RecordKey> rec;
    // pinned, device-mapped lists of the reuse path, two used alternately: per pair 4 indices + slot + 2 patch refs,
    // per changed view 16 floats + its index
    PinnedArray<int32_t> reuse_h[2];
    hipEvent_t reuse_ev[2] = {nullptr, nullptr};  // recorded after the k01 launch that read list b (asynchronous callers)
    bool reuse_ev_used[2] = {false, false};
    uint64_t reuse_gen = 0;
    std::vector<int> scratch_patched;
    std::vector<int> scratch_stale;     // views whose geometry on the device is behind the current matrices
    std::vector<int32_t> scratch_patch_of;
    // second stream of the reuse path: refit + list launch of the changed pairs run there while the all-pairs launch
    // (which skips them) already runs on the context's stream
    hipStream_t side_stream = nullptr;
    hipEvent_t fork_ev = nullptr, join_ev = nullptr;
    // ecc_metric_set_host_join: the synchronous all-pairs / range evaluations see join_ev complete on the host and then queue the
    // sum, instead of making the context's stream wait for it in front of the sum (ecc_evaluate.hip, wait_side_stream)
    int host_join = 1;
    // Everything this metric has queued on the context's stream or its side stream is KNOWN to have completed: set by the
    // synchronous evaluations once they have seen their result (the last thing they queued), cleared by whatever queues work for
    // the metric.  The two-stream refit then needs no fork event: what the side stream reads -- records, device geometry, the
    // row-paired copies, the pinned lists -- is written by this metric's own launches only, so nothing it must wait for is pending.
    // (hipEventRecord + hipStreamWaitEvent in front of the first launch cost the shard step of an 8-rank job 3.5-4.7 us of 72.)
    bool quiet = false;
    // What `quiet` may be set from: every call that queues work for the metric bumps queue_seq (ecc_mark_busy);
    // ecc_metric_publish_scalar remembers the value right after its own kernel.  ecc_metric_wait_scalar has only seen THAT kernel
    // complete -- in a pipelined order (async k, publish k, async k + 1, wait k) later work is still pending, and the wait
    // must not declare the metric quiet (advisor, round 5).
    uint64_t queue_seq = 0, publish_seq = 0, publish_generation = 0;
    // ecc_metric_set_small_eval: evaluations of at most ECC_SMALL_EVAL_MAX_PAIRS pairs as ONE launch (small_eval_kernel.hip).
    // E1 of the views whose matrix changed since the device arrays were made is done on the host and handed over in the
    // kernel arguments (dev_Ps above says which views those are).
    int small_eval = 1;
    int64_t small_max_pairs = -1;  // ecc_debug_set_small_eval_bound: >= 0 replaces the one-launch path's own size bound
    float economise_tol = ECC_POLY_ECONOMISE_TOL_BINS;  // ecc_debug_set_poly_tolerance
    PinnedArray<int32_t> sidx_h;  // index list of a fused index-list evaluation (4 per pair)
    PinnedArray<float> svals_h;   // pair values a caller wants on the host
    DeviceArray<unsigned> small_ticket_d;
    int64_t small_pending_count = 0;  // > 0: the result slot will receive the "done" word of a one-launch evaluation of that many pairs
    // ecc_metric_evaluate_pose_deltas (ecc_poses.hip): K poses as ONE record launch, ONE pair launch and ONE segmented sum.
    // Everything below is scratch of that path, grown on demand: the extended geometry (the base views, then one entry per
    // moved view of every pose), the pose-major x partner-major index grid, its records and values, the slice sums, and one
    // pinned, device-mapped block (extended matrices, the lists, the results).
    int pose_batching = 1;  // ecc_metric_set_pose_batching
    PinnedArray<char> pose_h;
    DeviceArray<float> pose_PinvTs_d;
    DeviceArray<float> pose_Cs_d;
    DeviceArray<int32_t> pose_idx_d;
    DeviceArray<EccPairRecord> pose_records_d;
    DeviceArray<float> pose_values_d;
    DeviceArray<double> pose_partial_d;
    DeviceArray<int32_t> pose_lists_d;
    int64_t last_batched_poses = 0;    // poses the last ecc_metric_evaluate_poses* call took through the batch (ecc_metric_last_batched_poses)
    // ecc_metric_evaluate_gradient (ecc_gradient.hip): the probes of one moved view as ONE record-and-sampling launch
    // (small_poses_kernel.hip) in front of the batch's segmented sum; it uses pose_values_d, pose_partial_d, pose_lists_d and pose_h.
    int gradient_launch = 0;     // ecc_debug_set_gradient_launch: off by default -- measured no faster than the pose batch
    int last_gradient_path = 0;  // ecc_metric_last_gradient_path
    // ecc_metric_evaluate_gram (ecc_gram.hip): records, pair entries (T columns) and slice sums of that call alone, grown on demand --
    // the call leaves the kept records and values above as they are
    DeviceArray<EccPairRecord> gram_records_d;
    DeviceArray<float> gram_values_d;
    DeviceArray<double> gram_partial_d;
    // ecc_metric_evaluate_view_coefficients (ecc_view_coeff.hip) shares the three arrays above and adds the coefficients on the
    // device and the per-(view, channel) sums of the gradient terms, K * n_views each
    DeviceArray<float> coeff_d;
    DeviceArray<double> coeff_sums_d;
    // ecc_metric_evaluate_view_hessian (ecc_view_hessian.hip) shares gram_records_d and has float64 scratch of its own: the T2
    // columns of pair-block entries (kept, like the Gram call's columns) and the (K n_views)^2 matrix (kept up to 64 MB, else freed
    // when the call returns)
    DeviceArray<double> view_moments_d;
    DeviceArray<double> view_hessian_d;
    // ecc_metric_evaluate_transforms (ecc_transforms.hip) uses the scratch above (pose_lists_d: its value slots) and, under the
    // automatic object radius, one float per transform of a batch
    DeviceArray<float> transform_radii_d;
    int64_t last_batched_transforms = 0;  // ecc_metric_last_batched_transforms
    // ecc_metric_evaluate_robust_map (ecc_robust_map.hip): the fixed-point planes of a call (zeroed per call, grown geometrically), the
    // per-intermediate plane table, and the float planes of the LAST map call -- HITS of every mapped view, then REJ -- which
    // ecc_metric_robust_map_weights reads; dropped (map_valid) by ecc_metric_refresh_dtrs and ecc_metric_set_params
    DeviceArray<unsigned long long> map_fixed_d;
    DeviceArray<int32_t> map_slot_d;
    DeviceArray<float> map_planes_d;
    int map_n_mapped = 0;
    bool map_valid = false;
    // which kind of map is held: the n-metric's, ecc_metric_evaluate_weighted_robust_map's (ecc_weighted_robust_map.hip: deposits
    // under the line weights of a 2 n metric) or ecc_metric_evaluate_variance_robust_map's (ecc_variance_robust_map.hip: the loss in
    // sigma units, deposits in count units); map_slot_d is the plane table (map_n_slots entries), then the mapped intermediates
    EccMapKind map_kind = ECC_MAP_PLAIN;
    int map_n_slots = 0;
    // ecc_metric_evaluate_residual_histogram (ecc_residual_histogram.hip): the n_views x n_bins table of a call, zeroed per call
    DeviceArray<unsigned long long> histogram_d;
    // ecc_metric_set_form_incremental (ecc_form_call.h): the T base columns of the last *_pose_deltas call of a form
    // family, col_stride apart as that call's columns are in gram_values_d, with the form, the parameters and the matrices they belong
    // to (ecc_form_base.h); the all-pairs, list, map and Gram calls keep to gram_values_d and neither see nor disturb them.  Dropped
    // (ecc_drop_form_base) wherever cache.valid is dropped for a data or parameter reason, and by a change of n_views.
    int form_incremental = 0;
    ecc_internal::Kept<ecc_form_base::Key> form_base;
    DeviceArray<float> form_base_d;
    int64_t last_form_base_pairs = 0;  // base pairs the last *_pose_deltas call of a form family evaluated (ecc_metric_last_form_base_pairs)
    // ecc_debug_step_stamps: host clock (seconds, steady) at fixed points of the last set_projections / synchronous evaluation
    double stamps[ECC_STEP_STAMPS] = {0};
};

inline void ecc_mark_busy(ecc_metric* m)
{
    m->quiet = false;
    ++m->queue_seq;
}

inline void ecc_drop_form_base(ecc_metric* m) { m->form_base.valid = false; }

inline void ecc_stamp(ecc_metric* m, int k)
{
    m->stamps[k] = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

namespace ecc_internal {

// ecc_radon_api.hip, for ecc_line_weights.hip: the range checks of the Radon calls; the Radon launches of a stack on the context's stream
int radon_check_args(ecc_ctx* ctx, const float* image, int n, int n_u, int n_v, int n_alpha, int n_t, int filter, int post,
                     ecc_dtr** out);
int radon_launch_stack(ecc_ctx* ctx, const float* images_d, int n, int n_u, int n_v, int n_alpha, int n_t, int filter, int post,
                       float* slabs, int64_t slab_stride);
// ecc_line_weights.hip: n line-weight handles (FILTER_NONE) over one slab stack, slab k at owner->ptr + k * ecc_layout_floats
int make_weight_handles(ecc_ctx* ctx, const std::shared_ptr<Slab>& owner, int n, int n_alpha, int n_t, int n_u, int n_v, ecc_dtr** out);
void arm_result(ecc_metric* m);
hipError_t wait_result(ecc_metric* m, hipStream_t stream, double* value);
int set_device(const ecc_ctx* ctx);
int ensure_poly_tables(ecc_ctx* ctx);
void decide_quad_copies(ecc_metric* m);  // ECC_QUAD_COPIES_AUTO: build the row-quad copies if the current matrices' pairs would read them
int ensure_e1(ecc_metric* m);  // E1 on the device for the staged matrices, if the device arrays are behind them
// ecc_evaluate.hip: the parameters of a launch; the stream-ordered launches over a pair range; the pose-delta path
int fill_pair_params(ecc_metric* m, EccPairParams* p, int64_t mode_count, bool need_e1 = true);
int launch_range(ecc_metric* m, int64_t first, int64_t count, float* pair_values_d, float* cost_d, float* K01_d, double* sum_d,
                 bool synchronous = false, bool host_join = false);
int evaluate_cached(ecc_metric* m, int64_t first, int64_t count, double* sum_d, float** vals_out);

// ecc_poses.hip: the segmented sum behind a batch's pair launch and the wait for its results; whether a pose keeps the base's
// (automatic) object radius
int sum_poses(ecc_metric* m, const float* base_vals_d, int K, int Q, volatile uint64_t* out, double* out_dev, double* sums);
bool pose_keeps_radius(const ecc_metric* m, double base_radius, int c, const int32_t* views, const double* moved_Ps);
// ecc_poses.hip, for the batches of ecc_form_call.h as well: the lists' checks; the host half of a batch's grid (pinned block,
// device arrays) and the launch of pose_list_kernel over it; the result slots' sentinel and the bounded wait for them
int check_lists(const ecc_metric* m, int n_poses, const int32_t* off, const int32_t* views);
int stage_pose_grid(ecc_metric* m, const double* base, int K, const int32_t* off, const int32_t* views, const double* moved_Ps,
                    int result_words, volatile uint64_t** out, double** out_dev);
hipError_t launch_pose_list(ecc_metric* m, int K, int Q, int result_words);
void arm_pose_results(volatile uint64_t* out, int K);
int wait_pose_results(ecc_ctx* ctx, volatile uint64_t* out, int K, double* sums, const char* batch_noun = "pose");
// ecc_poses.hip: the poses `rest` of a pose-delta call the sequential way -- the pose's full matrices, evaluate_pose(k), the
// matrices back -- then the base again
int pose_deltas_sequential(ecc_metric* m, const std::vector<int>& rest, const int32_t* off, const int32_t* views, const double* moved_Ps,
                           const std::function<int(int)>& evaluate_pose);
// ecc_transforms.hip, for the batches of ecc_form_call.h as well: the object radius the sequential calls would take for a
// transform; the host half of a batch's grid (pinned block, device arrays) and the launch of transform_list_kernel over it; the
// two drivers of a call -- the transforms one at a time over the cross list, then the base again; whole transforms in batches of at
// most max_per_batch within ECC_POSE_BATCH_MAX_ENTRIES grid entries, run_batch(first transform, how many) each
float radius_of_transform(const ecc_metric* m, const double* base, const double* T);
int stage_transform_grid(ecc_metric* m, const double* base, int n_source, int K, const double* Ts, int result_words,
                         volatile uint64_t** out, double** out_dev);
hipError_t launch_transform_list(ecc_metric* m, int n_source, int K, long long seg, int result_words);
int transforms_sequential(ecc_metric* m, const std::vector<double>& base, int n_source, int n_transforms, const double* Ts,
                          const std::function<int(int, const int32_t*, int)>& evaluate_list);
int transforms_batched(ecc_metric* m, int64_t count, int n_transforms, int64_t max_per_batch, const std::function<int(int64_t, int)>& run_batch);
// ecc_gram.hip: what the channel forms (Gram, view coefficients, view Hessian) need of n_channels and of the metric, with the call's
// own texts for the range of n_channels and for the correlation cost
int channel_form_check(const ecc_metric* m, int n_channels, const char* range_text, const char* corr_text);
// ecc_weighted.hip: the argument checks of the weighted calls
int weighted_check(const ecc_metric* m);
// ecc_robust.hip: the argument checks of the robust calls (value: the required result pointer)
int robust_check(const ecc_metric* m, const double* value, int loss, float delta);
// ecc_weighted_robust.hip: robust_check's conditions, then weighted_check's
int weighted_robust_check(const ecc_metric* m, const double* value, int loss, float delta);
// ecc_variance.hip: weighted_check's conditions on the metric and a finite floor > 0, in the order include/ecc_hip.h states
int variance_check(const ecc_metric* m, float floor);
// ecc_variance_robust.hip: the robust calls' conditions on value, loss and delta, then variance_check's
int variance_robust_check(const ecc_metric* m, const double* value, int loss, float delta, float floor);

// The distance of two channels' row-paired and row-quad copies, for the pair forms that read more than one copy per view (g: any
// of their parameter structs).
template <class Params>
inline void set_channel_strides(const ecc_metric* m, Params* g)
{
    const int64_t n = m->n_views;
    const int64_t paired_bytes = (int64_t)(m->n_alpha + 1) * m->pitch * 2 * (int64_t)sizeof(float);
    g->paired_channel_bytes = n * paired_bytes;
    g->quad_channel_bytes = n * m->quad_floats * (int64_t)sizeof(float);
}

// The planes of the metric's map call, for the three map forms (g: any parameter struct of ecc_robust_map.h): the fixed-point
// planes, the plane table, a plane's cells (ecc_robust_map_plane_cells: one per float of a slab) and the REJ planes behind all
// HITS planes.
template <class Params>
inline void set_map_planes(const ecc_metric* m, Params* g)
{
    g->planes = m->map_fixed_d.ptr;
    g->slot_of = m->map_slot_d.ptr;
    g->plane_cells = ecc_layout_floats(m->n_alpha, m->n_t);
    g->rej_cells = (int64_t)m->map_n_mapped * g->plane_cells;
}

// launch(stream) on the context's stream between its timing events (ecc_ctx_enable_timing).
template <class Launch>
inline hipError_t launch_timed(ecc_ctx* ctx, Launch&& launch)
{
    if (ctx->timing) {
        const hipError_t e = hipEventRecord(ctx->ev[0], ctx->stream);
        if (e != hipSuccess) return e;
    }
    const hipError_t e = launch(ctx->stream);
    if (e != hipSuccess || !ctx->timing) return e;
    const hipError_t e1 = hipEventRecord(ctx->ev[1], ctx->stream);
    if (e1 == hipSuccess) ctx->ev_valid[0] = true;
    return e1;
}

// The pair launch p -- or, with x, the one-launch evaluation -- between those events.
inline hipError_t launch_pairs_timed(ecc_ctx* ctx, const EccPairParams* p, const EccSmallEval* x = nullptr)
{
    return launch_timed(ctx, [&](hipStream_t s) { return x ? ecc_launch_small_eval(p, x, s) : ecc_launch_pairs(p, s); });
}

}  // namespace ecc_internal

#endif
