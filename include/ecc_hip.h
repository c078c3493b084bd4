/*
 * ecc_hip.h -- C ABI of the MI355X-native epipolar-consistency hot path (libecc_hip.so).
 *
 * Drop-in boundary for the reference's Radon-intermediate + pair-consistency path
 * (aaichert/EpipolarConsistency 1.2.2).  Plain C: opaque handles, raw pointers, int32 sizes,
 * every function returns an int status (0 = ECC_OK), no exceptions, no exit().  Citations are
 * relative to /root/reference/code/.  The reference-side bindings (what a maintainer adds to
 * RadonIntermediate.cpp / EpipolarConsistencyRadonIntermediate.cpp) are shown in INTEGRATION.md;
 * a header-only C++ adapter with the reference's class names lives in
 * epipolarconsistency_amd/cpp/EpipolarConsistencyHip.hxx.
 *
 * Layout contracts (same as the reference unless stated):
 *   - projection images: row-major float32, x (u) fastest, n_u x n_v;
 *   - Radon intermediate ("dtr") as seen through this API: n_t rows x n_alpha columns float32,
 *     alpha fastest, idx = iy*n_alpha + ix            (ref: LibEpipolarConsistency/RadonIntermediate.cu:44);
 *   - projection matrices: 3x4 float64 column-major, 12 doubles per view (Eigen default; the
 *     reference passes Ps[i].data(), ref: ...RadonIntermediate.cpp:148);
 *   - cost image: n x n float32, entry (i,j), i<j at index i + j*n; other entries untouched
 *     (ref: EpipolarConsistencyRadonIntermediate.cu:250,269; .cpp:183,214-221);
 *   - index lists: int32 x 4 per pair = (P0, P1, dtr0, dtr1)    (ref: ...RadonIntermediate.cu:49-50,202).
 * Device-resident dtrs are kept in a private transposed+padded layout (ECC_LAYOUT_T_FAST, see
 * DESIGN.md "Data layout in HBM"); ecc_dtr_readback/ecc_dtr_from_host convert.
 */
#ifndef ECC_HIP_H
#define ECC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ECC_HIP_VERSION 100 /* 1.0.0 */

/* status codes */
enum {
    ECC_OK = 0,
    ECC_ERR_INVALID_ARGUMENT = 1,
    ECC_ERR_HIP = 2,          /* a HIP runtime call failed: see ecc_last_error() */
    ECC_ERR_OUT_OF_MEMORY = 3,
    ECC_ERR_NO_DEVICE = 4,
    ECC_ERR_UNSUPPORTED = 5
};

/* RadonIntermediate::Filter / ::PostProcess (ref: LibEpipolarConsistency/RadonIntermediate.h:21-29) */
enum { ECC_FILTER_DERIVATIVE = 0, ECC_FILTER_RAMP = 1, ECC_FILTER_NONE = 2 };
enum { ECC_POST_IDENTITY = 0, ECC_POST_SQUARE_ROOT = 1, ECC_POST_LOGARITHM = 2 };

typedef struct ecc_ctx ecc_ctx;       /* one per (device, stream) */
typedef struct ecc_dtr ecc_dtr;       /* one Radon intermediate  (ref: class RadonIntermediate) */
typedef struct ecc_metric ecc_metric; /* ref: class MetricRadonIntermediate */

/* Thread-local message of the last failing call on this thread ("" if none). */
const char* ecc_last_error(void);
int ecc_version(void);
/* Number of HIP devices visible (0 when there is none; never fails). */
int ecc_device_count(void);

/* Environment variables the library reads -- two, both optional, neither changes a result; each is described next to
 * the entry point it affects:
 *   ECC_RECORD_REUSE = 0 | 1 | 2   default of ecc_metric_set_record_reuse for new metrics   (see ecc_metric_set_record_reuse)
 *   ECC_EXCHANGE_TIMEOUT_S         time-out of ecc_exchange_sum in seconds, default 60      (see ecc_exchange_open)
 * (the header-only C++ adapter additionally reads ECC_HIP_DEVICES: the devices of its process-wide default group).
 * Experiment hooks are explicit calls (ecc_debug_*, last section of this header), never environment variables: the
 * variables of earlier versions -- ECC_POLY_TOL, ECC_SMALL_MAX_PAIRS, ECC_SMALL_DEBUG, ECC_RESULT_WAIT, ECC_QUAD_COPIES --
 * are ignored (tests/test_gpu_env_hooks.py). */

/* ---- context ------------------------------------------------------------------------------ */
/* `stream` is a hipStream_t (may be NULL = the device's default stream).  All launches and
 * copies of objects created from this context are ordered on it.  Replaces the reference's
 * implicit "current device, default stream, cudaDeviceSynchronize after every launch". */
int ecc_ctx_create(int device, void* stream, ecc_ctx** out);
/* Destroy every dtr / metric created from a context BEFORE the context itself (they keep a pointer to it). */
int ecc_ctx_destroy(ecc_ctx* ctx);
int ecc_ctx_synchronize(ecc_ctx* ctx);

/* ---- Radon intermediate (R1/R2) ------------------------------------------------------------ */
/* Replaces computeDerivLineIntegrals(tex, n_x, n_y, n_alpha, n_t, filter, post, out_d)
 * (ref: LibEpipolarConsistency/RadonIntermediate.cu:149-170) and the ctor
 * RadonIntermediate(ImageView<float>, size_alpha, size_t, filter, post) (ref: RadonIntermediate.cpp:17-31).
 * `image` is n_u*n_v floats on the host (image_on_device = 0) or on ctx's device (= 1).
 * ECC_FILTER_RAMP: plain line integrals followed by the ramp filter along t of apply1DRampFilter
 * (ref: RadonIntermediate.cu:173-237), evaluated as the exact circular convolution the two cuFFT
 * calls amount to (binary64 accumulation, no FFT library). */
int ecc_radon_compute(ecc_ctx* ctx, const float* image, int image_on_device, int n_u, int n_v,
                      int n_alpha, int n_t, int filter, int post_process, ecc_dtr** out);

/* Same for a stack of n images (n*n_u*n_v floats); writes n handles to out[0..n).  The n dtrs
 * share one device slab; each handle is destroyed separately.  Work is asynchronous on the
 * context's stream. */
int ecc_radon_compute_batch(ecc_ctx* ctx, const float* images, int images_on_device, int n, int n_u,
                            int n_v, int n_alpha, int n_t, int filter, int post_process,
                            ecc_dtr** out);

/* Device-to-device form for callers that own both buffers (e.g. torch tensors): images_d holds n
 * images, slabs_d receives n dtrs in the private layout (ecc_dtr_slab_floats(n_alpha, n_t) floats
 * each, written completely incl. the replicated border).  Asynchronous on the context's stream;
 * adopt the result with ecc_dtr_wrap_device.  A metric that already holds handles on these slabs keeps
 * sampling its snapshot of the old contents until ecc_metric_refresh_dtrs (see there). */
int ecc_radon_compute_into(ecc_ctx* ctx, const float* images_d, int n, int n_u, int n_v, int n_alpha,
                           int n_t, int filter, int post_process, float* slabs_d);

/* Arithmetic convention of the Radon kernel's sampling loop (per context; default ECC_RADON_EXACT).
 *   ECC_RADON_EXACT: every float expression of ref: RadonIntermediate.cu:118-123 and of the bilinear rule
 *     ((1 - fx) * T00 + fx * T10, ...) rounded separately, source order -- the CPU reading of the source; results are
 *     bit-identical to the oracle's normative variant.
 *   ECC_RADON_FMA: the loop body contracted -- positions fmaf(t, d, o), lerps as T00 + fx * (T10 - T00) with one fused
 *     multiply-add each (3 differences + 3 fma instead of 11 operations per sample).  This is the arithmetic class of
 *     the reference's own GPU build, which interpolates in texture hardware (ref: LibUtilsCuda/CudaBindlessTexture.cpp:
 *     25-39) and whose compiler contracts o + t * d; results are bit-identical to the oracle's contracted variant
 *     (eccor_set_radon_contract(1)) and move the ECC metric by less than 2e-6 relative (tests/test_gpu_radon_fma.py,
 *     DESIGN.md 4.1).  About 25 % faster.
 * The per-bin set-up (line, clipping, bounds test), the accumulation order and the post-process are the same in both. */
enum { ECC_RADON_EXACT = 0, ECC_RADON_FMA = 1 };
int ecc_radon_set_arithmetic(ecc_ctx* ctx, int mode);
int ecc_radon_get_arithmetic(const ecc_ctx* ctx, int* mode);

/* The reference's launcher seam, device memory in and out (Option B): replaces
 *   void computeDerivLineIntegrals(cudaTextureObject_t in, int n_x, int n_y, int n_alpha, int n_t, int filter, int post, float* out_d)
 * (ref: RadonIntermediate.cpp:12, RadonIntermediate.cu:149-170) with the image as a linear device buffer in place of the
 * texture.  out_linear_d receives the result in the REFERENCE's layout: n_t rows of n_alpha floats, angle fastest,
 * n_t * n_alpha floats -- the buffer RadonIntermediate::compute allocates (ref: RadonIntermediate.cpp:208) and readback
 * copies verbatim (:148-163).  Stream-ordered. */
int ecc_radon_compute_linear(ecc_ctx* ctx, const float* image_d, int n_u, int n_v, int n_alpha, int n_t, int filter,
                             int post_process, float* out_linear_d);
/* A Radon intermediate from device memory in the reference's layout: what RadonIntermediate::getTexture turns into a
 * texture (ref: RadonIntermediate.cpp:188-196) -- a snapshot, as there. */
int ecc_dtr_from_device_linear(ecc_ctx* ctx, const float* data_d, int n_alpha, int n_t, int n_u, int n_v, int filter,
                               ecc_dtr** out);

/* Wraps existing host data (alpha-fast, n_t x n_alpha), ref: RadonIntermediate(ImageView<float>)
 * + replaceRadonIntermediateData (RadonIntermediate.cpp:69-80,105-123). */
int ecc_dtr_from_host(ecc_ctx* ctx, const float* data, int n_alpha, int n_t, int n_u, int n_v,
                      int filter, ecc_dtr** out);
/* ref: RadonIntermediate::readback (RadonIntermediate.cpp:148-163); host gets alpha-fast data. */
int ecc_dtr_readback(ecc_dtr* dtr, float* host_out);
/* Getters, ref: RadonIntermediate.cpp:130-133,165-178.  bin_size_angle = Pi/n_alpha,
 * bin_size_distance = sqrt(n_u^2+n_v^2)/n_t (RadonIntermediate.cpp:204-206). */
int ecc_dtr_info(const ecc_dtr* dtr, int* n_alpha, int* n_t, int* n_u, int* n_v, int* filter,
                 double* bin_size_angle, double* bin_size_distance);
/* Device pointer + pitch of the private layout: element (ix, iy) lives at
 * base[(ix + 1) * pitch + (iy + 1)], rows -1 and n_alpha and columns -1 and n_t replicate the
 * border (clamp addressing).  For callers that want to all-gather dtrs between GPUs. */
int ecc_dtr_device_view(const ecc_dtr* dtr, float** base, int* pitch, int* rows);
/* Size in floats of one dtr in the private layout, so that a caller (e.g. torch) can own the slab. */
int64_t ecc_dtr_slab_floats(int n_alpha, int n_t);
/* Adopt caller-owned device memory already holding a dtr in the private layout (no copy, no free).  The handle
 * aliases the caller's memory: see ecc_metric_refresh_dtrs for what a metric sees when the memory changes. */
int ecc_dtr_wrap_device(ecc_ctx* ctx, float* base, int n_alpha, int n_t, int n_u, int n_v, int filter,
                        ecc_dtr** out);
int ecc_dtr_destroy(ecc_dtr* dtr);

/* ---- line weights from a flagged-pixel image, made on the device ----------------------------- */
/* The weight intermediates of ecc_metric_evaluate_weighted (below) from images that are 1 where a pixel must not be trusted and 0
 * elsewhere, without a host round trip (csrc/ecc_line_weights.hip, csrc/line_weights_kernel.hip).  For one flagged
 * image F of n_v x n_u:
 *   1. D = F if dilate_px = 0, else D(y, x) = the maximum of F over the (2 dilate_px + 1)^2 square around (y, x), indices clamped
 *      to the image;
 *   2. L = the ECC_FILTER_NONE / ECC_POST_IDENTITY Radon intermediate of D on n_alpha x n_t bins -- the launches of
 *      ecc_radon_compute_batch in the context's arithmetic mode: the length in pixels of every bin's line inside flagged pixels;
 *   3. w = min(max(1.0f - L / zero_at_px, 0.0f), 1.0f): one binary32 division, one subtraction, no reciprocal, no contraction;
 *   4. W(ix, iy) = the minimum of w over the (2 guard_bins + 1)^2 bins around (ix, iy), indices clamped to the grid: with
 *      guard_bins >= 1 a bilinear sample with a weight above 0 touches no bin with L >= zero_at_px;
 *   5. W is written as a complete slab of the private layout: elements, replicated border, zeros in the pitch padding.
 * Caps: 0 <= dilate_px <= 16, 0 <= guard_bins <= 8, zero_at_px finite and positive.  Inputs are finite; NaNs are unspecified.
 * The results have the bits of the Python layer's line_weights (readback, numpy, ecc_dtr_from_host) on the dilated image. */
typedef struct ecc_line_weights_config { int32_t dilate_px; int32_t guard_bins; float zero_at_px; } ecc_line_weights_config;
void ecc_line_weights_defaults(ecc_line_weights_config* cfg);          /* 0, 1, 1.0f: line_weights' defaults */
/* cfg == NULL means the defaults.
 * ecc_radon_line_weights: n flagged images on the host (on_device = 0) or on ctx's device (= 1) -> n handles in out[0..n) that share
 *   one slab stack, as ecc_radon_compute_batch's do; they report ECC_FILTER_NONE.
 * ecc_radon_line_weights_into: the asynchronous device-to-device form for caller-owned slabs, with the argument shape and semantics
 *   of ecc_radon_compute_into -- the per-frame path of a tracker whose mask moves: follow it with
 *   ecc_metric_refresh_dtrs(m, n_views + i, 1).  Every float of the n slabs is written.
 * ecc_dtr_line_weights: steps 3 to 5 alone, for a caller who already holds a length intermediate (e.g. from a file); dilate_px is
 *   not applied (the caps of the whole config are still checked).  `lengths` must have ECC_FILTER_NONE and live on ctx's device.
 * Errors, before any launch, allocation or write, ECC_ERR_INVALID_ARGUMENT: ctx == NULL (checked first); null images, output or
 * slabs; the range checks of ecc_radon_compute_batch; a config outside the caps (a NaN or non-positive zero_at_px included).
 * Scratch (kept in the context): the lengths, and with dilate_px > 0 the dilated images, of at most 64 views; larger stacks go
 * through it 64 views at a time on the context's stream. */
int ecc_radon_line_weights(ecc_ctx* ctx, const float* flagged, int on_device, int n, int n_u, int n_v,
                           int n_alpha, int n_t, const ecc_line_weights_config* cfg, ecc_dtr** out);
int ecc_radon_line_weights_into(ecc_ctx* ctx, const float* flagged_d, int n, int n_u, int n_v,
                                int n_alpha, int n_t, const ecc_line_weights_config* cfg, float* slabs_d);
int ecc_dtr_line_weights(ecc_ctx* ctx, const ecc_dtr* lengths, const ecc_line_weights_config* cfg, ecc_dtr** out);

/* ---- projection pre-processing (the step in front of R1) ------------------------------------- */
/* ref: struct EpipolarConsistency::PreProccess (Gui/PreProccess.h:14-50), same fields and defaults
 * (ecc_preprocess_defaults).  Offsets in zero/feather are left, right, bottom, top; blanks are
 * n_blanks x 4 int32 (x0, y0, x1, y1) on the host. */
typedef struct ecc_preprocess_config {
    int32_t process;            /* 1: run PreProccess::process; 0: cosine weighting only            */
    int32_t normalize;          /* Intensity/Normalize                                               */
    double bias, scale;         /* Intensity/Bias, Intensity/Scale                                   */
    int32_t apply_log;          /* Intensity/Apply Minus Logarithm                                   */
    double gaussian_sigma;      /* Lowpass Filter/Gaussian Sigma   (1.84)                            */
    int32_t half_kernel_width;  /* Lowpass Filter/Half Kernel Width (5); at most 16 here            */
    int32_t flip_u, flip_v;     /* Geometry/Flip u-Axis, Flip v-Axis                                 */
    int32_t zero[4];            /* Border/Zero Border (1,1,1,1)                                      */
    int32_t feather[4];         /* Border/Feather (16,16,16,16)                                      */
    int32_t n_blanks;
    const int32_t* blanks;      /* Border/Blanks                                                     */
} ecc_preprocess_config;
void ecc_preprocess_defaults(ecc_preprocess_config* cfg);

/* ref: PreProccess::process(img) followed by PreProccess::apply_weight_cos_principal_ray(img, P)
 * (Gui/PreProccess.cpp:57-166; call order of Gui/InputDataDirect.cpp:85-86) for a stack of n images, as ONE
 * fused device kernel (intensity, border zero/feather, blanks, flips, Gaussian low-pass with the reference's
 * dropped last tap, cosine weight).  images / out: n * n_u * n_v floats, both on the host
 * (on_device = 0) or both on ctx's device (= 1); out may equal images (in place, like the reference).
 * Ps: n x 12 float64 column-major or NULL (no cosine weighting; an all-zero matrix skips that view,
 * PreProccess.cpp:149).  on_device = 1: asynchronous on the context's stream, in place (through a scratch stack kept
 * in the context) or out of place; `out` must be identical to `images` or disjoint from it (partial overlap is
 * rejected: tiles read halos of their neighbours).  on_device = 0 returns with `out` filled. */
int ecc_preprocess(ecc_ctx* ctx, const float* images, int on_device, float* out, int n, int n_u, int n_v,
                   const ecc_preprocess_config* cfg, const double* Ps);
/* K(0,0), K(0,2), K(1,2) of P = K[R|t] (ref: getCameraIntrinsics, ProjectionMatrix.cpp:61-67). */
void ecc_host_intrinsics(const double* P, float* sdd_px, float* ppu, float* ppv);

/* ---- metric (E1..E5) ----------------------------------------------------------------------- */
/* ref: MetricRadonIntermediate(Ps, dtrs) / setRadonIntermediates (…RadonIntermediate.cpp:53-66,87-106).
 * The metric borrows the dtrs ("DO NOT delete or change _dtrs during lifetime", .h:45).  Sizes and
 * the derivative flag are taken from dtrs[0] only, as the reference does (.cpp:92-98). */
int ecc_metric_create(ecc_ctx* ctx, int n_dtrs, ecc_dtr* const* dtrs, ecc_metric** out);
int ecc_metric_destroy(ecc_metric* m);
/* SNAPSHOT SEMANTICS.  ecc_metric_create copies every dtr into a private row-paired layout and the
 * all-pairs / range / index-list evaluations in the polynomial and per-sample modes sample THOSE copies: new slab
 * contents (ecc_radon_compute_into into the same slabs, an image-domain correction loop) are not seen until
 * ecc_metric_refresh_dtrs(m, first, count) re-copies dtrs [first, first + count) -- asynchronous on the context's
 * stream, ~1 us per dtr, ordered behind the kernels that wrote the slabs when they ran on the same stream.
 * ECC_SAMPLING_REFERENCE and ecc_metric_evaluate_for_image_pair read the slabs themselves (always current).  The
 * handles must stay alive for the metric's lifetime either way ("DO NOT delete or change _dtrs", ref: .h:45). */
int ecc_metric_refresh_dtrs(ecc_metric* m, int first, int count);

/* ref: MetricRadonIntermediate::setProjectionMatrices (…RadonIntermediate.cpp:134-163): per view
 * (P^+)^T and the source position in float64 (same Householder-QR arithmetic as
 * culaut/xprojectionmatrix.hxx:20-52,93-105), cast to float32.  The n x 12 doubles are uploaded
 * asynchronously and the pre-compute runs on the device, one thread per view (bit-identical to
 * ecc_host_pinvT / ecc_host_source_position). */
int ecc_metric_set_projections(ecc_metric* m, const double* Ps, int n_views);
/* The reference's launcher seam for the metric (Option B): what
 *   void epipolarConsistency(int n_x, int n_y, int num_dtrs, char* dtrs_d, int n_alpha, int n_t, float step_alpha, float step_t,
 *                            int num_Ps, float* Cs_d, float* PinvTs_d, int num_pairs, int* indices_d, float* K01s_d, float* out_d,
 *                            float object_radius_mm, float dkappa, bool isDerivative, bool use_corr, float* out_corr_d)
 * (ref: EpipolarConsistencyRadonIntermediate.cpp:16-37, .cu:300-409) does with the caller's device buffers: Cs_d / PinvTs_d
 * are the per-view geometry the caller's host class made (ref: ...RadonIntermediate.cpp:134-163), indices_d the optional
 * int4 list, K01s_d (nullable) the 16 floats per pair, out_d the n x n cost image (all pairs: entry i + j n, i < j; the rest
 * untouched) or num_pairs values (index list).  The Radon intermediates are the metric's (ecc_dtr_from_device_linear +
 * ecc_metric_create, once per data set: the reference builds its textures once too).  Synchronous, like the reference's
 * launcher.  With use_corr the value is the finished cost 1 - cc (the reference hands five moments to its host epilogue,
 * ref: .cu:116-149, .cpp:199-210: that epilogue goes).  The rest of the caller's host epilogue stays (ref: .cpp:197-224). */
int ecc_metric_evaluate_external(ecc_metric* m, int num_Ps, const float* Cs_d, const float* PinvTs_d, int num_pairs,
                                 const int32_t* indices_d, float* K01s_d, float* out_d, float object_radius_mm, float dkappa,
                                 int use_corr);
/* Debug: the device-side result of the pre-compute (12 + 4 floats per view, host output). */
int ecc_metric_debug_geometry(ecc_metric* m, float* PinvTs, float* Cs);

/* ref: Metric::setObjectRadius / setEpipolarPlaneStep / MetricRadonIntermediate::useCorrelation
 * (EpipolarConsistency.cpp:70-90, …RadonIntermediate.cpp:80-85).  0 = automatic for both scalars.
 * use_corr != 0: pair value = 1 - un-centred correlation of the two redundant signals, with the
 * reference's provisional per-sample weight kappa_max/kappa (ref: ...RadonIntermediate.cu:116-149,274;
 * .cpp:127-131); the reference has no test for it (parity unpinned). */
int ecc_metric_set_params(ecc_metric* m, double object_radius_mm, double dkappa, int use_corr);
/* How the pair kernel obtains the sample positions of a pair (not in the reference, which has one GPU path with
 * hardware texture filtering and no CPU twin).  All modes implement the same formulas; they differ in
 * fp32 rounding, which matters for a SINGLE pair: its value is a sum of squared, nearly cancelling differences and
 * moves by ~2e-5 (median) when sample positions move by 1e-5 bins, while means over many pairs average that out.
 *   ECC_SAMPLING_POLYNOMIAL  sample coordinates from per-pair polynomials in kappa fitted by the pair-geometry kernel
 *                            (pairs whose fit is rejected take PER_SAMPLE by themselves).  Fastest;
 *                            all-pairs means agree with the CPU path to < 1e-6, single pairs to ~1e-4.
 *   ECC_SAMPLING_PER_SAMPLE  every pair evaluates line -> lineToSampleDtr per sample with device approximations
 *                            (v_rsq, v_rcp + minimax atan); ~1.5x the kernel time, same accuracy class as POLYNOMIAL.
 *   ECC_SAMPLING_REFERENCE   the CPU path's arithmetic operation for operation (ref: EpipolarConsistencyCommon.hxx:152-171,
 *                            ...RadonIntermediate.cu:71-113 in fp32 source order, sin/cos/atan2 correctly rounded,
 *                            exact fp32 bilinear rule with index clamps): single pair values agree with the CPU path
 *                            to float rounding of the final sum.  ~10x the kernel time of POLYNOMIAL per pair; ranges
 *                            of at most 2048 pairs put four waves on every pair, so a small evaluation takes as long
 *                            as in the other modes (~46 us for one pair).
 *   ECC_SAMPLING_AUTO        (default) REFERENCE when one evaluation covers at most
 *                            ECC_SAMPLING_AUTO_REFERENCE_PAIRS pairs (the whole evaluation is one pair's latency either
 *                            way: 2-view metric values, index lists as in tools/Registration/Registration3D3D.hxx:95,109),
 *                            POLYNOMIAL above.  Callers that compare values ACROSS calls of different size fix the mode.
 * WHOSE ROUNDING a cost-image entry carries (measured, scripts/pair_error_attribution.py, tests/test_configs.py; bench.py reports
 * it at full size as pair_rel_err_attribution).  The same formulas with the line -> (angle, distance) mapping in binary64, rounded
 * once, give the noise-free pair values.  The REFERENCE arithmetic (fp32 in source order = ECC_SAMPLING_REFERENCE = the CPU path)
 * is p50 1.4e-5 / p99 7.0e-5 / max 1.3e-4 away from them at 64 views of 512^2 -- and its MEAN 9.9e-6, the systematic part being
 * its float constant Pi (EpipolarConsistencyCommon.hxx:155,159).  POLYNOMIAL is 9.8e-6 / 5.0e-5 / 1.2e-4 away from the same
 * noise-free values, PER_SAMPLE 9.9e-6 / 3.9e-5 / 5.8e-5: both are CLOSER to them than the reference arithmetic is, while they
 * reproduce the reference's mean (float Pi included) to 6e-8 / 1.6e-7.  So the ~1e-5 (median) by which a single entry of the
 * n x n cost image differs from the CPU path's is the fp32 rounding of the reference's own arithmetic, not an error this
 * library adds; a caller that needs the CPU path's entry bit for bit selects ECC_SAMPLING_REFERENCE. */
/* ECC_SAMPLING_AUTO resolves from the size of the EVALUATION, not of the launch: n (n - 1) / 2 for ecc_metric_evaluate_all
 * and for every ecc_metric_evaluate_range[_async] shard of it (so G shard sums add up to the one-device sum's arithmetic
 * whatever G, and cost-balanced or re-balanced shards never mix modes), the list length for index lists. */
enum { ECC_SAMPLING_AUTO = 0, ECC_SAMPLING_POLYNOMIAL = 1, ECC_SAMPLING_PER_SAMPLE = 2, ECC_SAMPLING_REFERENCE = 3 };
#define ECC_SAMPLING_AUTO_REFERENCE_PAIRS 512
int ecc_metric_set_sampling(ecc_metric* m, int mode);
/* Opt-in pose-delta evaluation (default off; not in the reference).  The reference's optimisation problems change ONE
 * view's matrix per cost-function call and call setProjectionMatrices + evaluate() over all pairs
 * (ref: Gui/SingleImageMotion.h:84-90, Gui/Visualization.h:78-98).  When enabled, ecc_metric_evaluate_all (without a cost
 * image) and ecc_metric_evaluate_range keep the pair values of their last evaluation on the device; the next call with
 * the same range and parameters compares the new matrices with the ones those values belong to and re-evaluates only
 * the pairs that contain a changed view (when at most a quarter of the views changed, otherwise everything), then sums
 * the whole array again.  The result is BIT-IDENTICAL to a full evaluation: a pair's value is a function of its two
 * matrices, its two Radon intermediates and the parameters only, the sampling mode is the one the full range resolves
 * to, and the float64 sum has a fixed order (csrc/ecc_sum_order.h).  Changing parameters, sampling mode, the range, the number of views or
 * calling ecc_metric_refresh_dtrs drops the kept values.  ecc_metric_last_evaluated_pairs reports how many pairs the
 * last evaluate_all / evaluate_range recomputed. */
int ecc_metric_set_incremental(ecc_metric* m, int enable);
int ecc_metric_last_evaluated_pairs(const ecc_metric* m, int64_t* pairs);
/* Record reuse (default ON; not in the reference; ECC_RECORD_REUSE=0 in the environment turns the default off).  The
 * per-pair geometry of an evaluation (the reference's K01 array, ref: ...RadonIntermediate.cu:13-67, here k01_kernel's
 * records) is a function of the pair's two matrices and the parameters only.  ecc_metric_evaluate_all /
 * ecc_metric_evaluate_range[_async] keep the records of their last evaluation; when the next call evaluates the same range
 * with the same parameters and at most a quarter of the matrices differ bit-wise from the ones the records were made
 * from, only the pairs that contain a changed view are refitted, E1 (ref: ...RadonIntermediate.cpp:134-163) of the
 * changed views is computed on the host by the same code, and e1_kernel is not launched.  EVERY pair is still sampled by
 * the pair kernel: the work that is skipped is geometry that would be recomputed to identical bits, so results are
 * bit-identical with the switch on or off (tests/test_gpu_record_reuse.py).  This is the callers' pattern: the reference's
 * optimisation problems overwrite one view's matrix per cost-function call (ref: Gui/SingleImageMotion.h:84-90).
 * With the switch on, ecc_metric_set_projections only stages the matrices; E1 runs with the next call that needs it.
 * The refit of the changed pairs and their own pair-kernel launch run on a stream of the metric's own beside the
 * all-pairs launch (which skips them) on the context's stream; an event orders that stream after whatever this metric had
 * queued on the context's stream -- it reads nothing anybody else writes: records, device geometry, the row-paired copies
 * (ecc_metric_refresh_dtrs), pinned lists -- and is left out when the previous call was a synchronous evaluation, which
 * returns only after it has seen its result; the final sum is ordered after both streams (up to 512 views, no cost image;
 * otherwise one stream).  The synchronous calls (ecc_metric_evaluate_all, ecc_metric_evaluate_range) order it on the host: they
 * wait for the side stream's event -- its launches end long before the all-pairs launch does -- and then queue the sum behind the
 * all-pairs launch, so no cross-stream wait stands between the two kernels; the asynchronous, RCCL and group forms order it with
 * an event on the device.  The same launches with the same arguments either way. */
#define ECC_RECORD_REUSE_MIN_PAIRS 4096
#ifndef ECC_RECORD_REUSE_SPLIT_PAIRS
#define ECC_RECORD_REUSE_SPLIT_PAIRS 8192
#endif
/* on: 0 = off; 1 (default) = by size: ranges of more than ECC_RECORD_REUSE_MIN_PAIRS pairs (up to there refitting
 * everything is one short launch), the two-stream form from ECC_RECORD_REUSE_SPLIT_PAIRS pairs on (a shorter pair kernel
 * cannot hide the refit's launches: measured 2016 pairs, 61 us per step with two streams, 40 us refitting everything; a
 * 10 873-pair shard 63 us with, 77 us without); 2 = the two-stream form for every size (tests). */
int ecc_metric_set_record_reuse(ecc_metric* m, int on);
/* The host-side join of the two-stream form described above (default on; 0: every call orders the sum with an event on the
 * device, as the asynchronous forms do).  With it ecc_metric_evaluate_all / ecc_metric_evaluate_range poll the side stream's event
 * while the all-pairs launch runs -- the calling thread would poll for the result anyway -- and the sum kernel starts about 3 us
 * behind the all-pairs launch instead of about 6 (MI355X, 79 800 pairs).  The metrics of an ecc_group are created with it off.
 * Results are bit-identical either way. */
int ecc_metric_set_host_join(ecc_metric* m, int on);

/* One launch per small evaluation (default on).  An evaluation of at most 192 pairs -- ecc_metric_evaluate_all of up to 20
 * views, small ecc_metric_evaluate_range shards, short ecc_metric_evaluate_pairs index lists; not with use_corr, not the
 * asynchronous form -- runs as ONE kernel instead of the stream-ordered launches E1, K01, pairs, sum (the reference: two
 * kernels, two device-wide syncs and a host loop, ref: EpipolarConsistencyRadonIntermediate.cu:300-409,
 * ...RadonIntermediate.cpp:197-224; its working optimiser caller evaluates a handful of pairs per objective call, ref:
 * tools/FluoroTracking/FluoroTracking.cpp:179-211): E1 of the views whose matrix changed is computed on the host (the same
 * code, bit-identical) and travels in the kernel arguments, each workgroup fits its pair's record and samples it with four
 * waves, every value goes to the device array and -- at system scope -- to pinned host memory, the workgroup that arrives
 * last writes the word the host polls, and the host adds the values in the sum kernel's order (csrc/ecc_sum_order.h).  Larger evaluations keep the
 * stream-ordered launches, up to 4096 pairs with several waves per pair (pairs_split_kernel), index lists without copy
 * commands (the list is read from pinned memory, the sum kernel hands the values back), and launches of at most 4096 pairs
 * also take E1 of up to 16 changed views in the arguments of their record kernel (k01_patched_kernel) instead of an e1_kernel
 * launch.  Every value and every sum has the
 * bits of the multi-launch one-wave-per-pair path (tests/test_gpu_small_eval.py, tests/test_gpu_stress_sequences.py); on = 0
 * keeps the stream-ordered launches for everything. */
int ecc_metric_set_small_eval(ecc_metric* m, int on);
/* ref: Metric::getObjectRadius (EpipolarConsistency.cpp:76-84): user value, or the estimate
 * from the FIRST projection matrix. */
int ecc_metric_get_object_radius(const ecc_metric* m, double* radius_mm);

/* All-pairs evaluate, ref: double MetricRadonIntermediate::evaluate(float* out)
 * (…RadonIntermediate.cpp:166-225) = K01 + pair kernel + host mean.  cost_nxn (host, nullable) is
 * read-modify-written exactly like the reference's `out`.  *mean = sum_pairs / n_pairs. */
/* The float64 sum over the pair values has a fixed order for a given number of values (the same bits every run), but the
 * order is a function of that number: up to 32 767 values one workgroup adds them, from 32 768 on sixteen workgroups add
 * contiguous slices and the slice sums are added in slice order.  A sum over G shards is the rank-ordered sum of G such
 * sums.  So one-device and sharded sums of the same pair values agree to float64 rounding (~1e-16), not bit for bit. */
int ecc_metric_evaluate_all(ecc_metric* m, float* cost_nxn, double* mean);
/* n_poses INDEPENDENT all-pairs evaluations of one data set (a sweep of poses, the probes of a finite-difference gradient;
 * ref: Gui/Visualization.h:59-112 plotCostFunction -- 100 steps x 6 parameters, BASELINE config 5 -- through
 * Gui/SingleImageMotion.h:84-90).  The reference evaluates them one setProjectionMatrices + evaluate at a time.
 *
 * ecc_metric_evaluate_pose_deltas: pose k = the metric's CURRENT matrices (the base: the last ecc_metric_set_projections)
 * with the views moved_views[moved_offsets[k] .. moved_offsets[k + 1]) (strictly ascending within a pose) replaced by the
 * matrices moved_Ps[12 * q ..] of the same entries q.  All poses of the call are ONE launch that lists the pairs and does E1
 * of the moved matrices, ONE record launch and ONE pair launch over the (pose, moved view) x partner grid -- n_views - 1 pairs
 * per moved view instead of n (n - 1) / 2 per pose -- and ONE segmented float64 sum that walks, per pose, the base's pair values with the pose's own
 * substituted in exactly the order the all-pairs sum adds them (csrc/ecc_sum_order.h): every mean has the bits of ecc_metric_set_projections +
 * ecc_metric_evaluate_all on that pose's matrices (tests/test_gpu_pose_batch.py).  The base's pair values are kept between
 * calls (only the pairs of views that changed since are redone).  The metric's current matrices are unchanged by the call.
 * A pose with more than 32 moved views, or one that moves view 0 under the automatic object radius and changes it, is
 * evaluated the sequential way inside the call (same bits).  400 views of 1024^2, 600 poses of one moved view on one MI355X:
 * see DESIGN.md 4.9 (two orders of magnitude above the sequential steps: the work is 239 400 pairs, not 47 880 000).
 *
 * ecc_metric_evaluate_poses[_strided]: the same for FULL matrices per pose (Ps_batch: n_poses x n_views x 12 float64); the
 * strided form evaluates the poses first, first + stride, ... only and leaves the other entries of `means` alone (rank r of
 * N: first = r, stride = N -- poses shard with no exchange at all).  The library finds the moved views itself by comparing
 * every pose with the metric's current matrices (or with the first pose when most poses are far from those) and takes the
 * batch above; poses that are no small delta are evaluated two deep on the context's stream (pose k + 1 is handed over
 * while the device runs pose k).  Same bits either way.  The matrices of the LAST evaluated pose stay the metric's current
 * ones.  ecc_metric_set_pose_batching(m, 0): everything two deep (the launches of n_poses x (ecc_metric_set_projections +
 * ecc_metric_evaluate_all) in the same order) -- what rounds 4-5 measured.  ecc_metric_last_batched_poses: how many poses of
 * the last of these calls went through the batch. */
int ecc_metric_evaluate_pose_deltas(ecc_metric* m, int n_poses, const int32_t* moved_offsets, const int32_t* moved_views,
                                    const double* moved_Ps, double* means);
int ecc_metric_evaluate_poses(ecc_metric* m, int n_poses, const double* Ps_batch, int n_views, double* means);
int ecc_metric_evaluate_poses_strided(ecc_metric* m, int n_poses, const double* Ps_batch, int n_views, int first, int stride,
                                      double* means);
int ecc_metric_set_pose_batching(ecc_metric* m, int on);
int ecc_metric_last_batched_poses(const ecc_metric* m, int64_t* poses);

/* The finite-difference gradient of the metric over n_params pose parameters of ONE view: the metric at the current matrices
 * and its 2 n_params central-difference probes in one call (what every optimiser step of a moved view asks for; ref:
 * Gui/SingleImageMotion.h:84-90, six parameters of the "3D Rigid" model).  The caller supplies the probe MATRICES -- Ps_plus and
 * Ps_minus: n_params x 12 float64, the view's 3x4 matrix (column-major) at x + h[p] e_p and at x - h[p] e_p -- so the library
 * stays free of any motion model.  h: the n_params step lengths.  value (nullable), grad (n_params), probes (nullable,
 * 2 n_params: plus_0, minus_0, plus_1, ...).
 *
 * The contract (tests/test_gpu_gradient.py):
 *   - probes[k] has THE BITS of ecc_metric_evaluate_pose_deltas for the pose "current matrices with `view` replaced by probe k",
 *     hence of ecc_metric_set_projections + ecc_metric_evaluate_all on those matrices; *value has the bits of
 *     ecc_metric_evaluate_all on the current matrices.
 *   - grad[p] = (probes[2p] - probes[2p + 1]) / (2.0 * h[p]) in binary64: one subtraction, one multiplication, one division,
 *     in that order, on the host.
 *   - The call leaves the metric as ecc_metric_evaluate_pose_deltas does: current matrices unchanged, the base's pair values
 *     kept for the next call (only the pairs of views changed since are redone).
 *   - Errors before anything is launched (ECC_ERR_INVALID_ARGUMENT): m == NULL (checked first), another null pointer among
 *     Ps_plus, Ps_minus, h, grad; n_params < 1; no matrices set, fewer than two views; view outside [0, n_views); an h[p] that
 *     is zero or not finite.
 *
 * ecc_metric_last_gradient_path: which way the last call went.
 *   1  (the default) ecc_metric_evaluate_pose_deltas with the 2 n_params probes and one pose that moves nothing (for *value);
 *      that call evaluates a probe that changes the automatic object radius the sequential way itself.
 *   0  the same call after ecc_metric_set_pose_batching(m, 0): every probe sequentially.
 *   2  ONE launch for records and sampling of all probes (csrc/small_poses_kernel.hip: E1 of the probe matrices on the host,
 *      handed over in the kernel arguments) + the segmented sum of the pose batch: two launches, three from 257 views, instead
 *      of five.  OPT-IN, ecc_debug_set_gradient_launch(m, 1): measured on one MI355X it is not faster than path 1 by more than
 *      the run-to-run spread at 400 views and slower at 258 (DESIGN.md 4.11 has the numbers), so the default stays path 1.
 * Same bits whichever way.  With the launch switched on, whatever it does not take goes through path 1 (or 0) INSIDE the same
 * call.  It declines, and only then:
 *   - n_params > 8 (the launch holds 16 probe entries);
 *   - view == 0 under the automatic object radius (object_radius_mm <= 0) when a probe changes the radius;
 *   - use_corr (MetricRadonIntermediate::useCorrelation);
 *   - ECC_SAMPLING_REFERENCE chosen with ecc_metric_set_sampling on more than 2048 pairs (65 views or more; the automatic mode
 *     never resolves to the reference arithmetic there);
 *   - ecc_metric_set_pose_batching(m, 0) (path 0).
 * Every other state is taken: the automatic sampling mode at every size, ECC_SAMPLING_POLYNOMIAL / _PER_SAMPLE, a user dkappa, a
 * fixed or automatic radius, record reuse on or off, the pose-delta mode on or off. */
int ecc_metric_evaluate_gradient(ecc_metric* m, int view, int n_params, const double* Ps_plus, const double* Ps_minus,
                                 const double* h, double* value, double* grad, double* probes);
int ecc_metric_last_gradient_path(const ecc_metric* m, int* path);

/* The metric as a QUADRATIC FORM of channel coefficients, for the optimisers that move the IMAGES and leave the matrices alone
 * (beam-hardening linearisation, empirical scatter or offset correction):
 *     corrected image of view i = sum_c a_c I_c,i      (I_c,i: K fixed "channel" images per view, a: K coefficients).
 * Line integrals, the derivative across t, the ramp filter and bilinear sampling are linear, so the Radon intermediate of the
 * corrected image is sum_c a_c D_c,i (D_c,i: the intermediate of I_c,i), every redundant sample is linear in a, and
 *     metric(a) = a^T G a,   G[c][d] = mean over the pairs of g_ij[c][d],
 *     g_ij[c][d] = sum_kappa (delta_c+ delta_d+ + delta_c- delta_d-) K0[6] dkappa,  delta_c = signed sample of D_c,i - of D_c,j,
 * with the sample positions, fold signs, kappa range and weights of ecc_metric_evaluate_all (they depend on the matrices only).
 * One call replaces the device work of the whole optimisation: G gives the metric of every a in closed form.
 *
 * The metric must hold n_dtrs = n_channels * n_views Radon intermediates, CHANNEL-MAJOR: channel c of view i is dtr
 * c * n_views + i.  The POST-PROCESS of every intermediate must be the identity (ECC_POST_IDENTITY): square root and logarithm
 * are not linear, and the metric cannot check it (ecc_dtr_info does not report it).  All channels need the same bin counts
 * (ecc_metric_create checks that) and the same image size.  The other calls keep their meaning on such a metric:
 * ecc_metric_evaluate_all and the pose calls evaluate dtrs 0 .. n_views - 1, i.e. channel 0; ecc_metric_evaluate_transforms
 * wants n_dtrs == n_views and goes on refusing it.  Memory: the metric's private copies grow with K * n like any metric's
 * (row-paired always, row-quad when they are built); the call adds none, only 296 + 2 K (K + 1) bytes per pair of scratch.
 *
 * gram (required): n_channels x n_channels float64, the full symmetric matrix.  pair_grams (host, nullable): n_pairs x T
 * float32, T = K (K + 1) / 2, pair-major in the pair order of get_ij, entries in the order (0,0), (0,1) .. (0,K-1), (1,1) ..
 * (K-1,K-1).  All pairs over the current matrices.  The sampling mode resolves from n (n - 1) / 2 as in ecc_metric_evaluate_all;
 * ECC_SAMPLING_POLYNOMIAL (with its per-pair fallback and exact tail), _PER_SAMPLE and _REFERENCE are all taken, and so are a
 * fixed or automatic object radius, a user dkappa and non-derivative intermediates (the flag comes from dtrs[0], as everywhere).
 *
 * The contract (tests/test_gpu_gram.py):
 *   1. Diagonal, bit for bit.  pair_grams[q][(c,c)] has the bits of the cost-image entry ecc_metric_evaluate_all writes for pair
 *      q on a metric created from channel c's n_views intermediates alone with the same matrices, parameters and sampling mode;
 *      gram[c][c] has the bits of that call's mean.  Per sample the term of entry (c, d) is that evaluation's expression with the
 *      second factor exchanged, accumulated in float64 per lane in the same trip order, reduced by the same wave tree, rounded to
 *      float32 per pair entry; each of the T columns is summed over the pairs in the order of csrc/ecc_sum_order.h and divided
 *      by n_pairs.  n_channels = 1 is ecc_metric_evaluate_all with a cost image.
 *   2. Symmetric by construction: only c <= d is computed, gram[d][c] is a copy.
 *   3. Off-diagonal entries agree with the polarisation of the CPU oracle's pair values to its own floor (the tests measure it).
 *   - The call changes nothing a later call can see: current matrices, kept records, the kept values of the pose-delta mode and
 *     of the pose batch.
 *   - Errors before anything is launched, ECC_ERR_INVALID_ARGUMENT: m == NULL (checked first), gram == NULL, n_channels outside
 *     [1, ECC_GRAM_MAX_CHANNELS], no matrices set or fewer than two views, n_dtrs != n_channels * n_views.  use_corr set:
 *     ECC_ERR_UNSUPPORTED (the correlation cost is not a quadratic form).
 * Launches (csrc/ecc_gram.hip, csrc/gram_kernel.hip): the record kernel over all pairs, pairs_gram_kernel -- one wave per pair,
 * the position arithmetic of a kappa step once for all channels, 4 K gathers and T products per step --, one launch for the T
 * column sums.  A once-per-data-set call: it has no small-evaluation or sharded form. */
#define ECC_GRAM_MAX_CHANNELS 4
int ecc_metric_evaluate_gram(ecc_metric* m, int n_channels, float* pair_grams, double* gram);

/* The metric at PER-VIEW channel coefficients, and its gradient with respect to all of them, in one call -- for the image-domain
 * corrections whose coefficients differ from view to view (a gain, an offset or a scatter scale per view):
 *     corrected intermediate of view i = sum_c a_c,i D_c,i      (n_channels * n_views coefficients instead of n_channels).
 * The metric is a quadratic form f(a) = a^T G a of the n K coefficients, so its gradient 2 G a is linear in a and THE SAME CALL at
 * a direction v returns the Hessian-vector product: H v = grad f(v).  Gradient descent, L-BFGS or conjugate gradients over
 * n K coefficients need nothing else, and the (n K) x (n K) matrix is never formed; a call costs about one
 * ecc_metric_evaluate_gram call of the same n_channels.
 *
 * The metric holds n_channels * n_views Radon intermediates, channel-major, with the identity post-process, exactly as for
 * ecc_metric_evaluate_gram: channel c of view i is dtr c * n_views + i.
 *   coeffs (host, required): n_channels * n_views float32, coeffs[c * n_views + i] = a_c,i.
 *   value (required): the metric of the corrected intermediates, the mean over all pairs.
 *   grad (host, nullable): n_channels * n_views float64, grad[c * n_views + i] = d value / d a_c,i.
 *   pair_terms (host, nullable): n_pairs x (1 + 2 K) float32, pair-major in the pair order of get_ij (the order of
 *     ecc_metric_evaluate_all's cost image), per pair i < j the entries {value, h0[0 .. K), h1[0 .. K)} with
 *     h0[c] = 1/2 d (pair value) / d a_c,i and h1[c] = 1/2 d (pair value) / d a_c,j.
 * All pairs over the current matrices; the sampling mode resolves from n (n - 1) / 2 as in ecc_metric_evaluate_all, and
 * ECC_SAMPLING_POLYNOMIAL (with its per-pair fallback and exact tail), _PER_SAMPLE and _REFERENCE are all taken, as are a fixed
 * or automatic object radius, a user dkappa and non-derivative intermediates.
 *
 * The contract (tests/test_gpu_view_coefficients.py):
 *   1. Per sample and side the combined sample is s = a_0 v_0, then s = fmaf(a_c, v_c, s) in channel order; the two differences
 *      and the value term are ecc_metric_evaluate_all's expressions, accumulated in float64 per lane in the same trip order,
 *      reduced by the same wave tree, rounded to float32 per pair, summed in the order of csrc/ecc_sum_order.h and divided by
 *      n_pairs.  So with ONE coefficient 1.0 per view and the others 0.0, value and the pair values have the bits of
 *      ecc_metric_evaluate_all on a metric of the selected intermediates alone (n_channels = 1, all ones: of this metric).
 *   2. The gradient terms are the value term with its second factor exchanged for the channel's sample (signed so that h1 is the
 *      derivative by view j's coefficient); grad[c * n + v] = 2 / n_pairs * the float64 sum of the n - 1 terms of the pairs that
 *      contain v, added in ONE fixed order (csrc/sum_kernel.hip, sum_view_terms_kernel): no atomics, the same bits on every run.
 *   3. value, grad and the pair terms agree with the CPU oracle on intermediates combined on the host to the project's bars, and
 *      sum_k a_k grad_k = 2 value (Euler) to 1e-5 of the terms' magnitudes.
 *   - The call changes nothing a later call can see: current matrices, kept records, the kept values of the pose-delta mode and
 *     of the pose batch.  (It shares ecc_metric_evaluate_gram's scratch.)
 *   - Errors before anything is launched or written, ECC_ERR_INVALID_ARGUMENT: m == NULL (checked first), value == NULL,
 *     coeffs == NULL, n_channels outside [1, ECC_VIEW_COEFF_MAX_CHANNELS], no matrices set or fewer than two views,
 *     n_dtrs != n_channels * n_views.  use_corr set: ECC_ERR_UNSUPPORTED.
 * Launches (csrc/ecc_view_coeff.hip, csrc/view_coeff_kernel.hip): the record kernel over all pairs, pairs_coeff_kernel -- one
 * wave per pair, a pair's 2 K coefficients in scalar registers, the position arithmetic of a kappa step once, 4 K gathers and
 * 1 + 2 K products per step --, one launch for the value's sum, one for the n K gradient sums.  No small-evaluation, range, group
 * or sharded form. */
#define ECC_VIEW_COEFF_MAX_CHANNELS 4
int ecc_metric_evaluate_view_coefficients(ecc_metric* m, int n_channels, const float* coeffs,
                                          double* value, double* grad, float* pair_terms);

/* The quadratic form of PER-VIEW channel coefficients AS A MATRIX: f(a) = a^T H a, grad f = 2 H a, with the index
 * k = c * n_views + i of ecc_metric_evaluate_view_coefficients' coeffs.  For the callers who need the form itself and not its
 * products -- a direct constrained solve, a regularisation sweep, many gauge or constraint choices on one data set, an
 * eigen-analysis of what the data do not determine: one call, then every coefficient vector in closed form on the host, which is
 * what ecc_metric_evaluate_gram gives the shared case.  (Through ecc_metric_evaluate_view_coefficients the matrix costs n K calls
 * at one-hot coefficients.)
 *
 * The metric holds n_channels * n_views Radon intermediates, channel-major, with the identity post-process, exactly as for
 * ecc_metric_evaluate_gram and ecc_metric_evaluate_view_coefficients.  For the pair q = (i < j) with the signed samples v0_c(s),
 * v1_c(s) of channel c in view i and in view j over the pair's +-kappa samples s -- positions, fold signs, kappa range and sampling
 * mode of ecc_metric_evaluate_all -- and the weight w = K0[6] * dkappa formed in binary64 from the two float32 values:
 *     P00[c][d] = w sum_s v0_c v0_d,   P11[c][d] = w sum_s v1_c v1_d,   P01[c][d] = -w sum_s v0_c v1_d   (P01 is not symmetric),
 *     pair value(a_i, a_j) = a_i^T P00 a_i + a_j^T P11 a_j + 2 a_i^T P01 a_j,
 *     H[(c,i),(d,i)] = (sum_{j>i} P00_ij[c][d] + sum_{w<i} P11_wi[c][d]) / N,   H[(c,i),(d,j)] = H[(d,j),(c,i)] = P01_ij[c][d] / N
 * for i < j, N = n_views (n_views - 1) / 2.
 *   hessian (host, nullable): (n_views * n_channels)^2 float64, the full symmetric matrix; n_views * n_channels must not exceed
 *     ECC_VIEW_HESSIAN_MAX_DIM then (512 MB on the device and on the host).
 *   pair_blocks (host, nullable): n_pairs x T2 float64, T2 = K (K + 1) + K^2, pair-major in the pair order of get_ij; per pair
 *     P00's upper triangle in ecc_metric_evaluate_gram's entry order, then P11's upper triangle, then P01 row-major.
 *   At least one of the two must be given.
 *
 * The contract (tests/test_gpu_view_hessian.py):
 *   1. Accuracy by construction.  The form is used near its minimum, where f(a) is a small difference of large moments, so nothing
 *      is rounded in float32 behind the samples: the kernels see the float32 sample values ecc_metric_evaluate_view_coefficients
 *      sees, convert each to binary64 once, and every product of two samples is exact in binary64; an entry is
 *      acc = fma(x, y, acc) for the + and then the - sample of a kappa step, per lane in the trip order of the other pair kernels,
 *      reduced by the same wave tree, multiplied by w once and stored as float64.
 *   2. Every off-diagonal entry of H and its transposed twin are written once as P01 / N; every diagonal-block entry is the float64
 *      sum over the view's n_views - 1 pairs in ONE fixed order (partners ascending, as csrc/sum_kernel.hip's sum_view_terms_kernel
 *      adds the gradient terms) divided by N.  No atomics: the same bits on every run, and H == H^T bit for bit.
 *   3. The pair blocks agree with a float64 oracle and with the one-hot calls of ecc_metric_evaluate_view_coefficients to the
 *      project's bars relative to the entries' Cauchy-Schwarz scales.
 *   - The call changes nothing a later call can see: current matrices, kept records, the kept values of the pose-delta mode and
 *     of the pose batch.  It shares ecc_metric_evaluate_gram's record scratch and has value scratch of its own, 8 T2 bytes per pair
 *     (23 MB at 400 views and four channels), plus the matrix when it is asked for.  The value scratch stays with the metric until
 *     it is destroyed, as ecc_metric_evaluate_gram's does; the matrix stays only while it is at most 64 MB and is freed before the
 *     call returns otherwise.
 *   - Errors before anything is launched or written, ECC_ERR_INVALID_ARGUMENT: m == NULL (checked first), hessian and pair_blocks
 *     both NULL, n_channels outside [1, ECC_VIEW_HESSIAN_MAX_CHANNELS], no matrices set or fewer than two views,
 *     n_dtrs != n_channels * n_views.  ECC_ERR_UNSUPPORTED: use_corr set; hessian given with n_views * n_channels above
 *     ECC_VIEW_HESSIAN_MAX_DIM.
 * Launches (csrc/ecc_view_hessian.hip, csrc/view_hessian_kernel.hip): the record kernel over all pairs, pairs_moments_kernel -- one
 * wave per pair, the position arithmetic of a kappa step once, 4 K gathers and 2 T2 binary64 fused multiply-adds per step --, and
 * assemble_view_hessian_kernel when the matrix is asked for.  No small-evaluation, range, group or sharded form. */
#define ECC_VIEW_HESSIAN_MAX_CHANNELS 4
#define ECC_VIEW_HESSIAN_MAX_DIM 8192   /* n_views * n_channels when hessian != NULL: 512 MB */
int ecc_metric_evaluate_view_hessian(ecc_metric* m, int n_channels, double* hessian, double* pair_blocks);

/* The metric with PER-LINE WEIGHTS in Radon space: which redundant samples count.  An instrument in one view of a fluoroscopy
 * sequence, a collimator blade, a defective detector column or a table edge present in some views only breaks exactly the epipolar
 * lines that cross it and leaves every other line consistent; zeroing or feathering the region in the image changes the integral of
 * every line through it and only moves the inconsistency.  The reference has a weight slot per sample for this, wired to 1.0f
 * (ref: EpipolarConsistencyRadonIntermediate.cu:254), and its host epilogue already returns sum value w / sum w
 * (ref: ...RadonIntermediate.cpp:197-224).
 *
 * The metric holds 2 * n_views Radon intermediates, channel-major as for ecc_metric_evaluate_gram: dtr i is the data of view i, dtr
 * n_views + i the LINE WEIGHTS W_i of view i on the same bin grid, normally made without a filter and with values in [0, 1]; any
 * finite float is taken as it is.  For the pair i < j a +-kappa sample has the positions, kappa range and sampling mode of
 * ecc_metric_evaluate_all; d is that evaluation's difference of the two signed data samples, and mu = W_i(sample) * W_j(sample) one
 * float32 multiply of two bilinear samples taken at the same taps as the data.  The fold sign is never applied to a weight sample.
 * Per kappa step the value term is ecc_metric_evaluate_all's expression with mu multiplied into the first factor only --
 *     polynomial loops             fmaf(mu_p * dp, dp, (mu_m * dm) * dm) * w06_dkappa
 *     exact and reference loops    (((mu_p * dp) * dp + (mu_m * dm) * dm) * K0[6]) * dkappa
 * -- accumulated in float64 per lane in the same trip order and reduced by the same wave tree; beside it each lane adds
 * (double)(mu_p + mu_m), the weight mass, and 2.0, the sample count.  Per pair q:
 *     c_q = the float32 value,
 *     u_q = (float)(mass / count), the COVERAGE in [0, 1]; a pair without samples has c_q = 0, u_q = 1.0f.
 *   value (required): sum c_q / sum u_q, both sums in the order of csrc/ecc_sum_order.h.  Dividing by sum u_q keeps an optimiser from
 *     lowering the metric by pushing lines into masked regions; the unnormalised sums are in the pair terms.
 *   coverage (nullable): sum u_q / n_pairs.  sum u_q == 0: value = 0.0, coverage = 0.0 and ECC_OK.
 *   pair_terms (host, nullable): n_pairs x 2 float32, pair-major in the pair order of get_ij, each row {c_q, u_q}.
 * All pairs over the current matrices; the sampling mode resolves from n (n - 1) / 2 as in ecc_metric_evaluate_all, and
 * ECC_SAMPLING_POLYNOMIAL (with its per-pair fallback and exact tail), _PER_SAMPLE and _REFERENCE are all taken, as are a fixed or
 * automatic object radius, a user dkappa, non-derivative data and row-paired and row-quad copies.
 *
 * The contract (tests/test_gpu_weighted.py):
 *   1. With every weight 1.0f, value and the c column have the bits of ecc_metric_evaluate_all on the same metric, every u_q and
 *      coverage are 1.0.
 *   2. With W_v = 0 for one view and 1 elsewhere the pairs that contain v are {0, 0}, every other pair keeps its bits, and value is
 *      the mean over the other pairs.
 *   3. c_q and u_q agree with a float64 oracle (tests/weighted_terms.py) to the project's bars.
 *   4. Data that differ only on lines whose weight is 0 give the same bits.
 *   - The call changes nothing a later call can see: current matrices, kept records, the kept values of the pose-delta mode and of
 *     the pose batch.  (It shares ecc_metric_evaluate_gram's scratch.)
 *   - Errors before anything is launched or written, ECC_ERR_INVALID_ARGUMENT: m == NULL (checked first), value == NULL, no matrices
 *     set or fewer than two views, n_dtrs != 2 * n_views.  use_corr set: ECC_ERR_UNSUPPORTED.
 * Launches (csrc/ecc_weighted.hip, csrc/weighted_kernel.hip): the record kernel over all pairs, pairs_weighted_kernel -- one wave per
 * pair, the position arithmetic of a kappa step once, 8 gathers --, one launch for the two sums.
 * Index lists and pose deltas: ecc_metric_evaluate_weighted_pairs, ecc_metric_evaluate_weighted_pose_deltas below.
 * The registration of two scans: ecc_metric_evaluate_weighted_transforms below.
 * Out of scope: full-matrices pose batches, range, group and RCCL forms; weights under use_corr.  The
 * 1 / (sigma0^2 + sigma1^2) variance form is ecc_metric_evaluate_variance below.  A per-sample robust loss, for callers who do not know where the bad lines are:
 * ecc_metric_evaluate_robust and its pose-delta and transform forms below (on a metric of n_views intermediates); the loss combined
 * with these weights: ecc_metric_evaluate_weighted_robust below. */
int ecc_metric_evaluate_weighted(ecc_metric* m, double* value, double* coverage, float* pair_terms);

/* The weighted metric for pose optimisers (csrc/ecc_weighted_poses.hip): a tracker that scores one frame against
 * reference views has an index list, an optimiser step with a finite-difference gradient has a batch of poses that each move a few
 * views.  Both need a metric as ecc_metric_evaluate_weighted does: n_dtrs == 2 * n_views (data, then line weights), no use_corr.
 *
 * ecc_metric_evaluate_weighted_pairs: idx4 holds n_pairs tuples (P0, P1, D0, D1) as for ecc_metric_evaluate_pairs.  P* index the
 * current matrices.  D* index the DATA intermediates and must lie in [0, n_views); the weights of a sample come from dtr
 * n_views + D* -- the weight follows the data index, never the matrix index.  A tuple with P0 == P1 has no samples: {c, u} =
 * {0, 1}.  The sampling mode resolves from n_pairs of the LIST, as ecc_metric_evaluate_pairs resolves it (ECC_SAMPLING_AUTO: up to
 * 512 tuples use the reference arithmetic).  Per tuple c and u are those of ecc_metric_evaluate_weighted's pair; pair_terms
 * (nullable): n_pairs x 2 floats in list order.  *value = sum c / sum u, *coverage (nullable) = sum u / n_pairs, both sums in the
 * order of csrc/ecc_sum_order.h for n_pairs values; sum u == 0: 0, 0 and ECC_OK.  n_pairs == 0: ECC_OK, nothing written.
 * With tuples (i, j, i, j) the rows have the bits of ecc_metric_evaluate_weighted's rows of those pairs under the same resolved
 * mode; with every weight 1.0f the c column and value have the bits of ecc_metric_evaluate_pairs of the same list.
 * Launches: the record kernel with the list, the weighted pair kernel, one launch for the two sums, the copies.
 *
 * ecc_metric_evaluate_weighted_pose_deltas: the lists of ecc_metric_evaluate_pose_deltas -- pose k = the CURRENT matrices with the
 * views moved_views[moved_offsets[k] .. moved_offsets[k + 1]) (strictly ascending) replaced by moved_Ps[12 q ..]; n_poses < 1:
 * ECC_OK.  values[k] and coverages[k] (coverages nullable) have THE BITS of ecc_metric_set_projections(pose k) +
 * ecc_metric_evaluate_weighted (tests/test_gpu_weighted_poses.py).  Per call: {c, u} of all pairs at the current matrices (the
 * launches of ecc_metric_evaluate_weighted; recomputed on every call), then per batch ONE launch that lists the pairs and does E1
 * of the moved matrices, ONE record launch and ONE weighted pair launch over the (pose, moved view) x partner grid, and ONE
 * segmented sum that adds, per pose and column, the base's values with the pose's own substituted in the order of
 * csrc/ecc_sum_order.h.  A pose with more than 32 moved views, one that moves view 0 under the automatic object radius and changes
 * it, and every pose after ecc_metric_set_pose_batching(m, 0) is evaluated the sequential way inside the call (same bits);
 * ecc_metric_last_batched_poses reports how many went through the batch.  Calls of more than 2^20 grid entries run as several
 * batches over the same base columns.
 *
 * Both: errors are returned before anything is launched or written.  ECC_ERR_INVALID_ARGUMENT: m == NULL (checked first); a null
 * value / values / moved_offsets / idx4 (with n_pairs > 0); null list arrays when moved_offsets[n_poses] > 0; no matrices set or
 * fewer than two views; n_dtrs != 2 * n_views; a bad list or tuple.  ECC_ERR_UNSUPPORTED under use_corr.  The calls change nothing a
 * later call can see: current matrices, kept records, the kept values of the pose-delta mode and of the pose batch.  (They rewrite
 * the pose batch's per-batch scratch and ecc_metric_evaluate_gram's scratch, as every call of those families does.)
 * Not built: base columns kept between calls; the full-matrices, strided, group and RCCL forms; the
 * incremental (ecc_metric_set_incremental) mode for the weighted value; a one-launch small path for weighted lists. */
int ecc_metric_evaluate_weighted_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, double* value, double* coverage, float* pair_terms);
int ecc_metric_evaluate_weighted_pose_deltas(ecc_metric* m, int n_poses, const int32_t* moved_offsets, const int32_t* moved_views,
                                             const double* moved_Ps, double* values, double* coverages);

/* n_transforms rigid source-to-target transforms of two scans in one call: the registration of two scans (ref:
 * tools/Registration/Registration3D3D.hxx:56-62, :91-110 -- a cost call multiplies every source matrix by one 4x4 transform,
 * calls setProjectionMatrices and evaluates the index list of all source x target pairs).
 *
 * The metric's CURRENT matrices are the base.  Views [0, n_source) are the source scan, views [n_source, n_views) the target
 * scan (n_target = n_views - n_source), as the reference orders them.  For transform k (Ts + 16 k, a 4x4 float64 matrix stored
 * column-major like every matrix of this ABI) the source matrices become ecc_host_compose_transform(P_i, T_k), the target
 * matrices stay, and the index list is: entry q = j * n_source + i -> (i, n_source + j, i, n_source + j), source index fast.
 * means[k] = the total of that list's values in the order of csrc/ecc_sum_order.h divided by n_source * n_target -- the mean
 * over the CROSS pairs only: source x source pairs do not change under a common rigid transform and target x target pairs do
 * not change at all.  pair_values (host, nullable) receives n_transforms x n_target x n_source floats in list order.
 *
 * The contract: every means[k] and every pair value has the bits of ecc_metric_set_projections(the composed matrices) +
 * ecc_metric_evaluate_pairs(that list) on a metric with the same parameters (tests/test_gpu_transforms.py).  So the sampling
 * mode resolves from the list length n_source * n_target, and under the automatic object radius (the default) the radius of
 * transform k is the one derived from the COMPOSED view 0: it differs from transform to transform, and with it the range of
 * epipolar planes, so the values of a sweep are not strictly comparable with each other.  A registration caller should FIX
 * the radius (ecc_metric_set_params); the automatic one is supported, inside the batch, because it is the default and the
 * contract is the sequential calls' bits.  use_corr, a user dkappa and a fixed radius work as in the sequential calls.
 *
 * All transforms of the call are ONE launch that composes P_i T_k, does E1 of the composed matrices and lists the pairs, ONE
 * record launch and ONE pair launch over the pair x transform grid, and ONE segmented float64 sum (csrc/ecc_transforms.hip);
 * calls of more than 2^20 grid entries are cut into batches of whole transforms.  The call leaves the metric as it found it:
 * current matrices, kept records, the kept values of the pose-delta mode and of the pose batch.  A single transform whose list
 * alone exceeds a batch, and every transform after ecc_metric_set_pose_batching(m, 0), is evaluated the sequential way inside
 * the call (same bits).  n_transforms = 0 does nothing.  ecc_metric_last_batched_transforms: how many transforms of the last
 * call went through the batch.  Needs one Radon intermediate per view and 1 <= n_source < n_views.
 * An "evaluation" here is n_source * n_target sampled pairs; it is not the all-pairs evaluation the pose batch counts. */
int ecc_metric_evaluate_transforms(ecc_metric* m, int n_source, int n_transforms, const double* Ts, double* means,
                                   float* pair_values);
int ecc_metric_last_batched_transforms(const ecc_metric* m, int64_t* transforms);
/* P (3x4) times T (4x4), both float64 and stored column-major: out(r, c) = ((P(r,0) T(0,c) + P(r,1) T(1,c)) + P(r,2) T(2,c))
 * + P(r,3) T(3,c), every product and every sum rounded to binary64 on its own (no fused multiply-add) -- host, device and
 * tests agree on the bits.  out12 may be P12. */
void ecc_host_compose_transform(const double* P12, const double* T16, double* out12);

/* ecc_metric_evaluate_transforms for the metric with per-line weights (csrc/ecc_weighted_transforms.hip): the
 * registration of two scans of which one is truncated or collimated, sees a table edge the other does not, or holds an instrument
 * the other does not -- each breaks exactly the lines that cross it, in every cross pair of that view.  The metric is
 * ecc_metric_evaluate_weighted's: n_dtrs == 2 * n_views (the data of every view, then its line weights), no use_corr.
 *
 * Views, transforms and the cross list are those of ecc_metric_evaluate_transforms: views [0, n_source) are the source scan, the
 * rest the target scan; Ts + 16 k is a column-major 4x4 float64 transform; the source matrices become
 * ecc_host_compose_transform(P_i, T_k); list entry q = j * n_source + i is the tuple (i, n_source + j, i, n_source + j);
 * count = n_source * n_target.  The weights follow the DATA index (dtr n_views + D), never the extended matrix index.
 *   values[k] (required): sum c / sum u over the list of transform k.
 *   coverages[k] (nullable): sum u / count.  sum u == 0: value 0.0, coverage 0.0 and ECC_OK.
 *   pair_terms (host, nullable): n_transforms x n_target x n_source x 2 float32, per transform its count rows {c, u} in list order.
 * The contract (tests/test_gpu_weighted_transforms.py): all three have THE BITS of ecc_metric_set_projections(the composed
 * matrices) + ecc_metric_evaluate_weighted_pairs(that list) on a metric with the same parameters.  So the sampling mode (and the
 * reference arithmetic's wave split) resolves from a list of count tuples, under the automatic object radius every transform takes
 * the radius of its composed view 0 (fix the radius for a sweep whose values are compared with each other), and each column's sum is
 * added in the order of csrc/ecc_sum_order.h for count values, the slice sums -- the single one too -- added to 0.0 in slice order.
 *
 * Per batch: ecc_metric_evaluate_transforms' ONE launch that composes P_i T_k, does E1 of the n + K n_source extended matrices and
 * writes the pair-major, transform-minor index grid, ONE record launch, ONE weighted pair launch over the grid and ONE segmented
 * sum of both columns, which reads a transform's values K floats apart where the pair launch left them.  Calls of more than 2^20
 * grid entries are cut into batches of whole transforms.  A transform whose list alone exceeds a batch, and every transform after
 * ecc_metric_set_pose_batching(m, 0), is evaluated the sequential way inside the call (same bits, the base matrices set again);
 * ecc_metric_last_batched_transforms counts what went through the batch.  The call leaves the metric as it found it: current
 * matrices, kept records, the kept values of the pose-delta mode and of the pose batch.  (It rewrites the pose batch's per-batch
 * scratch, and the sequential way ecc_metric_evaluate_gram's scratch.)
 *
 * Errors are returned before anything is launched or written, checked in this order: m == NULL; n_transforms < 0; null Ts or values
 * with n_transforms > 0; no matrices set, fewer than two views, n_dtrs != 2 * n_views (ECC_ERR_INVALID_ARGUMENT) or use_corr
 * (ECC_ERR_UNSUPPORTED); n_source outside [1, n_views).  After them n_transforms == 0 is ECC_OK with nothing written.
 * Not built: the full-matrices and strided pose forms of the weighted metric; kept base columns; range, group and RCCL forms;
 * weights under use_corr. */
int ecc_metric_evaluate_weighted_transforms(ecc_metric* m, int n_source, int n_transforms, const double* Ts, double* values,
                                            double* coverages, float* pair_terms);

/* The metric with INVERSE-VARIANCE SAMPLE WEIGHTS (csrc/ecc_variance.hip, csrc/variance_kernel.hip): how noisy
 * a redundant sample is.  In a low-dose or photon-starved scan the variance of a line integral is known from the physics -- it is
 * the integral of the pixel variances along the line --, and the statistically right weight of the squared difference of two such
 * integrals is 1 / (sigma0^2 + sigma1^2).  That is not a product of one weight per view, so no line weights W_i express it, and a
 * robust loss reacts only after the noise has entered d^2.
 *
 * The metric holds 2 * n_views Radon intermediates, channel-major as for ecc_metric_evaluate_weighted: dtr i is the data of view i,
 * dtr n_views + i its VARIANCE FIELD V_i on the same bin grid, normally the unfiltered (ECC_FILTER_NONE) transform of the image of
 * pixel variances; any finite float is taken as it is.  A +-kappa sample of the pair i < j has the positions, kappa range and
 * sampling mode of ecc_metric_evaluate_all; d is that evaluation's difference of the two signed data samples.  Per sample
 *     s     = V_i(sample) + V_j(sample)        one float32 add of two UNSIGNED bilinear samples taken at the data's taps
 *     omega = 1.0f / (s < floor ? floor : s)   one correctly rounded IEEE float32 division
 * The fold sign is never applied to a variance sample.  The value term is the weighted form's with omega in mu's place --
 *     polynomial loops             fmaf(om_p * dp, dp, (om_m * dm) * dm) * w06_dkappa
 *     exact and reference loops    (((om_p * dp) * dp + (om_m * dm) * dm) * K0[6]) * dkappa
 * -- accumulated in float64 per lane in the same trip order and reduced by the same wave tree; beside it each lane adds
 * (double)(om_p + om_m), the weight mass, and 2.0, the sample count.  Per pair q:
 *     c_q = the float32 value,
 *     u_q = (float)(mass / count), the MEAN WEIGHT of the pair's samples; a pair without samples has c_q = 0, u_q = 1.0f.
 *   floor: finite and > 0, in the units of V: the least s a weight is formed from, so that a line through air (V = 0 in both
 *     views) cannot take the whole sum.  ecc_host_variance_floor proposes one from the fields.
 *   *value (required) = sum c_q / sum u_q, *mean_weight (nullable) = sum u_q / n_pairs, both sums in the order of
 *     csrc/ecc_sum_order.h.  sum u_q == 0: 0, 0 and ECC_OK.  Only RELATIVE variances matter to value: a common factor on all V and
 *     the floor cancels.
 *   pair_terms (host, nullable): n_pairs x 2 float32, pair-major in the pair order of get_ij, each row {c_q, u_q}.
 * Model: V is the line integral of the pixel variances up to a constant factor.  For derivative data the same field is used, which
 * ignores the correlation of the two neighbouring lines of the finite difference.
 *
 * The contract (tests/test_gpu_variance.py):
 *   1. V == 0.5f everywhere and floor <= 1: value and the c column have the bits of ecc_metric_evaluate_all, every u_q and
 *      mean_weight are 1.0.
 *   2. V == 0 everywhere and floor == 4: every c_q is exactly 1/4 of ecc_metric_evaluate_all's entry, every u_q is 0.25, value has
 *      ecc_metric_evaluate_all's bits.
 *   3. All V and the floor multiplied by 4: every c_q and u_q is multiplied by 1/4 exactly, value keeps its bits.
 *   4. c_q and u_q agree with a float64 statement (tests/variance_terms.py) to the project's bars.
 *   - The call changes nothing a later call can see.  (It shares ecc_metric_evaluate_gram's scratch.)
 *   - Errors before anything is launched or written, ECC_ERR_INVALID_ARGUMENT, checked in this order: m == NULL, value == NULL, no
 *     matrices set, fewer than two views, n_dtrs != 2 * n_views, a floor that is not finite and > 0.  use_corr set: ECC_ERR_UNSUPPORTED.
 *
 * ecc_metric_evaluate_variance_pairs: an index list of n_pairs tuples (P0, P1, D0, D1) as for ecc_metric_evaluate_weighted_pairs: P*
 * index the current matrices, D* the DATA intermediates in [0, n_views); the variance of a sample comes from dtr n_views + D*.  The
 * sampling mode resolves from the list's length.  With tuples (i, j, i, j) the rows have the bits of ecc_metric_evaluate_variance's
 * rows of those pairs under the same resolved mode.  n_pairs == 0: ECC_OK, nothing written.
 * ecc_metric_evaluate_variance_pose_deltas: the lists of ecc_metric_evaluate_pose_deltas; values[k] and mean_weights[k]
 * (mean_weights nullable) have THE BITS of ecc_metric_set_projections(pose k) + ecc_metric_evaluate_variance
 * (tests/test_gpu_variance_batches.py).  The launches, the batches and what the batch does not take are those of
 * ecc_metric_evaluate_weighted_pose_deltas, with the variance pair kernel in the weighted one's place.
 * ecc_metric_evaluate_variance_transforms: views, transforms and the cross list of ecc_metric_evaluate_weighted_transforms;
 * values[k] = sum c / sum u, mean_weights[k] (nullable) = sum u / count over the list of transform k, pair_terms (nullable)
 * n_transforms x n_target x n_source x 2 floats; all three have THE BITS of ecc_metric_set_projections(the composed matrices) +
 * ecc_metric_evaluate_variance_pairs(that list).
 * The argument checks of the three are those of their weighted siblings, then the floor's.
 *
 * ecc_host_variance_floor (host only, no device): *floor = (float)(fraction x the median of the strictly positive finite entries of
 * v[0 .. count)); an even number of them: the mean of the two middle ones.  ECC_ERR_INVALID_ARGUMENT for a null pointer, a negative
 * count, a fraction that is not in (0, infinity), or no positive entry.
 * Not built: kept base columns; range, group and RCCL forms; the variance form under use_corr; its combination with the robust
 * loss; a covariance-aware model for derivative data. */
int ecc_metric_evaluate_variance(ecc_metric* m, float floor, double* value, double* mean_weight, float* pair_terms);
int ecc_metric_evaluate_variance_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, float floor, double* value, double* mean_weight,
                                       float* pair_terms);
int ecc_metric_evaluate_variance_pose_deltas(ecc_metric* m, int n_poses, const int32_t* moved_offsets, const int32_t* moved_views,
                                             const double* moved_Ps, float floor, double* values, double* mean_weights);
int ecc_metric_evaluate_variance_transforms(ecc_metric* m, int n_source, int n_transforms, const double* Ts, float floor, double* values,
                                            double* mean_weights, float* pair_terms);
int ecc_host_variance_floor(const float* v, int64_t count, double fraction, float* floor);

/* The metric under a PER-SAMPLE ROBUST LOSS (csrc/ecc_robust.hip, csrc/robust_kernel.hip): for callers who do NOT
 * know where the bad lines are -- an instrument nobody flagged, a truncated view, a detector defect that appears mid-scan.  The
 * squared difference lets a few percent of the samples decide the value; line weights (above) need somebody to say which.  Every
 * loss here is rho(d) = w(d) d^2 with an IRLS weight w in (0, 1], so the kernel is the weighted kernel with its per-sample factor
 * computed from the residual instead of gathered: four gathers per kappa step instead of eight, and the same bit-for-bit link to
 * ecc_metric_evaluate_all.
 *
 * For a pair a +-kappa sample has the positions, kappa range and sampling mode of ecc_metric_evaluate_all; d is that evaluation's
 * difference of the two signed data samples.  delta is a float32 > 0; +infinity is allowed and down-weights nothing;
 * inv_delta = (float)(1.0 / (double)delta) is formed on the host.  Per sample, every operation one float32 operation, nothing
 * contracted unless written as fmaf, the division the IEEE one:
 *     a = fabsf(d)        t = fminf(1.0f, delta / a)                       (a == 0: +inf -> 1)
 *     ECC_LOSS_HUBER           w = t * (2.0f - t)                          rho = d^2 inside delta, 2 delta |d| - delta^2 outside
 *     ECC_LOSS_TRUNCATED       w = t * t                                   rho = min(d^2, delta^2)
 *     ECC_LOSS_GEMAN_MCCLURE   s = a * inv_delta; w = 1.0f / fmaf(s, s, 1.0f)   rho = d^2 delta^2 / (delta^2 + d^2)
 * Per kappa step the value term is the weighted call's expression with w in place of mu --
 *     polynomial loops             fmaf(w_p * dp, dp, (w_m * dm) * dm) * w06_dkappa
 *     exact and reference loops    (((w_p * dp) * dp + (w_m * dm) * dm) * K0[6]) * dkappa
 * -- accumulated in float64 per lane in the same trip order and reduced by the same wave tree, so w == 1.0f gives
 * ecc_metric_evaluate_all's bits.  Beside it each lane adds (double)(w_p + w_m), the weight mass, (double)(dp * dp) +
 * (double)(dm * dm), the raw squares (products in float32), and 2.0, the sample count.  Per pair q, three float32 columns:
 *     c_q = the value,
 *     u_q = (float)(mass / count), the mean IRLS weight: the INLIER MASS in (0, 1],
 *     r_q = (float)(raw / count), the mean squared raw residual, independent of loss and delta;
 *     a pair without samples, or a list tuple with P0 == P1, has {0, 1, 0}.
 *   value (required): sum c_q / n_pairs, the sum in the order of csrc/ecc_sum_order.h for that many values, then the division an
 *     all-pairs or list evaluation makes.  A mean, NOT divided by the inlier mass: dividing would reward pushing samples into the tails.
 *   inlier_mass (nullable): sum u_q / n_pairs.
 *   pair_terms (host, nullable): n_pairs x 3 float32, pair-major, rows {c_q, u_q, r_q}; get_ij order (all pairs), list order (list).
 * ecc_metric_evaluate_robust takes whatever metric ecc_metric_evaluate_all takes; the sampling mode resolves from n (n - 1) / 2 as
 * there.  ecc_metric_evaluate_robust_pairs takes (P0, P1, D0, D1) tuples as ecc_metric_evaluate_pairs does; its mode resolves from
 * the list's length; n_pairs == 0: ECC_OK, nothing written.  Both take ECC_SAMPLING_POLYNOMIAL (with its per-pair fallback and exact
 * tail), _PER_SAMPLE and _REFERENCE (one or four waves per pair), a fixed or automatic object radius, a user dkappa, non-derivative
 * data and row-paired and row-quad copies.
 *
 * ecc_host_robust_scale: k x the median of sqrt((double)r_q) over the rows with r_q > 0 (even count: the mean of the two middle
 * values); no such row: 0.0.  Touches no device.  The intended use: one call with delta = INFINITY -- which is also
 * ecc_metric_evaluate_all's value --, then delta = ecc_host_robust_scale(terms, n_pairs, k).  A minority of corrupted views reaches
 * a minority of the pairs, so the median over pairs stays put where the pooled rms does not.
 *
 * The contract (tests/test_gpu_robust.py):
 *   1. delta = +infinity or FLT_MAX: the c column and value have the bits of ecc_metric_evaluate_all (the list form: of
 *      ecc_metric_evaluate_pairs of that list), every u_q and inlier_mass are 1.0.
 *   2. {c, u, r} agree with a float64 oracle (tests/robust_terms.py) to the project's bars.
 *   3. A block pasted into one view: the pairs without that view keep their bits; corrupted / clean is ordered
 *      truncated < Huber < ecc_metric_evaluate_all and Geman-McClure < Huber.
 *   - The calls change nothing a later call can see: current matrices, kept records, the kept values of the pose-delta mode and of
 *     the pose batch.  (They share ecc_metric_evaluate_gram's scratch; the list form stages its tuples in the pose batch's index
 *     scratch.)
 *   - Errors before anything is launched or written, ECC_ERR_INVALID_ARGUMENT: m == NULL (checked first); value == NULL; idx4 == NULL
 *     with n_pairs > 0; n_pairs < 0; loss outside 0..2; delta NaN or <= 0; no matrices set or fewer than two views (the all-pairs
 *     call: fewer intermediates than views); a bad tuple.  ECC_ERR_UNSUPPORTED under use_corr.
 * Launches: the record kernel over all pairs or the list, pairs_robust_kernel -- one wave per pair, the position arithmetic of a
 * kappa step once, 4 gathers --, one launch for the sums of c and u (r is not summed), the copies.
 * Pose deltas and transforms per call: ecc_metric_evaluate_robust_pose_deltas, ecc_metric_evaluate_robust_transforms below.
 * The loss combined with line weights on a 2 n metric: ecc_metric_evaluate_weighted_robust below.
 * Not built: range, group and RCCL forms; the loss under use_corr; Tukey's biweight (not d^2 near zero, so no bit link to
 * ecc_metric_evaluate_all). */
enum { ECC_LOSS_HUBER = 0, ECC_LOSS_TRUNCATED = 1, ECC_LOSS_GEMAN_MCCLURE = 2 };
int ecc_metric_evaluate_robust(ecc_metric* m, int loss, float delta, double* value, double* inlier_mass, float* pair_terms);
int ecc_metric_evaluate_robust_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, int loss, float delta, double* value,
                                     double* inlier_mass, float* pair_terms);
double ecc_host_robust_scale(const float* pair_terms, int64_t n_pairs, double k);

/* Where the robust loss rejects (csrc/ecc_robust_map.hip, csrc/robust_map_kernel.hip): ecc_metric_evaluate_robust
 * with every sample's distrust, 1 - w, accumulated where the sample was taken, in each view's own Radon space.
 *
 * ecc_metric_evaluate_robust_map / _map_pairs take the metric, loss, delta (+infinity allowed), value, inlier_mass and pair_terms of
 * ecc_metric_evaluate_robust / _robust_pairs and return THEIR BITS in them: the kernel forms the same positions, residuals d,
 * weights w and per-lane sums in the same order.  Beside that, per +-kappa sample of a pair and per view of the pair that is MAPPED:
 * the sample's 2 x 2 footprint -- the clamped cells (i0, i1) x (j0, j1) its gather reads, with the fractions fx (angle) and fy
 * (distance) -- and b = (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy, float32 products,
 *     HITS[cell] += b          REJ[cell] += b * (1 - w)          ((1 - w) and the product float32)
 * in that view's planes; view i's two samples of a kappa step lie in view i's planes and view j's in view j's; clamped cells that
 * coincide receive both deposits (the map is the adjoint of the sampling).  On the device the planes are unsigned 64-bit fixed
 * point with quantum 2^-32 (a deposit is the float32 value times 2^32, exact), summed with integer atomics: the same arguments give
 * the same bits on every call, in any order of an index list.  hits, rejected (host, either may be NULL): n_mapped planes of
 * n_t x n_alpha floats, alpha fastest, plane k for views[k]; an entry is (float)((double)q * 2^-32).
 *   views, n_mapped   distinct indices of Radon intermediates, in [0, n_views) for the all-pairs call and in [0, n_dtrs) for the list
 *                     call, where the view of a sample is the tuple's data index (D0 or D1); n_mapped == 0: every one, in order.
 *                     A view that is not listed receives nothing and costs nothing.  A pair listed twice deposits twice.
 *   delta = +infinity REJ is exactly 0 everywhere, value has ecc_metric_evaluate_all's bits.
 * Memory: 16 bytes per padded bin and mapped view on the device, owned by the metric, grown geometrically, freed with it, plus the
 * float planes (8 bytes per bin and mapped view), which the metric HOLDS until the next map call, ecc_metric_refresh_dtrs or
 * ecc_metric_set_params.
 *   - Errors before anything is launched or written, in this order: those of ecc_metric_evaluate_robust[_pairs] in their order
 *     (use_corr: ECC_ERR_UNSUPPORTED); then n_mapped < 0, views == NULL with n_mapped > 0, an index out of range, a duplicate:
 *     ECC_ERR_INVALID_ARGUMENT.  After them the list call with n_pairs == 0 is ECC_OK: planes of zeros, no map held.
 * Launches: the record kernel, the planes' memset, pairs_robust_map_kernel (the reference kernels under the reference arithmetic)
 * between the timing events, the sums of c and u, robust_map_finish_kernel, the copies, one wait.  A diagnostic, meant to be called
 * once per outer iteration of an optimiser: the deposits are 8 to 16 atomics per sample and mapped view.
 *
 * ecc_metric_robust_map_weights: the held map as line weights, one intermediate per mapped view in out[0 .. n_mapped), handles of the
 * kind ecc_dtr_line_weights returns (release them with ecc_dtr_destroy), ready to be the second half of a 2 n metric.  With h and r
 * the float32 plane values of a bin: mu = 1.0f where h < min_hits, else (float)fmax(0.0, 1.0 - (double)gain * ((double)r / (double)h))
 * -- every operation an IEEE float64 one.  One elementwise launch, no wait.
 *   - Errors, ECC_ERR_INVALID_ARGUMENT: m == NULL, out == NULL, min_hits or gain negative or not finite; no map held (no map call yet,
 *     or the map was dropped by ecc_metric_refresh_dtrs / ecc_metric_set_params).
 * The map under line weights (a 2 n metric): ecc_metric_evaluate_weighted_robust_map below.
 * Not built: the map's batches of pose deltas and of transforms, its range, group and RCCL forms; the map under use_corr; an IRLS
 * loop inside the library. */
int ecc_metric_evaluate_robust_map(ecc_metric* m, int loss, float delta, const int32_t* views, int n_mapped, float* hits, float* rejected,
                                   double* value, double* inlier_mass, float* pair_terms);
int ecc_metric_evaluate_robust_map_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, int loss, float delta, const int32_t* views,
                                         int n_mapped, float* hits, float* rejected, double* value, double* inlier_mass, float* pair_terms);
int ecc_metric_robust_map_weights(ecc_metric* m, float min_hits, float gain, ecc_dtr** out);
/* Debug: the fixed-point sums of the held map themselves -- every HITS plane, then every REJ plane, each (n_alpha + 2) rows of
 * `pitch` cells in the padded geometry of a Radon intermediate on the device (cell (row, bin) for the bin (row - 1, bin - 1), the
 * border rows and columns folding into the clamped bins); capacity in cells.  For tests that add maps in fixed point. */
int ecc_debug_robust_map_fixed(ecc_metric* m, uint64_t* out, int64_t capacity);

/* The robust loss for optimisers (csrc/ecc_robust_batches.hip): a population of poses or of source-to-target
 * transforms per call, as ecc_metric_evaluate_pose_deltas / ecc_metric_evaluate_transforms take them for the plain metric and the
 * weighted siblings for line weights.  The losses, delta, the three float32 columns {c, u, r} per pair and the value convention are
 * exactly those of ecc_metric_evaluate_robust: a value is the mean of c over the pairs, never divided by the inlier mass.
 *
 * ecc_metric_evaluate_robust_pose_deltas: the lists of ecc_metric_evaluate_pose_deltas -- pose k = the CURRENT matrices with the
 * views moved_views[moved_offsets[k] .. moved_offsets[k + 1]) (strictly ascending) replaced by moved_Ps[12 q ..]; n_poses < 1:
 * ECC_OK.  values[k] and inlier_masses[k] (inlier_masses nullable) have THE BITS of ecc_metric_set_projections(pose k) +
 * ecc_metric_evaluate_robust(loss, delta) (tests/test_gpu_robust_poses.py).  The call runs in four steps:
 *   1. once per call, the base columns {c, u} (and r) of all pairs at the current matrices: the launches of
 *      ecc_metric_evaluate_robust, recomputed on every call -- kept base columns are not built;
 *   2. per batch, ONE launch that lists the pairs and does E1 of the extended matrices, and ONE record launch over the n x Q grid;
 *   3. per batch, ONE robust pair launch over that grid under the sampling mode (and wave split) of an all-pairs evaluation;
 *   4. per batch, ONE segmented float64 sum per pose of columns c and u, the base's values with the pose's own entries substituted,
 *      in the order of csrc/ecc_sum_order.h.
 * A pose with more than ECC_POSE_BATCH_MAX_MOVED (32) moved views, one that moves view 0 under the automatic object radius and changes
 * it, and every pose after ecc_metric_set_pose_batching(m, 0) is evaluated the sequential way inside the call (same bits);
 * ecc_metric_last_batched_poses reports how many went through the batch.  Calls of more than 2^20 grid entries are cut into batches
 * over the same base columns.
 *
 * ecc_metric_evaluate_robust_transforms: views, transforms, the cross list (entry q = j * n_source + i is the tuple
 * (i, n_source + j, i, n_source + j)) and the batching are those of ecc_metric_evaluate_transforms; count = n_source * n_target.
 *   values[k] (required): sum c / count over the list of transform k;  inlier_masses[k] (nullable): sum u / count.
 *   pair_terms (host, nullable): n_transforms x n_target x n_source x 3 float32, per transform its count rows {c, u, r} in list order.
 * All three have THE BITS of ecc_metric_set_projections(the composed matrices) + ecc_metric_evaluate_robust_pairs(that list, loss,
 * delta) (tests/test_gpu_robust_transforms.py).  So the sampling mode resolves from a list of count tuples, and under the automatic
 * object radius every transform takes the radius of its composed view 0.  Per batch: ecc_metric_evaluate_transforms' list launch and
 * record launch, ONE robust pair launch over the pair-major grid, ONE segmented sum of columns c and u.  A transform whose list
 * alone exceeds a batch, and every transform after ecc_metric_set_pose_batching(m, 0), is evaluated the sequential way inside the call
 * (same bits); ecc_metric_last_batched_transforms counts the batched ones.  Needs at least one Radon intermediate per view and
 * 1 <= n_source < n_views.  n_transforms == 0 (after the checks): ECC_OK, nothing written.
 *
 * Both: with delta = +infinity (or FLT_MAX) values has the bits of ecc_metric_evaluate_pose_deltas / ecc_metric_evaluate_transforms
 * on the same metric, and every inlier mass is 1.0.  The calls leave the metric as they found it: current matrices, kept records,
 * the kept values of the pose-delta mode and of the pose batch.  (They rewrite the pose batch's per-batch scratch and
 * ecc_metric_evaluate_gram's scratch, as their weighted siblings do.)
 * Errors are returned before anything is launched or written, checked in this order: (1) m == NULL: ECC_ERR_INVALID_ARGUMENT;
 * (2) null or negative arguments as in the weighted siblings (moved_offsets / values; Ts / values with n_transforms > 0;
 * n_transforms < 0; the list arrays when moved_offsets[n_poses] > 0); (3) loss outside 0..2, delta NaN or <= 0, no matrices set or
 * fewer than two views, fewer intermediates than views: ECC_ERR_INVALID_ARGUMENT -- use_corr: ECC_ERR_UNSUPPORTED; (4) a bad list,
 * n_source outside [1, n_views).
 * Not built: kept base columns; the full-matrices and strided pose forms; range, group and RCCL forms; pose-delta and transform
 * batches of the loss combined with line weights (ecc_metric_evaluate_weighted_robust below has the all-pairs and list forms); the
 * loss under use_corr. */
int ecc_metric_evaluate_robust_pose_deltas(ecc_metric* m, int n_poses, const int32_t* moved_offsets, const int32_t* moved_views,
                                           const double* moved_Ps, int loss, float delta, double* values, double* inlier_masses);
int ecc_metric_evaluate_robust_transforms(ecc_metric* m, int n_source, int n_transforms, const double* Ts, int loss, float delta,
                                          double* values, double* inlier_masses, float* pair_terms);

/* LINE WEIGHTS AND THE ROBUST LOSS TOGETHER (csrc/ecc_weighted_robust.hip, csrc/weighted_robust_kernel.hip): real
 * scans have both kinds of bad data at once -- a fluoroscopy sequence has collimator blades, known and flagged once per view
 * (ecc_radon_line_weights), and a catheter nobody flagged.  ecc_metric_evaluate_weighted alone leaves the instrument in;
 * ecc_metric_evaluate_robust alone spends its scale on lines whose badness was known in advance, reports an inlier mass that mixes
 * the two causes, and on a 2 n metric would take the weights for data.
 *
 * The metric is ecc_metric_evaluate_weighted's: n_dtrs == 2 * n_views, the data of every view, then its line weights.  For a pair a
 * +-kappa sample has the positions, kappa range and sampling mode of ecc_metric_evaluate_all; d is that evaluation's difference of the
 * two signed data samples.  loss, delta and inv_delta are ecc_metric_evaluate_robust's.  Per sample, every operation one float32
 * operation:
 *     mu = W_i(sample) * W_j(sample)      as in ecc_metric_evaluate_weighted: unsigned taps of the weight intermediates
 *     w  = the IRLS weight of ecc_metric_evaluate_robust's table, of the RAW residual d -- a line weight says how far a line is
 *          trusted, it does not rescale its residual
 *     f  = mu * w
 * Per kappa step the value term is the weighted call's expression with f in place of mu --
 *     polynomial loops             fmaf(f_p * dp, dp, (f_m * dm) * dm) * w06_dkappa
 *     exact and reference loops    (((f_p * dp) * dp + (f_m * dm) * dm) * K0[6]) * dkappa
 * -- accumulated in float64 per lane in the same trip order and reduced by the same wave tree.  Beside it each lane adds
 * (double)(mu_p + mu_m), the weight mass, (double)(f_p + f_m), the mass the loss keeps, (double)(mu_p * (dp * dp)) +
 * (double)(mu_m * (dm * dm)), the weighted raw squares (products in float32), and 2.0, the sample count.  Per pair q, four float32
 * columns:
 *     c_q = the value,
 *     u_q = (float)(mass / count), the COVERAGE of ecc_metric_evaluate_weighted,
 *     k_q = (float)(kept / count), the weight mass the loss keeps; k_q <= u_q for weights >= 0,
 *     r_q = (float)(raw / count), the weighted mean squared raw residual, independent of loss and delta;
 *     a pair without samples, or a list tuple with P0 == P1, has {0, 1, 1, 0}.
 *   value (required): sum c_q / sum u_q, the sums in the order of csrc/ecc_sum_order.h.  Normalised by the line-weight coverage, as
 *     the weighted call does and for its reason; NEVER divided by the mass the loss keeps, as the robust call refuses to and for its
 *     reason.
 *   coverage (nullable): sum u_q / n_pairs.
 *   inlier_mass (nullable): sum k_q / sum u_q, the mean IRLS weight among the lines that are trusted at all.
 *   sum u_q == 0: all three are 0.0 and ECC_OK.
 *   pair_terms (host, nullable): n_pairs x 4 float32, pair-major, rows {c_q, u_q, k_q, r_q}; get_ij order (all pairs), list order
 *     (list).
 * ecc_metric_evaluate_weighted_robust: all pairs over the current matrices; the sampling mode resolves from n (n - 1) / 2.
 * ecc_metric_evaluate_weighted_robust_pairs: (P0, P1, D0, D1) tuples exactly as ecc_metric_evaluate_weighted_pairs takes them: D*
 * must lie in [0, n_views), the weight follows the data index, the mode resolves from the list's length; n_pairs == 0: ECC_OK,
 * nothing written.
 *
 * ecc_host_weighted_robust_scale: k x the median of sqrt((double)r_q / (double)u_q) over the rows with r_q > 0 and u_q > 0 (even
 * count: the mean of the two middle values); no such row: 0.0.  Touches no device.  The intended use: one call with delta = INFINITY
 * -- which is also ecc_metric_evaluate_weighted's value --, then delta = ecc_host_weighted_robust_scale(terms, n_pairs, k).  With
 * every u_q == 1.0f it is ecc_host_robust_scale of the rows {c, k, r}, to the bit.
 *
 * The contract (tests/test_gpu_weighted_robust.py), three bit links that hold by construction:
 *   1. delta = +infinity or FLT_MAX (every w == 1.0f, f == mu): {c, u}, value and coverage have the bits of
 *      ecc_metric_evaluate_weighted, k_q has the bits of u_q, inlier_mass == 1.0.
 *   2. Every weight 1.0f (f == w): {c, k, r}, value and inlier_mass have the bits of ecc_metric_evaluate_robust's {c, u, r}, value
 *      and inlier_mass on the n_views metric over the same data; u_q == 1.0 and coverage == 1.0.
 *   3. Both: the bits of ecc_metric_evaluate_all.
 *   4. {c, u, k, r} agree with a float64 oracle (tests/weighted_robust_terms.py) to the project's bars.
 *   5. With W_v = 0 for one view the pairs with v are {0, 0, 0, 0}; data that differ only on lines of weight 0 give the same bits
 *      (f = 0 * w with w finite for all three losses; the differing data must keep d * d finite for r).
 *   - The calls change nothing a later call can see: current matrices, kept records, the kept values of the pose-delta mode and of
 *     the pose batch.  (They share ecc_metric_evaluate_gram's scratch; the list form stages its tuples in the pose batch's index
 *     scratch.)
 *   - Errors before anything is launched or written, checked in this order: (1) m == NULL: ECC_ERR_INVALID_ARGUMENT; (2) the list
 *     form: n_pairs < 0, idx4 == NULL with n_pairs > 0: ECC_ERR_INVALID_ARGUMENT; (3) ecc_metric_evaluate_robust's conditions in its
 *     order -- value == NULL, loss outside 0..2, delta NaN or <= 0 (+infinity is allowed), no matrices set, fewer than two views:
 *     ECC_ERR_INVALID_ARGUMENT, then use_corr: ECC_ERR_UNSUPPORTED; (4) n_dtrs != 2 * n_views: ECC_ERR_INVALID_ARGUMENT; (5) the list
 *     form: a tuple with an index outside [0, n_views): ECC_ERR_INVALID_ARGUMENT.  After them n_pairs == 0 is ECC_OK.
 * Launches: the record kernel over all pairs or the list, pairs_weighted_robust_kernel -- one wave per pair, the position arithmetic
 * of a kappa step once, 8 gathers --, one launch for the sums of c, u and k (r is not summed), the copies.
 * Not built: the pose-delta and transform batches of this form (they need no kernel beyond this one); range, group and RCCL forms;
 * use_corr; Tukey's biweight; a 1 / (sigma0^2 + sigma1^2) variance form. */
int ecc_metric_evaluate_weighted_robust(ecc_metric* m, int loss, float delta, double* value, double* coverage,
                                        double* inlier_mass, float* pair_terms);
int ecc_metric_evaluate_weighted_robust_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, int loss, float delta,
                                              double* value, double* coverage, double* inlier_mass, float* pair_terms);
double ecc_host_weighted_robust_scale(const float* pair_terms, int64_t n_pairs, double k);

/* Where the robust loss rejects UNDER LINE WEIGHTS (csrc/ecc_weighted_robust_map.hip, csrc/weighted_robust_map_kernel.hip, DESIGN.md
 * 4.25): ecc_metric_evaluate_robust_map for a metric that already carries weights -- an earlier pass's, a collimator flag from
 * ecc_radon_line_weights, both -- so that the loss and the line weights can be iterated.
 *
 * ecc_metric_evaluate_weighted_robust_map / _map_pairs take the metric (n_dtrs == 2 * n_views), loss, delta, value, coverage,
 * inlier_mass and pair_terms of ecc_metric_evaluate_weighted_robust / _weighted_robust_pairs and return THEIR BITS in them, the
 * n_pairs x 4 rows {c, u, k, r} included.  Beside that, per +-kappa sample of a pair with the weight product mu = W_i * W_j and the
 * loss weight w of its raw residual, per view of the pair that is mapped and per cell of the sample's footprint in that view, with
 * the float32 footprint products b of ecc_metric_evaluate_robust_map:
 *     x = b * mu          HITS[cell] += x          REJ[cell] += x * (1 - w)          (all float32)
 * mu is the product of BOTH views' weights in either view's planes.  The planes, their fixed point (quantum 2^-32, integer
 * atomics: the same arguments give the same bits in any order), hits, rejected, views and n_mapped are those of
 * ecc_metric_evaluate_robust_map, with `views` distinct DATA indices in [0, n_views) for both forms: weight and map follow the data
 * index.  The metric holds the float planes in the same place, and remembers which kind of map it holds;
 * ecc_debug_robust_map_fixed serves both kinds.
 *   delta = +infinity REJ is exactly 0 everywhere; value and coverage have ecc_metric_evaluate_weighted's bits.
 *   every weight 1.0f the fixed-point sums are those of ecc_metric_evaluate_robust_map on the n-metric over the same data.
 *   weights          are expected in [0, 1] (what ecc_radon_line_weights, ecc_dtr_line_weights and the map's own weights produce).
 *                    Outside that range value, coverage, inlier_mass and pair_terms are still ecc_metric_evaluate_weighted_robust's
 *                    and nothing is written out of bounds; the PLANES ARE UNSPECIFIED.
 *   - Errors before anything is launched or written, in this order: those of ecc_metric_evaluate_weighted_robust[_pairs] in their
 *     order; then the views list's as for ecc_metric_evaluate_robust_map.  After them n_pairs == 0 is ECC_OK: planes of zeros, no map
 *     held.
 * Launches: ecc_metric_evaluate_robust_map's sequence with pairs_weighted_robust_map_kernel (8 gathers per kappa step) and the sums of
 * c, u and k.  A diagnostic, once per outer iteration.
 *
 * ecc_metric_weighted_robust_map_weights: the next pass's weights from the held map, one intermediate per mapped view v in
 * out[0 .. n_mapped), handles as ecc_metric_robust_map_weights returns them: per padded element W_v * factor, one float32 multiply,
 * W_v read from the CURRENT contents of intermediate n_views + v and factor ecc_metric_robust_map_weights' rule on the held float
 * planes.  One elementwise launch, no wait.  ecc_metric_robust_map_weights itself refuses a map made by these calls.
 *   - Errors, ECC_ERR_INVALID_ARGUMENT: as ecc_metric_robust_map_weights; the held map is not one of these calls'.
 * Not built: pose-delta and transform batches of either map; range, group and RCCL forms; use_corr; Tukey's biweight; an IRLS loop
 * inside the library (the Python layer's refine_line_weights iterates the calls); a wave-level pre-sum of the deposits. */
int ecc_metric_evaluate_weighted_robust_map(ecc_metric* m, int loss, float delta, const int32_t* views, int n_mapped,
        float* hits, float* rejected, double* value, double* coverage, double* inlier_mass, float* pair_terms);
int ecc_metric_evaluate_weighted_robust_map_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, int loss, float delta,
        const int32_t* views, int n_mapped, float* hits, float* rejected,
        double* value, double* coverage, double* inlier_mass, float* pair_terms);
int ecc_metric_weighted_robust_map_weights(ecc_metric* m, float min_hits, float gain, ecc_dtr** out);

/* Line weights and the robust loss together, for optimisers (csrc/ecc_weighted_robust_batches.hip, csrc/form_sums_kernel.hip,
 * DESIGN.md 4.26): a population of poses or of source-to-target transforms per call, as the plain, the weighted and the robust
 * siblings take them.  This block supersedes the "Not built" sentences of the robust-batches block and of the weighted-robust block
 * above where they name the pose-delta and transform batches of the combined form: they are built here.  The metric, the losses,
 * delta, the four float32 columns {c, u, k, r} per pair and the three results are exactly those of
 * ecc_metric_evaluate_weighted_robust: n_dtrs == 2 * n_views, value = sum c / sum u, coverage = sum u / count, inlier mass =
 * sum k / sum u; sum u == 0 gives 0.0 for all three and ECC_OK.
 *
 * ecc_metric_evaluate_weighted_robust_pose_deltas: the lists of ecc_metric_evaluate_pose_deltas; n_poses < 1: ECC_OK.  values[k],
 * coverages[k] and inlier_masses[k] (the latter two nullable) have THE BITS of ecc_metric_set_projections(pose k) +
 * ecc_metric_evaluate_weighted_robust(loss, delta) (tests/test_gpu_weighted_robust_poses.py).  The steps are those of
 * ecc_metric_evaluate_robust_pose_deltas with the weighted-robust pair launch, and in step 4 ONE segmented float64 sum per pose of the
 * three columns c, u and k in one walk of the pose's grid entries (r is not summed).  The fallbacks (more than
 * ECC_POSE_BATCH_MAX_MOVED moved views, view 0 moved under the automatic object radius, batching off), the cut at 2^20 grid entries
 * and ecc_metric_last_batched_poses are the siblings'.
 *
 * ecc_metric_evaluate_weighted_robust_transforms: views, transforms, the cross list and the batching of
 * ecc_metric_evaluate_transforms; count = n_source * n_target.  values[k] (required), coverages[k], inlier_masses[k] (nullable) and
 *   pair_terms (host, nullable): n_transforms x n_target x n_source x 4 float32, per transform its count rows {c, u, k, r} in list
 *   order
 * have THE BITS of ecc_metric_set_projections(the composed matrices) + ecc_metric_evaluate_weighted_robust_pairs(that list, loss,
 * delta) (tests/test_gpu_weighted_robust_transforms.py).  A transform whose list alone exceeds a batch, and every transform after
 * ecc_metric_set_pose_batching(m, 0), is evaluated the sequential way inside the call (same bits);
 * ecc_metric_last_batched_transforms counts the batched ones.  n_transforms == 0 (after the checks): ECC_OK, nothing written.
 *
 * Both: delta = +infinity (or FLT_MAX) gives values and coverages the bits of ecc_metric_evaluate_weighted_pose_deltas /
 * ecc_metric_evaluate_weighted_transforms and every inlier mass 1.0; weights of 1.0f give values and inlier masses the bits of
 * ecc_metric_evaluate_robust_pose_deltas / ecc_metric_evaluate_robust_transforms on the n_views metric and every coverage 1.0.  The
 * calls leave the metric as they found it, as the siblings do.
 * Errors are returned before anything is launched or written.  Pose form, in this order: m == NULL; moved_offsets or values NULL:
 * ECC_ERR_INVALID_ARGUMENT; (n_poses < 1: ECC_OK); the list arrays NULL with moved_offsets[n_poses] > 0; the conditions of
 * ecc_metric_evaluate_weighted_robust in its order (use_corr: ECC_ERR_UNSUPPORTED; n_dtrs != 2 * n_views); a bad list.  Transform
 * form: m == NULL; n_transforms < 0; Ts or values NULL with n_transforms > 0; the conditions of ecc_metric_evaluate_weighted_robust;
 * n_source outside [1, n_views).
 * Not built: kept base columns; the full-matrices and strided pose forms; range, group and RCCL forms; use_corr; the batches of the
 * maps (ecc_metric_evaluate_robust_map, ecc_metric_evaluate_weighted_robust_map). */
int ecc_metric_evaluate_weighted_robust_pose_deltas(ecc_metric* m, int n_poses, const int32_t* moved_offsets, const int32_t* moved_views,
                                                    const double* moved_Ps, int loss, float delta, double* values, double* coverages,
                                                    double* inlier_masses);
int ecc_metric_evaluate_weighted_robust_transforms(ecc_metric* m, int n_source, int n_transforms, const double* Ts, int loss, float delta,
                                                   double* values, double* coverages, double* inlier_masses, float* pair_terms);

/* Inverse-variance sample weights and the robust loss together: the loss in sigma units (csrc/ecc_variance_robust.hip,
 * csrc/variance_robust_kernel.hip).  This block supersedes the "Not built" sentences of the variance block and of the
 * weighted-robust block above where they name the combination of the variance form with the robust loss: it is built here.  A
 * low-dose sequence has photon-starved lines whose variance is known, and an instrument nobody flagged.
 * ecc_metric_evaluate_robust thresholds the raw residual d, so a line that is merely noisy, and known to be, is rejected as an
 * outlier; ecc_metric_evaluate_variance keeps the instrument at full weight.  Here the loss is applied to the studentised residual
 * z = d / sigma with sigma^2 = V_i + V_j, and delta is "so many sigmas".
 *
 * The metric is ecc_metric_evaluate_variance's: n_dtrs == 2 * n_views, the data of every view, then its variance field.  Positions,
 * kappa range, sampling mode and d are those of ecc_metric_evaluate_all.  loss and delta as for ecc_metric_evaluate_robust:
 * ECC_LOSS_*, float32 > 0, +infinity allowed; inv_delta = (float)(1.0 / (double)delta) is formed on the host.  floor as for
 * ecc_metric_evaluate_variance: finite, > 0.  Per sample, every operation is one float32 operation, nothing is contracted but the
 * written fmaf, division and square root are the compiler's correctly rounded ones (no intrinsic, no fast-math flag):
 *     s   = V_i(sample) + V_j(sample)            unsigned taps, as in the variance form
 *     sc  = s < floor ? floor : s
 *     om  = 1.0f / sc
 *     a   = fabsf(d)
 *     HUBER, TRUNCATED:   thr = delta * sqrtf(sc);  t = fminf(1.0f, thr / a);   w = t * (2.0f - t)  |  t * t
 *     GEMAN_MCCLURE:      q = a * inv_delta;        w = 1.0f / fmaf(q * om, q, 1.0f)
 *     f   = om * w
 * The value term is the weighted call's with f in mu's place, in the polynomial and in the exact / reference wording.  Beside it,
 * per +-kappa step: mass (double)(om_p + om_m), kept (double)(f_p + f_m), raw (double)(om_p * (dp * dp)) + (double)(om_m * (dm * dm)),
 * count 2.0.  Per pair four float32 columns {c, u, k, r}: c the value, u = mass / count the mean weight, k = kept / count the weight
 * mass the loss keeps, r = raw / count the mean squared studentised residual -- a reduced chi^2 of the pair, free of loss and
 * delta.  A pair with no trip, or a tuple with P0 == P1, has {0, 1, 1, 0}.  The column sums are added in the order of
 * ecc_sum_order.h:
 *     *value       = sum c / sum u     (never divided by the kept mass)
 *     *mean_weight = sum u / n_pairs   (nullable)
 *     *inlier_mass = sum k / sum u     (nullable)
 * sum u == 0 gives 0, 0, 0 and ECC_OK.  pair_terms (host, nullable): n_pairs x 4 float32 rows {c, u, k, r}.
 *
 * ecc_host_variance_robust_scale (host only, no device): k x the median of sqrt((double)r_q) over the rows {c, u, k, r} with
 * r_q > 0; an even count takes the mean of the two middle values; no such row gives 0.0.  V is the line variance only up to a
 * constant factor, so this call calibrates "one sigma" from the data: one call at delta = +infinity, then delta = scale(terms, n, k).
 *
 * By construction (tests/test_gpu_variance_robust.py holds each to the bit):
 *   1. delta = +infinity gives {c, u}, value and mean_weight the bits of ecc_metric_evaluate_variance; k has u's bits and
 *      inlier_mass == 1.0.
 *   2. V == 0.5f everywhere with floor <= 1 gives {c, k, r}, value and inlier_mass the bits of ecc_metric_evaluate_robust's {c, u, r}
 *      at the same loss and delta on the n_views metric; u == 1.0 and mean_weight == 1.0.
 *   3. Both together give the bits of ecc_metric_evaluate_all.
 *   4. All V and the floor x 4 with delta x 1/2 multiply every column by 1/4 exactly; value and inlier_mass keep their bits.
 *
 * ecc_metric_evaluate_variance_robust_pairs: an index list as for ecc_metric_evaluate_variance_pairs; with tuples (i, j, i, j) the
 * rows have the bits of the all-pairs rows under the same resolved sampling mode.
 * ecc_metric_evaluate_variance_robust_pose_deltas: the lists of ecc_metric_evaluate_pose_deltas; values[k], mean_weights[k] and
 * inlier_masses[k] (the latter two nullable) have THE BITS of ecc_metric_set_projections(pose k) +
 * ecc_metric_evaluate_variance_robust; what the batch does not take is evaluated sequentially inside the call.
 * ecc_metric_evaluate_variance_robust_transforms: views, transforms and the cross list of ecc_metric_evaluate_variance_transforms;
 * every result and the pair rows (n_transforms x n_target x n_source x 4) have THE BITS of ecc_metric_set_projections(the composed
 * matrices) + ecc_metric_evaluate_variance_robust_pairs(that list); the fallback is sequential, inside the call.
 *
 * Errors are returned before anything is launched or written, in this order: m == NULL; list form: n_pairs < 0, or idx4 == NULL with
 * n_pairs > 0 (pose form: moved_offsets or values NULL, then n_poses < 1: ECC_OK, then the list arrays NULL with entries; transform
 * form: n_transforms < 0, Ts or values NULL with n_transforms > 0); value == NULL, loss outside 0..2, delta NaN or <= 0; the
 * conditions of ecc_metric_evaluate_variance in its order -- no matrices, fewer than two views, n_dtrs != 2 * n_views, a floor that is
 * not finite and > 0: ECC_ERR_INVALID_ARGUMENT, then use_corr: ECC_ERR_UNSUPPORTED; list form: a bad tuple (pose form: a bad list;
 * transform form: n_source outside [1, n_views)).  After these checks n_pairs == 0 is ECC_OK with nothing written.  The calls change
 * nothing a later call can see.
 * Not built: kept base columns; range, group and RCCL forms; use_corr; a covariance-aware model for derivative data.
 * (Listed here before and built since: the maps of this form, ecc_metric_evaluate_variance_robust_map below.) */
int ecc_metric_evaluate_variance_robust(ecc_metric* m, int loss, float delta, float floor, double* value, double* mean_weight,
                                        double* inlier_mass, float* pair_terms);
int ecc_metric_evaluate_variance_robust_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, int loss, float delta, float floor,
                                              double* value, double* mean_weight, double* inlier_mass, float* pair_terms);
int ecc_metric_evaluate_variance_robust_pose_deltas(ecc_metric* m, int n_poses, const int32_t* moved_offsets, const int32_t* moved_views,
                                                    const double* moved_Ps, int loss, float delta, float floor, double* values,
                                                    double* mean_weights, double* inlier_masses);
int ecc_metric_evaluate_variance_robust_transforms(ecc_metric* m, int n_source, int n_transforms, const double* Ts, int loss, float delta,
                                                   float floor, double* values, double* mean_weights, double* inlier_masses, float* pair_terms);
double ecc_host_variance_robust_scale(const float* pair_terms, int64_t n_pairs, double k);

/* The form batches' base columns kept between pose-delta calls (opt-in, default off; not in the reference; csrc/ecc_form_base.h,
 * csrc/ecc_form_call.h, csrc/form_base_scatter_kernel.hip).  This block supersedes the "Not built" sentences of the
 * weighted, robust, weighted-robust, variance and variance-robust blocks above where they name kept base columns: they are built
 * here, for these five calls.
 * ecc_metric_evaluate_weighted_pose_deltas, _robust_pose_deltas, _weighted_robust_pose_deltas, _variance_pose_deltas and
 * _variance_robust_pose_deltas begin every call with the form's T columns over ALL n (n - 1) / 2 pairs of the current matrices, although
 * their caller -- a pose optimiser: set one view, probe -- changed one view since its previous call, or none.  With the mode on the
 * metric keeps those columns in a buffer of its own (T columns of n (n - 1) / 2 float32; ecc_metric_device_bytes counts it under
 * other_bytes; the all-pairs, list, map, transform and Gram calls use other scratch and neither see nor disturb it), together with
 * what they belong to: the form, T and S; loss, delta and floor bitwise, as the form has them; the sampling mode the call resolved
 * and the scalar parameters of its launch (the object radius it resolved, dkappa, the polynomial tolerance, use_corr); n_views and
 * n_dtrs; the n x 12 matrices.  The next of the five calls, in this order:
 *   miss     nothing is kept; one of these fields other than the matrices differs (another form is a miss: ONE form's columns are
 *            kept at a time); the resolved mode is ECC_SAMPLING_REFERENCE; more than min(ECC_POSE_BATCH_MAX_MOVED, n_views / 4) views
 *            differ bitwise from the kept matrices; view 0 differs and the automatic object radius moved with it.  Everything is
 *            evaluated as with the mode off, into the kept buffer, and the key and the matrices are taken.  Under
 *            ECC_SAMPLING_REFERENCE -- chosen, or resolved by ECC_SAMPLING_AUTO for up to ECC_SAMPLING_AUTO_REFERENCE_PAIRS pairs --
 *            NOTHING IS EVER KEPT: that mode reads the callers' slabs, which are current without ecc_metric_refresh_dtrs.
 *   hit      no view differs: no record launch and no pair launch for the base.
 *   refresh  1 <= c <= the limit views differ: ONE pose grid of c columns (the changed views at their current matrices over the
 *            current matrices: the launches of a batch of one pose) and one copy launch from its T columns to the pairs' all-pairs
 *            positions in the kept columns.  A grid entry has the bits of the all-pairs launch for the same two matrices -- the
 *            contract of the batches themselves -- so the refreshed columns have the bits of a full evaluation.
 * Then the call proceeds as with the mode off, reading the kept columns: the batches, their segmented sums, the sequential route for
 * what the batches do not take.  EVERY VALUE A CALL RETURNS HAS THE BITS OF THE SAME CALL WITH THE MODE OFF
 * (tests/test_gpu_form_incremental.py).  With the mode off nothing changes: the same launches with the same arguments and scratch.
 * The kept columns are dropped by ecc_metric_set_form_incremental itself (any call of it), ecc_metric_refresh_dtrs (any non-empty
 * range), ecc_metric_set_params, ecc_metric_set_sampling, ecc_debug_set_poly_tolerance and a change of n_views in
 * ecc_metric_set_projections.  As with every metric here, slab contents changed WITHOUT ecc_metric_refresh_dtrs are not seen by the
 * polynomial and per-sample modes, kept columns or not.
 * ecc_metric_last_form_base_pairs: how many BASE pairs the last *_pose_deltas call of any of the five forms evaluated --
 * n (n - 1) / 2 with the mode off or on a miss, c (n - 1) - c (c - 1) / 2 when c views were refreshed, 0 on a hit, and 0 when the call
 * computed no base columns at all (ecc_metric_set_pose_batching(m, 0)); a call that returns before its lists are looked at
 * (n_poses < 1, an argument error) leaves the count as it was.
 * Errors: m == NULL, and pairs == NULL for the counter: ECC_ERR_INVALID_ARGUMENT.
 * Not built: the kept columns for the all-pairs form calls, the index-list, transform and map calls and ecc_metric_evaluate_gradient;
 * more than one kept form at a time; range, group and RCCL forms; a default-on or automatic mode. */
int ecc_metric_set_form_incremental(ecc_metric* m, int enable);
int ecc_metric_last_form_base_pairs(const ecc_metric* m, int64_t* pairs);

/* Where the robust loss rejects IN SIGMA UNITS (csrc/ecc_variance_robust_map.hip, csrc/variance_robust_map_kernel.hip):
 * the map of ecc_metric_evaluate_variance_robust, and the held map as the next pass's variance fields.  This block supersedes the
 * "Not built" sentence of the block above where it names the maps of that form.  A map of the raw-residual loss
 * (ecc_metric_evaluate_robust_map) points at the lines that are known to be noisy; this one studentises first.
 *
 * ecc_metric_evaluate_variance_robust_map / _map_pairs take the metric (n_dtrs == 2 * n_views: the data, then the variance
 * fields), loss, delta, floor, value, mean_weight, inlier_mass and pair_terms of ecc_metric_evaluate_variance_robust / _pairs and
 * return THEIR BITS in them, the n_pairs x 4 rows {c, u, k, r} included.  Beside that, per +-kappa sample of a pair with the loss
 * weight w of its studentised residual (w alone: t * (2 - t), t * t or 1 / fmaf(q * om, q, 1), never f = om * w), per view of the
 * pair that is mapped and per cell of the sample's footprint in that view, with the float32 footprint products b of
 * ecc_metric_evaluate_robust_map:
 *     HITS[cell] += b          REJ[cell] += b * (1 - w)          (all float32)
 * The deposits are in COUNT units: they are not multiplied by om, which carries the data's units and reaches 1 / floor.
 * REJ / HITS is then the share of a bin's samples whose |z| exceeded delta, which has a known expectation under a correct noise
 * model.  REJ deposits with w == 1.0f are skipped; no address depends on w.  The planes, their fixed point (quantum 2^-32, integer
 * atomics: the same arguments give the same bits in any order), hits, rejected, views and n_mapped are those of
 * ecc_metric_evaluate_robust_map, with `views` distinct DATA indices in [0, n_views) for both forms, n_mapped == 0: every view.  The
 * metric holds the float planes in the same place and remembers which of the three kinds of map it holds;
 * ecc_debug_robust_map_fixed serves all of them.
 *   delta = +infinity      REJ is exactly 0 everywhere and HITS has the bits of ecc_metric_evaluate_robust_map's on the n-metric
 *                          over the same data, whatever V is.
 *   V == 0.5f, floor <= 1  the fixed-point sums are those of ecc_metric_evaluate_robust_map on the n-metric at the same loss and delta.
 *   V and floor x 4, delta x 1/2   both planes keep their bits.
 *   - Errors before anything is launched or written, in this order: those of ecc_metric_evaluate_variance_robust[_pairs] in their
 *     order; then the views list's as for ecc_metric_evaluate_robust_map.  After them n_pairs == 0 is ECC_OK: planes of zeros, no map
 *     held.
 * Launches: ecc_metric_evaluate_robust_map's sequence with pairs_variance_robust_map_kernel (8 gathers per kappa step) and the sums of
 * c, u and k.  A diagnostic, once per outer iteration.
 *
 * ecc_metric_variance_robust_map_variances: the next pass's variance fields from the held map, one intermediate per mapped view v in
 * out[0 .. n_mapped), handles as ecc_metric_robust_map_weights returns them.  One elementwise launch, no wait; every padded element e
 * of every slab is written.  With old = V_v[e] read from the CURRENT contents of intermediate n_views + v, h and r the held float
 * planes at the bin that e replicates and half = 0.5f * floor (exact):
 *     mu     = h < min_hits ? 1.0f : (float)fmax(0.0, 1.0 - (double)gain * ((double)r / (double)h))      ecc_metric_robust_map_weights' rule
 *     factor = (mu * max_factor <= 1.0f) ? max_factor : 1.0f / mu                                        float32
 *     out    = factor == 1.0f ? old : (old < half ? half : old) * factor                                 float32
 * V / mu is the IRLS reading: a sample's effective variance is sigma^2 / w, and mu is the mean w that reached the bin.  The raise to
 * half the floor lets a field of zeros (a clean view) be raised at all; two raised samples sum to the floor exactly.  A bin with
 * factor == 1 keeps its bits: a map that rejected nothing, or max_factor == 1, returns V.
 *   - Errors, ECC_ERR_INVALID_ARGUMENT, in this order: m or out NULL; floor not finite and > 0; min_hits, gain not finite and >= 0;
 *     max_factor not finite and >= 1; no map held, or the held map is not one of these calls' (ecc_metric_robust_map_weights and
 *     ecc_metric_weighted_robust_map_weights in turn refuse a map of this kind).
 * Not built: pose-delta and transform batches of any map; range, group and RCCL forms; use_corr; a third plane of squared residuals
 * (a per-bin excess-variance estimate in place of 1 / mu); an IRLS loop inside the library (the Python layer's refine_variances
 * iterates the calls). */
int ecc_metric_evaluate_variance_robust_map(ecc_metric* m, int loss, float delta, float floor, const int32_t* views, int n_mapped,
        float* hits, float* rejected, double* value, double* mean_weight, double* inlier_mass, float* pair_terms);
int ecc_metric_evaluate_variance_robust_map_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, int loss, float delta, float floor,
        const int32_t* views, int n_mapped, float* hits, float* rejected,
        double* value, double* mean_weight, double* inlier_mass, float* pair_terms);
int ecc_metric_variance_robust_map_variances(ecc_metric* m, float floor, float min_hits, float gain, float max_factor, ecc_dtr** out);

/* The distribution of the per-sample residual, per view, from one pair launch (csrc/ecc_residual_histogram.hip,
 * csrc/residual_histogram_kernel.hip, csrc/ecc_histogram_host.h).  Every robust call above takes a scale delta, and
 * ecc_host_robust_scale can only propose one from per-pair figures, which the outliers themselves pull up; the maps say where a loss
 * rejected at a delta somebody already chose.  These calls count the samples themselves, before any delta exists: delta from sample
 * quantiles ("1.48 x the median absolute residual", "reject the worst 5 %"), a per-view tail share that names the view with the
 * instrument, and in sigma units the calibration check of a variance model (the share of |z| below 1).
 *
 * counts is n_views x n_bins, row-major, and is WRITTEN COMPLETELY.  Row v holds every +-kappa sample of every evaluated pair that has
 * v as one of its two DATA indices (the list forms: D0 and D1, both in [0, n_views)): a sample counts once in each of its pair's two
 * rows.  A row's sum is that view's sample count, the sum over all cells 2 x the samples.  Counts are integers, added with integer
 * atomics: the same arguments give the same bits in any launch order.
 *
 * ecc_metric_evaluate_residual_histogram / _pairs take whatever metric ecc_metric_evaluate_robust / _pairs take.  Positions, kappa
 * range, sampling mode and the residual d of a sample are that call's, in every loop class.  Per sample, every line one float32
 * operation:
 *     a   = fabsf(d)
 *     x   = a * inv_width                                      inv_width = (float)(1.0 / (double)width), formed on the host
 *     bin = x < (float)(n_bins - 1) ? (int)x : n_bins - 1      NaN and +inf land in the last bin: the last bin is the OVERFLOW bin
 * so bin k < n_bins - 1 holds the samples with k <= |d| * inv_width < k + 1.  Doubling width halves inv_width exactly: the bins of
 * width 2 w are pairs of the bins of width w, bit for bit.
 *
 * ecc_metric_evaluate_variance_residual_histogram / _pairs take ecc_metric_evaluate_variance_robust's metric (n_dtrs == 2 * n_views:
 * the data, then the variance fields) and bin the STUDENTISED residual with that call's own statements: s = V_i + V_j from the
 * UNSIGNED samples at the data's taps, sc = s < floor ? floor : s, a = fabsf(d) / sqrtf(sc) (the correctly rounded division and
 * root), then x and bin as above; width counts sigmas.  floor as for ecc_metric_evaluate_variance.
 *   V == 0.5f, floor <= 1          the counts of the raw form on the n-metric over the same data, bit for bit.
 *   V and floor x 4, width x 1/2   the counts keep their bits.
 *   - width: finite and > 0, and so must inv_width be.  n_bins: a multiple of 64 with 64 <= n_bins <= 1024.
 *   - Errors before anything is launched or written, in this order: ECC_ERR_INVALID_ARGUMENT for m NULL; counts NULL; a bad width
 *     or n_bins; the list forms' n_pairs < 0 or (n_pairs > 0 and idx4 NULL); no projection matrices; fewer than two views; the
 *     variance forms' n_dtrs != 2 * n_views or bad floor (the raw forms: fewer intermediates than matrices, behind use_corr as for
 *     ecc_metric_evaluate_robust); ECC_ERR_UNSUPPORTED for use_corr; ECC_ERR_INVALID_ARGUMENT for list indices out of range.
 *     After them n_pairs == 0 is ECC_OK: counts is all zeros.
 * Launches: a column-form call's without value columns -- E1 if needed, k01_kernel, the memset of the table, ONE pair launch
 * (pairs_residual_histogram_kernel or pairs_variance_residual_histogram_kernel, in ECC_SAMPLING_REFERENCE their reference kernels)
 * between the timing events, the copy of the table, one wait.  Each wave counts into a private sub-histogram in LDS and adds its
 * non-zero bins to the pair's two rows when its pair is done: one LDS atomic per sample (measured at 400 views: 0.82 to 0.98 x
 * pairs_robust_kernel's time, min 0.811 and max 0.977 over the windows).
 * The current matrices and everything the metric keeps stay.
 *
 * ecc_host_histogram_quantile (host only, no device): the q-quantile of the binned quantity from one row of counts, or from the
 * caller's sum of rows, at the width the counts were made with.  Linear interpolation inside the bin where the cumulative count
 * crosses q x total: (k + (q total - below) / counts[k]) * width.  +infinity when the crossing lies in the overflow bin (widen and
 * call again); 0.0 for an empty row, for counts NULL or n_bins < 1; NaN for q outside [0, 1] or a width that is not finite and > 0.
 *
 * Not built: pose-delta and transform batches; the form under line weights (counts would not be integers); range, group and RCCL
 * forms; use_corr. */
int ecc_metric_evaluate_residual_histogram(ecc_metric* m, float width, int n_bins, uint64_t* counts);
int ecc_metric_evaluate_residual_histogram_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, float width, int n_bins, uint64_t* counts);
int ecc_metric_evaluate_variance_residual_histogram(ecc_metric* m, float floor, float width, int n_bins, uint64_t* counts);
int ecc_metric_evaluate_variance_residual_histogram_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, float floor, float width, int n_bins,
        uint64_t* counts);
double ecc_host_histogram_quantile(const uint64_t* counts, int n_bins, double width, double q);   /* host only */

/* Multi-GPU building block: evaluate only pairs ij in [first, first+count) of the get_ij order
 * (ref: EpipolarConsistencyCommon.hxx:52-79); returns the partial sum (float64) -- the caller
 * all-reduces {sum, count}.  pair_values (host, nullable) receives `count` floats. */
int ecc_metric_evaluate_range(ecc_metric* m, int64_t first, int64_t count, float* pair_values,
                              double* partial_sum);

/* Asynchronous form for callers that own the device buffers (torch): nothing is copied to the
 * host and the call does not synchronise.  pair_values_d: `count` floats on the device
 * (nullable); sum_d: one double on the device, overwritten with the partial sum. */
int ecc_metric_evaluate_range_async(ecc_metric* m, int64_t first, int64_t count,
                                    float* pair_values_d, double* sum_d);

/* Companions of ecc_metric_evaluate_range_async for the one-process-per-GPU form: after the collective that adds the
 * ranks' partial sums has been queued on the context's stream (an RCCL all-reduce of sum_d), ecc_metric_publish_scalar
 * queues a one-thread kernel behind it that stores *value_d into the metric's pinned result slot, and
 * ecc_metric_wait_scalar polls that slot (bounded, like ecc_metric_evaluate_all's wait): the reduced value reaches the
 * host without a device-to-host copy command and its stream synchronisation. */
int ecc_metric_publish_scalar(ecc_metric* m, const double* value_d);
int ecc_metric_wait_scalar(ecc_metric* m, double* value);

/* Index-list evaluate, ref: evaluate(const std::vector<Eigen::Vector4i>&, float*)
 * (…RadonIntermediate.cpp:267-322).  idx4: n_pairs x 4 int32 on the host.  Indices are range
 * checked in every build (the reference only checks under _DEBUG, .cpp:248-264). */
int ecc_metric_evaluate_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, float* out,
                              double* mean);

/* ref: MetricRadonIntermediate::evaluateForImagePair(i, j, redundant_samples0, redundant_samples1, kappas,
 * radon_samples0, radon_samples1) (...RadonIntermediate.cpp:324-393, "visualization only"): the two
 * redundant signals of ONE pair over kappa in (-kappa_max, kappa_max) with num_samples = image diagonal
 * (:349) and the fp32-accumulated kappa loop (:367).  The reference does this on the host from read-back
 * dtrs; here one small kernel samples the device-resident dtrs.  The evident intent is implemented where
 * the reference code is unfinished: the (alpha+pi, -t) fold flips the sign of derivative
 * dtrs, sampling uses the metric's own texel rule, and *ecc = SUM (v0-v1)^2 dkappa (the reference assigns).
 * All output arrays are on the host and nullable; each holds `capacity` entries (radon_samples: 2 floats
 * per sample = texture coordinates (angle, distance) in [0,1]).  *n_samples receives the number of samples;
 * fails with ECC_ERR_INVALID_ARGUMENT (and *n_samples set) when capacity is too small --
 * ecc_metric_pair_samples_bound gives a sufficient capacity.  K01 (nullable) receives 16 floats. */
int ecc_metric_pair_samples_bound(const ecc_metric* m, int* capacity);
int ecc_metric_evaluate_for_image_pair(ecc_metric* m, int i, int j, int capacity, int* n_samples,
                                       float* redundant_samples0, float* redundant_samples1, float* kappas,
                                       float* radon_samples0, float* radon_samples1, float* K01,
                                       double* ecc);

/* Debug: the 16 K01 floats per pair the kernel used (ref: kernelEpipolarConsistencyComputeK01,
 * …RadonIntermediate.cu:13-67), for ij in [first, first+count).  Host output. */
int ecc_metric_debug_K01(ecc_metric* m, int64_t first, int64_t count, float* K01s);

/* ---- MetricDirect: consistency straight from the projection images ---------------------------- */
/* ref: class MetricDirect (LibEpipolarConsistency/EpipolarConsistencyDirect.h:28-60) and computeForImagePair
 * (EpipolarConsistencyDirect.cpp:67-219) -- no Radon intermediates; per pair 2 x n_lines line integrals through
 * the images (n_lines = twice the image diagonal unless dkappa is given), so it is ~1000x the work of
 * MetricRadonIntermediate per evaluation and meant for few views / images that change every iteration.
 * images: n x n_v x n_u float32.  on_device = 1: the metric BORROWS the device pointer (as the reference borrows
 * its textures); on_device = 0: it uploads and owns a copy.
 * use_fbcc != 0 (setFanBeamConsistency): the rectified fan-beam variant -- plain line integrals weighted by the
 * line perspectivity onto a virtual detector through the baseline (RectifiedFBCC.h, ...Direct.cpp:133-196)
 * instead of the derivative. */
typedef struct ecc_direct ecc_direct;
int ecc_direct_create(ecc_ctx* ctx, int n_images, const float* images, int on_device, int n_u, int n_v,
                      ecc_direct** out);
int ecc_direct_destroy(ecc_direct* d);
/* The metric keeps a transposed copy of the images (coalesced access for near-horizontal epipolar lines).  After
 * changing the pixels of borrowed device images call this before the next evaluation (asynchronous, a few
 * microseconds per image) -- the counterpart of re-binding the reference's textures. */
int ecc_direct_update_images(ecc_direct* d);
/* ref: MetricDirect::setProjectionMatrices; n x 12 float64 column-major. */
int ecc_direct_set_projections(ecc_direct* d, const double* Ps, int n_views);
/* ref: Metric::setObjectRadius / setEpipolarPlaneStep / MetricDirect::setFanBeamConsistency; 0 = automatic. */
int ecc_direct_set_params(ecc_direct* d, double object_radius_mm, double dkappa, int use_fbcc);
int ecc_direct_get_object_radius(const ecc_direct* d, double* radius_mm);
/* ref: double MetricDirect::evaluate(float* out) (.cpp:247-259): returns the SUM over all pairs (not the mean);
 * cost_nxn (host, nullable): entry (i,j), i<j at index i + j*n is written, the rest is preserved. */
int ecc_direct_evaluate(ecc_direct* d, float* cost_nxn, double* cost_sum);
/* ref: MetricDirect::evaluateForImagePair(i, j, redundant_samples0, redundant_samples1, kappas) (.cpp:261-272).
 * Host outputs, nullable, `capacity` entries each (lines01: 6 floats per kappa = the two epipolar lines in pixel
 * coordinates, Hessian normal form); ecc_direct_lines_bound gives a sufficient capacity.  A caller-provided
 * kappa grid (the reference accepts a non-empty `kappas` as input, .cpp:105-117) is not supported. */
int ecc_direct_lines_bound(const ecc_direct* d, int* capacity);
int ecc_direct_evaluate_for_image_pair(ecc_direct* d, int i, int j, int capacity, int* n_lines,
                                       float* redundant_samples0, float* redundant_samples1, float* kappas,
                                       float* lines01, double* metric);

/* The same with a caller-provided grid of epipolar-plane angles (the reference takes a non-empty `kappas` vector as
 * the grid, .cpp:105-117): n_kappas float32 angles on the host; outputs hold n_kappas entries each; the metric is
 * SUM (v0 - v1)^2 dkappa with the dkappa of ecc_direct_set_params (or the automatic one), as in the reference. */
int ecc_direct_evaluate_for_image_pair_kappas(ecc_direct* d, int i, int j, int n_kappas, const float* kappas_in,
                                              float* redundant_samples0, float* redundant_samples1, float* lines01,
                                              double* metric);

/* Index lists and pose batches for optimisers that move ONE view (or a few) between evaluations of images that change --
 * the setting MetricDirect is for (ref: Metric::evaluate(indices, out); Gui/SingleImageMotion.h builds the list
 * (input_index, i, input_index, i) of every other view i).  Only the pairs that contain a moved view change, and these calls
 * integrate only those.  DESIGN.md 4.27 says when this beats the Radon route (few poses x few reference views, or new pixels
 * per evaluation) and when it does not.
 *
 * ecc_direct_evaluate_pairs: idx4 holds n_pairs tuples (P0, P1, I0, I1) -- P0, P1 rows of the matrix table of
 * ecc_direct_set_projections (which may hold MORE matrices than there are images: that is how candidate matrices are passed),
 * I0, I1 image indices.  Entries are evaluated as written, in order, nothing reordered or merged.  pair_values[q] (host,
 * nullable) has THE BITS of the `metric` of ecc_direct_evaluate_for_image_pair on a metric whose matrices of views I0, I1 are
 * rows P0, P1; object radius, plane step and the FBCC switch are the metric's, as ecc_direct_evaluate applies them.
 * segment_offsets: n_segments + 1 non-decreasing offsets into the list, the first 0, the last n_pairs; segment_sums[s] (host,
 * nullable) is the float64 sum of pair_values[segment_offsets[s] .. segment_offsets[s + 1]) in the fixed order ecc_direct_evaluate
 * adds one batch in (1024 strided partials, a shuffle tree per wave, the 16 wave sums in order): the list of all pairs in get_ij
 * order as one segment has the bits of ecc_direct_evaluate's sum while that runs as one batch.  A null segment_offsets is one
 * segment holding the whole list.  Not both outputs null.  n_pairs == 0: ECC_OK, sums zeroed.
 *
 * ecc_direct_evaluate_pose_deltas: the packed lists of ecc_metric_evaluate_pose_deltas -- pose k = the SET matrices with the views
 * moved_views[moved_offsets[k] .. moved_offsets[k + 1]) (any order, each once) replaced by the blocks moved_Ps[12 q ..] of the same
 * entries q.  sums[k] = the sum (order as above) over the pairs i < j < n_images with at least one moved view, each once, in
 * ascending (i, j) order.  The pairs WITHOUT a moved view are a constant of the batch (the one the comment in the reference's
 * SingleImageMotion::evaluate speaks of): the caller owns it -- add ecc_direct_evaluate_pairs over those pairs, computed once,
 * where absolute values are wanted; differences between poses of the same moved views do not need it.  Under the automatic
 * object radius a pose that moves view 0 takes the radius of ITS view 0, as ecc_direct_set_projections + the single-pair call
 * would.  The set matrices are unchanged by the call.  pair_values / pair_idx4 (host, nullable): the terms and their (i, j, i, j)
 * tuples, pose after pose, ecc_direct_pose_pairs_bound entries (it is exact).  n_poses < 1: ECC_OK.
 *
 * Both refuse with ECC_ERR_INVALID_ARGUMENT and a text naming the entry: matrices not set, an index out of range, P0 == P1, a
 * view named twice in a pose, offsets that decrease or end elsewhere than the list, more than 2^20 pairs in a call.  (A caller's
 * kappa grid exists for the single-pair call only; these calls have no argument for one.)  They allocate nothing once their
 * scratch has grown, and wait for the device once, at the end.  The list runs in batches of at most 256 MB of line integrals;
 * ecc_debug_set_direct_batch lowers the batch to max_pairs entries (0: the library's bound) -- same bits, for tests. */
int ecc_direct_evaluate_pairs(ecc_direct* d, const int32_t* idx4, int64_t n_pairs, const int64_t* segment_offsets,
                              int n_segments, double* pair_values, double* segment_sums);
int ecc_direct_evaluate_pose_deltas(ecc_direct* d, int n_poses, const int32_t* moved_offsets, const int32_t* moved_views,
                                    const double* moved_Ps, double* sums, double* pair_values, int32_t* pair_idx4);
int ecc_direct_pose_pairs_bound(const ecc_direct* d, int n_poses, const int32_t* moved_offsets, int64_t* n_pairs);
int ecc_debug_set_direct_batch(ecc_direct* d, int64_t max_pairs);

/* Debug: what the pair-geometry kernel fitted for pairs ij in [first, first+count): per pair
 * ECC_POLY_RECORD_FLOATS floats = { degree evaluated (4, 6, 8, 10; 0 = exact path; + 0.5 when the fit's bound says that no sample
 * of the pair can reach a clamp of the pair kernel, which then runs its clamp-free loop), x_scale, fold0, fold1 (1 = folded on the +kappa side),
 * ca[0][0..DEG+2], ca[1][...], cd[0][0..DEG+1], cd[1][...] } with DEG = 10.  Host output. */
#define ECC_POLY_RECORD_FLOATS (4 + 2 * 13 + 2 * 12)
int ecc_metric_debug_polynomials(ecc_metric* m, int64_t first, int64_t count, float* out);

/* ---- helpers shared with callers ------------------------------------------------------------ */
/* ref: get_ij (EpipolarConsistencyCommon.hxx:52-79), closed form. */
void ecc_get_ij(int64_t ij, int n, int* i, int* j);
/* Host-side E1/E5 pieces, exported for tests and for callers that shard work themselves. */
void ecc_host_pinvT(const double* P, float* PinvT12);
void ecc_host_source_position(const double* P, float* C4);
double ecc_host_object_radius(const double* P, int n_u, int n_v);

/* ref: lineToSampleDtr (EpipolarConsistencyCommon.hxx:152-171), host: line (l0, l1, l2) relative to the image
 * centre -> line[0] = angle / Pi in [0, 1], line[1] = distance in [0, 1]; returns 1 when the (alpha + Pi, -t)
 * periodicity was used (the sample's sign flips for a derivative dtr).  fp32, atan2 correctly rounded. */
int ecc_host_line_to_sample_dtr(float* line3, float range_t);

/* ref: estimateAngularRange(join_pluecker(C0, C1), radius) (EpipolarConsistency.cpp:49-59): the kappa interval
 * of epipolar planes through the baseline of P0, P1 that touch a sphere of object_radius_mm about the origin. */
void ecc_host_angular_range(const double* P0, const double* P1, double object_radius_mm, double* kappa_first,
                            double* kappa_second);
/* ref: estimateAngularStep(P0, P1, n_u, n_v) (EpipolarConsistency.cpp:61-68). */
double ecc_host_angular_step(const double* P0, const double* P1, int n_u, int n_v);
/* ref: estimateIsoCenter(Ps) (EpipolarConsistency.cpp:8-33): least-squares intersection of the principal rays;
 * O receives 4 doubles (w = 1). */
void ecc_host_iso_center(const double* Ps, int n_views, double* O);

/* ---- single-process multi-GPU: a group of devices behind the same two calls ----------------------- */
/* The reference's callers are one process, one optimiser thread: ecc->setProjectionMatrices(Ps); ecc->evaluate()
 * (ref: Gui/SingleImageMotion.h:84-90, HeaderOnly/LibOpterix/WrapNLOpt.hxx:151-173).  A group gives such a caller
 * every GPU of the node: one context, stream and host thread per device, the Radon-intermediate stack replicated on
 * every device, the pair range cut into contiguous cost-balanced shards of the get_ij order (ecc_pair_shards_balanced,
 * fixed at the first evaluation; ecc_group_metric_rebalance recomputes them), the partial sums (8 bytes per device, pinned host memory) added on the host in rank order -- the same bits on every
 * call.  Nothing is exchanged between devices on the per-evaluation path.
 * devices: n_dev HIP device indices (NULL = 0 .. n_dev-1).  An index may repeat: ranks on the same device get their
 * own stream and thread and share the caller's slabs (rehearsal of the multi-rank path on one GPU). */
typedef struct ecc_group ecc_group;
typedef struct ecc_group_metric ecc_group_metric;
int ecc_group_create(int n_dev, const int* devices, ecc_group** out);
/* Destroy group metrics first, then dtrs made from the group's contexts, then the group. */
int ecc_group_destroy(ecc_group* g);
int ecc_group_size(const ecc_group* g);
/* The context of one rank (borrowed): e.g. to produce Radon intermediates on that device yourself. */
int ecc_group_ctx(ecc_group* g, int rank, ecc_ctx** ctx);
/* Data-parallel form of ecc_radon_compute_batch for host images: rank r computes the contiguous chunk of views
 * [r*ceil(n/G), ...) on its own device, all ranks concurrently.  out[k] lives on the device that computed it;
 * ecc_group_metric_create replicates. */
int ecc_group_radon_compute_batch(ecc_group* g, const float* images, int n, int n_u, int n_v, int n_alpha, int n_t,
                                  int filter, int post_process, ecc_dtr** out);
/* rank r of `world` evaluates pairs [first, first + count) of the get_ij order: first = r*n_pairs/world (integer). */
void ecc_pair_shard(int64_t n_pairs, int world, int rank, int64_t* first, int64_t* count);
/* Cost-balanced alternative: contiguous chunks of equal MODEL COST instead of equal count -- the pair kernel's time per
 * pair grows with the pair's kappa_max, and for a circular scan the expensive pairs sit in the first rows of the pair
 * triangle (equal-count shards of an 8-rank job measured 93 ... 68 us; model for balanced shards 77.5 us each; the fit is in
 * ecc_metric_api.hip).  bounds receives world + 1 pair indices, rank r evaluates [bounds[r], bounds[r+1]).  Host, float64, a
 * function of the matrices and the object radius only (every rank of a job computes the same bounds); ~0.3 ms for 400
 * views -- once per data set.  ecc_metric_balanced_shards uses the metric's current matrices and object radius. */
int ecc_pair_shards_balanced(const double* Ps, int n_views, double object_radius_mm, int world, int64_t* bounds);
int ecc_metric_balanced_shards(ecc_metric* m, int world, int64_t* bounds);

/* ref: MetricRadonIntermediate(Ps, dtrs) (...RadonIntermediate.cpp:53-66,87-106) over a group.  dtrs may live on
 * any devices; every rank gets a replica of the whole stack (device-to-device copies, peer access where available;
 * a rank whose device already holds all of them borrows them instead) and its own ecc_metric.  Same borrowing
 * contract as ecc_metric_create. */
int ecc_group_metric_create(ecc_group* g, int n_dtrs, ecc_dtr* const* dtrs, ecc_group_metric** out);
/* Debug / test hook: groups metrics created while it is on copy the Radon-intermediate stack on every rank even when it
 * is already on the rank's device (the code path of a real multi-GPU group on a one-GPU box; doubles the memory). */
int ecc_group_debug_force_replica(int on);
int ecc_group_metric_destroy(ecc_group_metric* gm);
/* ref: setProjectionMatrices.  The matrices are copied and handed to the devices together with the next
 * evaluation (one hand-off to the rank threads per optimiser step). */
int ecc_group_metric_set_projections(ecc_group_metric* gm, const double* Ps, int n_views);
int ecc_group_metric_set_params(ecc_group_metric* gm, double object_radius_mm, double dkappa, int use_corr);
int ecc_group_metric_set_incremental(ecc_group_metric* gm, int enable);  /* every rank keeps its own shard's values */
int ecc_group_metric_set_sampling(ecc_group_metric* gm, int mode);
int ecc_group_metric_get_object_radius(ecc_group_metric* gm, double* radius_mm);
/* ref: double MetricRadonIntermediate::evaluate(float* out): all pairs, sharded over the group; *mean = sum/n_pairs.
 * cost_nxn (host, nullable): entry (i,j), i<j at index i + j*n is written, the rest preserved.  With one rank the
 * result is bit-identical to ecc_metric_evaluate_all; with G ranks it is the rank-ordered float64 sum of G shard sums. */
int ecc_group_metric_evaluate_all(ecc_group_metric* gm, float* cost_nxn, double* mean);
/* n_poses INDEPENDENT all-pairs evaluations (Ps_batch: n_poses x n_views x 12 float64; means: n_poses results): a sweep
 * of poses (ref: Gui/Visualization.h:78-98 plotCostFunction; BASELINE config 5) or the probes of a finite-difference
 * gradient.  Pose p is evaluated entirely on rank p mod G -- no exchange, G times one device's throughput; every value
 * is bit-identical to ecc_metric_evaluate_all on one device.  The matrices of the last ecc_group_metric_set_projections
 * stay the group's current ones. */
int ecc_group_metric_evaluate_poses(ecc_group_metric* gm, int n_poses, const double* Ps_batch, int n_views, double* means);
/* Recompute the cost-balanced shard boundaries from the current matrices (they are otherwise fixed at the first
 * evaluation so that repeated evaluations add the same partial sums in the same order). */
int ecc_group_metric_rebalance(ecc_group_metric* gm);
/* The per-rank metric (borrowed): few-pair calls (index lists, evaluateForImagePair) go to rank 0's metric.  Pending
 * projection matrices are handed to the devices first. */
int ecc_group_metric_rank_metric(ecc_group_metric* gm, int rank, ecc_metric** m);

/* ---- multi-process sum of the partial results (one process per GPU, one node) ------------------ */
/* The path's only exchange step is the final sum over pairs (ref: ...RadonIntermediate.cpp:216-224; SURVEY.md 8e:
 * "one all-reduce of 2 doubles per evaluation -- latency-bound").  ecc_metric_evaluate_range leaves each rank's
 * partial sum on the host; ecc_exchange_sum adds the partial sums of all ranks through a POSIX shared-memory segment
 * (a cache line per rank, polled; ~1 us) in rank order, so every rank returns the same bits.  No device is
 * involved.  All ranks call ecc_exchange_sum the same number of times.
 * name: shm name starting with '/', the same on all ranks and unique per job; rank 0 creates the segment, the other
 * ranks wait for it.  A rank that does not show up makes the others fail with ECC_ERR_UNSUPPORTED after
 * ECC_EXCHANGE_TIMEOUT_S seconds (environment, default 60) instead of hanging; after such a failure the exchange
 * stays failed (every later ecc_exchange_sum returns the error at once) -- close it, do not retry.
 * SINGLE NODE ONLY: the segment lives in this node's /dev/shm, so rank / world are the node-local rank and the number
 * of ranks on this node (LOCAL_RANK / LOCAL_WORLD_SIZE under torchrun); a job that spans nodes adds the node sums
 * with a collective of its own (sharding.open_exchange refuses WORLD_SIZE != LOCAL_WORLD_SIZE). */
/* The same exchange as an RCCL all-reduce issued by the library (one process per GPU; the exchange north_star names).  Every rank
 * owns a communicator on its context's device: rank 0 makes the 128-byte id (ecc_comm_unique_id) and the job hands it to the
 * other ranks (bench.py: torch.distributed's broadcast); ecc_comm_create is RCCL's ncclCommInitRank -- a collective, it returns
 * when all `world` ranks have called it.  ecc_metric_evaluate_range_allreduce then does one rank's share of an evaluation in
 * ONE call: pair kernel over [first, first + count) -> float64 sum on the device -> ncclAllReduce over the ranks -> the scalar
 * published to pinned host memory -> poll; all on the context's stream, no host round trip in between.  *sum_all is the sum over
 * ALL ranks' pairs (the same bits on every rank); the mean is sum_all / (n (n - 1) / 2).  All ranks call it the same number of
 * times.  RCCL is loaded at run time (dlopen of librccl.so.1: the copy the process already has -- PyTorch's -- or ROCm's);
 * without it these calls fail with ECC_ERR_UNSUPPORTED and nothing else of the library is affected.
 * ecc_comm_available: ECC_OK when RCCL can be bound in this process -- no GPU call, no collective.  A job must AGREE on it
 * across its ranks (a MIN all-reduce of the answers) before any rank calls ecc_comm_create: a rank that cannot load RCCL
 * returns from ecc_comm_create at once, and the others would wait for it inside ncclCommInitRank for ever
 * (sharding.RcclComm does this when it is given an `agree` callable; bench.py passes one). */
typedef struct ecc_comm ecc_comm;
#define ECC_COMM_ID_BYTES 128
int ecc_comm_available(void);
int ecc_comm_unique_id(void* id128);
int ecc_comm_create(ecc_ctx* ctx, const void* id128, int rank, int world, ecc_comm** out);
int ecc_comm_destroy(ecc_comm* c);
int ecc_metric_evaluate_range_allreduce(ecc_metric* m, ecc_comm* comm, int64_t first, int64_t count, double* sum_all);
#define ECC_EXCHANGE_MAX_RANKS 64
typedef struct ecc_exchange ecc_exchange;
int ecc_exchange_open(const char* name, int rank, int world, ecc_exchange** out);
int ecc_exchange_sum(ecc_exchange* ex, double partial, double* total);
int ecc_exchange_close(ecc_exchange* ex);

/* Last kernel timings measured with HIP events on the context's stream (ms), for bench.py:
 * which = 0 pair kernel of the last evaluate, 1 Radon kernel of the last radon_compute[_batch],
 * 2 pre-processing kernel of the last ecc_preprocess.
 * Timing is off by default (no events recorded); enable with ecc_ctx_enable_timing. */
int ecc_ctx_enable_timing(ecc_ctx* ctx, int enable);
int ecc_ctx_last_kernel_ms(ecc_ctx* ctx, int which, float* ms);

/* ---- experiment hooks (not part of the drop-in surface) ------------------------------------------ */
/* What scripts/ uses for A/B measurements.  Explicit calls on a handle, so that nothing outside the caller's code can
 * change the arithmetic of an evaluation.
 * ecc_debug_set_poly_tolerance: the bound (in Radon bins) on what lowering a pair's polynomial degree may cost in
 *   ECC_SAMPLING_POLYNOMIAL (DESIGN.md 4.2 "economise"); default ECC_POLY_ECONOMISE_TOL_BINS.  Changes pair values at the
 *   1e-7 level; drops the kept records / values.
 * ecc_debug_set_small_eval_bound: max_pairs >= 0 lowers the size bound of the one-launch path (192 pairs; 0 = never taken,
 *   the path's other conditions still apply); -1 restores the default.  Same bits either way.
 * ecc_debug_set_result_polling: process-wide; 0 = synchronous calls wait for the stream instead of polling the pinned
 *   result slot.  Same bits.
 * ecc_debug_set_quad_copies: ecc_ctx_set_quad_copies(ctx, on ? ECC_QUAD_COPIES_ON : ECC_QUAD_COPIES_OFF), the experiments' old name.
 * ecc_debug_set_gradient_launch: 1 = ecc_metric_evaluate_gradient takes its own launch (path 2, csrc/small_poses_kernel.hip)
 *   where that launch applies; 0 (default) = always the pose batch.  Same bits either way.
 * ecc_debug_small_stamps: only in builds with -DECC_SMALL_STAMPS (returns ECC_ERR_INVALID_ARGUMENT otherwise). */
#define ECC_POLY_ECONOMISE_TOL_BINS 2e-8f
int ecc_debug_set_poly_tolerance(ecc_metric* m, float tol_bins);
int ecc_debug_set_small_eval_bound(ecc_metric* m, int64_t max_pairs);
int ecc_debug_set_result_polling(int on);
int ecc_debug_set_quad_copies(ecc_ctx* ctx, int on);
int ecc_debug_set_gradient_launch(ecc_metric* m, int on);
/* Row-quad copies.  Metrics created from ctx AFTERWARDS keep, beside the row-paired copy of every Radon intermediate (one
 * 16-byte footprint per sample), a second copy in which four consecutive angle rows share a 128-byte line (4x the slab's
 * memory: 3.9 GB for 400 views of 768 x 768 bins).  The pairs whose baseline passes through the object (kappa_max = pi/2,
 * 3.5 % of a short scan's pairs, a fifth of its evaluation time) cross the Radon intermediates diagonally, a new angle row
 * every sample or two; the exact part of their sampling reads the row-quad copies: +2 % evaluations/s on the 400-view
 * benchmark, bit-identical values (tests/test_gpu_sampling_modes.py).  ECC_QUAD_COPIES_AUTO (default): decided ONCE per metric
 * by its first all-pairs evaluation (or shard of one) over at least 32 768 pairs, from the matrices it runs with -- built when at least 2 % of their pairs have
 * kappa_max > pi/4 (a 200-degree short scan: 3.5 %; a 90-degree scan: none, and no memory is spent) and all copies together
 * take at most a quarter of the device memory free at that time (an allocation that fails after all means "none"); that
 * evaluation is ~1.5 ms longer.  _OFF: never; _ON: always, at ecc_metric_create (offsets permitting; an allocation failure is
 * the metric's failure).
 * MEMORY a metric owns per Radon intermediate of n_alpha x n_t bins, pitch = roundup(n_t + 2, 32) floats (ecc_metric_device_bytes
 * reports the totals; the Radon intermediates themselves, (n_alpha + 2) x pitch x 4 bytes each, belong to their ecc_dtr):
 *   row-paired copy (always):  (n_alpha + 1) x pitch x 8 bytes                   768 x 768 bins: 4.92 MB, 400 views 1.97 GB
 *   row-quad copy (see above): ceil((n_alpha + 1) / 4) x pitch x 64 bytes        768 x 768 bins: 9.88 MB, 400 views 3.95 GB
 * i.e. 2x and 4x the slab (2.46 MB): a 400-view metric holds 5.9 GB beside the 0.99 GB of the stack itself -- for 0.300 -> 0.294 ms
 * per evaluation in the row-quad case.  A process that keeps many metrics alive on one device should create them from a context
 * with ECC_QUAD_COPIES_OFF (same bits, -2 %). */
#define ECC_QUAD_COPIES_AUTO (-1)
#define ECC_QUAD_COPIES_OFF 0
#define ECC_QUAD_COPIES_ON 1
int ecc_ctx_set_quad_copies(ecc_ctx* ctx, int mode);
/* Device memory the metric owns right now, in bytes (any pointer may be null): the row-paired copies, the row-quad copies
 * (0 when they were not built), everything else (geometry, per-pair records of 296 bytes, pair values, cost image, index
 * lists, the pose batch's scratch -- grown on demand, kept until the metric is destroyed). */
int ecc_metric_device_bytes(const ecc_metric* m, int64_t* paired_bytes, int64_t* quad_bytes, int64_t* other_bytes);
int ecc_debug_small_stamps(unsigned long long* out, int n_blocks);
/* Host clock (seconds, std::chrono::steady_clock) at fixed points of the metric's last ecc_metric_set_projections and last
 * synchronous all-pairs / range evaluation -- where the host's share of a step goes (scripts/step_fixed_cost.py):
 * [0] set_projections entered, [1] returned; [2] evaluate entered, [3] change detection done (first launch next),
 * [4] first pair-kernel launch returned, [5] refit / list launches queued, [6] sum launch returned, [7] result seen,
 * [8] step queued: every launch of the evaluation but the sum is in its stream ([6] - [8] is then the host-side join of the
 * two-stream form -- ecc_metric_evaluate_all and ecc_metric_evaluate_range wait for the moved views' list launch on the host and
 * queue the sum behind the all-pairs launch with no cross-stream wait -- plus the sum's launch call).  out: ECC_STEP_STAMPS doubles. */
#define ECC_STEP_STAMPS 9
int ecc_debug_step_stamps(const ecc_metric* m, double* out);

#ifdef __cplusplus
}
#endif
#endif /* ECC_HIP_H */
