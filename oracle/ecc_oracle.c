/*
 * ecc_oracle.c -- CPU ORACLE for the epipolar-consistency hot path.  TEST INFRASTRUCTURE ONLY.
 *
 * This file is a plain-C restatement of the reference's algorithm (aaichert/EpipolarConsistency,
 * lib 1.2.2) for the Radon-intermediate + all-pairs ECC path.  It is the checker the HIP path is
 * compared against.  Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
 * load it; the product library (epipolarconsistency_amd/csrc) never links, includes or calls it.
 *
 * PARITY STATUS (see DESIGN.md "Oracle"):
 *   - E1/E2 geometry (pseudo-inverse, source position, computeK01, lineToSampleDtr, get_ij) is
 *     PINNED: tests compare it against the reference's own host-compilable headers built into
 *     oracle/_ref/libecc_ref.so (oracle/Makefile) and against the known-answer scalars of the
 *     example pair recorded in SURVEY.md 8c.
 *   - R1 (radonDerivative) and E3 (kernelEpipolarCosistency) exist in the reference only as CUDA
 *     kernels that cannot be compiled or run here and the reference ships no tests or golden
 *     vectors for them: for those two bodies PARITY IS UNPINNED -- this restatement follows the
 *     reference source line by line and is the normative definition.
 *
 * Arithmetic convention: every float expression is the reference's C++ source expression
 * evaluated in IEEE-754 binary32, left to right, WITHOUT fused contraction (build with
 * -ffp-contract=off; see oracle/Makefile).  Elementary functions (sinf, cosf, atan2f, asinf) are
 * taken CORRECTLY ROUNDED (evaluated in binary64 and rounded once) so that the oracle does not
 * depend on one libm: glibc 2.35's atan2f is biased by 0.135 ulp towards zero, which alone moves
 * the 400-view metric by 2e-5 (measured, DESIGN.md "Oracle"); CUDA's atan2f/__sincosf, which the
 * reference actually runs, are different again.  eccor_set_variant(2) switches to the platform's
 * float libm -- that is the variant pinned bit-for-bit against the reference headers.  CUDA's hardware bilinear filter (9-bit weights)
 * is replaced by the exact fp32 rule of SURVEY.md 8c ("normative sampling rule").
 * Per-pair sums (atomicAdd in arbitrary order in the reference) are accumulated in binary64
 * and rounded once to float.
 *
 * All "ref:" citations are relative to /root/reference/code/.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define ECCOR_API __attribute__((visibility("default")))

/* 0 normative (correctly rounded elementary functions); 1 sensitivity probe: line -> (angle,
 * distance) mapping in binary64; 2 platform float libm (pinned against oracle/_ref). */
static int g_variant = 0;
ECCOR_API void eccor_set_variant(int v) { g_variant = v; }

static int g_use_corr = 0;
ECCOR_API void eccor_set_use_corr(int v) { g_use_corr = v; }

static float or_sinf(float x) { return g_variant == 2 ? sinf(x) : (float)sin((double)x); }
static float or_cosf(float x) { return g_variant == 2 ? cosf(x) : (float)cos((double)x); }
static float or_atan2f(float y, float x) { return g_variant == 2 ? atan2f(y, x) : (float)atan2((double)y, (double)x); }
static float or_logf(float x) { return g_variant == 2 ? logf(x) : (float)log((double)x); }
static float or_asinf(float x) { return g_variant == 2 ? asinf(x) : (float)asin((double)x); }

/* ------------------------------------------------------------------------------------------ */
/* E1: per-view pre-compute (double in, float out)                                             */
/* ------------------------------------------------------------------------------------------ */

/* Householder QR of a square N x N column-major matrix, A := R, Q explicit.
 * ref: LibUtilsCuda/culaut/xgeinv.hxx:40-105 (xsqqr).  Quirk kept: `scale` is a running
 * maximum over all columns processed so far (initialised once, :47).  abs() is taken as the
 * floating-point absolute value (what nvcc/MSVC resolve it to). */
static void or_sqqr(int N, double *A, double *Q)
{
    double d[4], c[4];
    double scale = 0.0, sigma = 0.0, sum = 0.0, tau = 0.0;
    int i, j, k;
    for (k = 0; k < N; k++) {
        for (i = k; i < N; i++)
            if (scale < fabs(A[i + N * k])) scale = fabs(A[i + N * k]);
        if (scale == 0.0) {
            c[k] = d[k] = 0.0;
        } else {
            for (i = k; i < N; i++) A[i + N * k] /= scale;
            for (sum = 0.0, i = k; i < N; i++) sum += A[i + N * k] * A[i + N * k];
            sigma = A[k + N * k] > 0.0 ? sqrt(sum) : -sqrt(sum);
            A[k + N * k] += sigma;
            c[k] = sigma * A[k + N * k];
            d[k] = -scale * sigma;
            for (j = k + 1; j < N; j++) {
                for (sum = 0.0, i = k; i < N; i++) sum += A[i + N * k] * A[i + N * j];
                tau = sum / c[k];
                for (i = k; i < N; i++) A[i + N * j] -= tau * A[i + N * k];
            }
        }
    }
    d[N - 1] *= -1;
    if (Q) {
        for (i = 0; i < N; i++) {
            for (j = 0; j < N; j++) Q[i + N * j] = 0.0;
            Q[i + N * i] = 1.0;
        }
        for (k = 0; k < N - 1; k++)
            if (c[k] != 0.0)
                for (j = 0; j < N; j++) {
                    sum = 0.0;
                    for (i = k; i < N; i++) sum += A[i + N * k] * Q[j + N * i];
                    sum /= c[k];
                    for (i = k; i < N; i++) Q[j + N * i] -= sum * A[i + N * k];
                }
    }
    for (i = 0; i < N; i++)
        for (j = 0; j < N; j++) {
            if (i == j) A[i + N * i] = d[i];
            else if (i < j) { /* keep */ }
            else A[i + N * j] = 0;
        }
}

/* ref: xgeinv.hxx:108-119 (xutsolve) */
static void or_utsolve(int N, const double *A, const double *b, double *x)
{
    int i, j;
    x[N - 1] = b[N - 1] / A[(N - 1) * N + (N - 1)];
    for (i = N - 2; i >= 0; i--) {
        x[i] = b[i];
        for (j = i + 1; j < N; j++) x[i] -= A[j * N + i] * x[j];
        x[i] = x[i] / A[i * N + i];
    }
}

/* ref: xgeinv.hxx:137-168 (xsqqrsolve + xgeinv), N = 3 */
static void or_geinv3(const double *Ain, double *Ainv)
{
    double Q[9], R[9], unit[3] = {0, 0, 0}, Qtb[3];
    int i, j, c;
    for (i = 0; i < 9; i++) R[i] = Ain[i];
    or_sqqr(3, R, Q);
    for (c = 0; c < 3; c++) {
        unit[c] = 1;
        for (j = 0; j < 3; j++) {
            double sum = 0;
            for (i = 0; i < 3; i++) sum += unit[i] * Q[i + 3 * j];
            Qtb[j] = sum;
        }
        or_utsolve(3, R, Qtb, Ainv + c * 3);
        unit[c] = 0;
    }
}

/* (P^+)^T as 3x4 column-major float.  P is 3x4 column-major double.
 * ref: LibUtilsCuda/culaut/xprojectionmatrix.hxx:20-52 */
ECCOR_API void eccor_pinvT(const double *P, float *PinvT)
{
    double PPT[9], PPTinv[9];
    int r;
    PPT[0] = P[0] * P[0] + P[3] * P[3] + P[6] * P[6] + P[9] * P[9];
    PPT[1] = P[0] * P[1] + P[3] * P[4] + P[6] * P[7] + P[9] * P[10];
    PPT[2] = P[0] * P[2] + P[3] * P[5] + P[6] * P[8] + P[9] * P[11];
    PPT[4] = P[1] * P[1] + P[4] * P[4] + P[7] * P[7] + P[10] * P[10];
    PPT[5] = P[1] * P[2] + P[4] * P[5] + P[7] * P[8] + P[10] * P[11];
    PPT[8] = P[2] * P[2] + P[5] * P[5] + P[8] * P[8] + P[11] * P[11];
    PPT[3] = PPT[1]; PPT[6] = PPT[2]; PPT[7] = PPT[5];
    or_geinv3(PPT, PPTinv);
    for (r = 0; r < 4; r++) {
        const double *p = P + 3 * r;
        PinvT[3 * r + 0] = (float)(p[0] * PPTinv[0] + p[1] * PPTinv[1] + p[2] * PPTinv[2]);
        PinvT[3 * r + 1] = (float)(p[0] * PPTinv[3] + p[1] * PPTinv[4] + p[2] * PPTinv[5]);
        PinvT[3 * r + 2] = (float)(p[0] * PPTinv[6] + p[1] * PPTinv[7] + p[2] * PPTinv[8]);
    }
}

/* Homogeneous source position (w = 1) via QR of (P^T | 0).
 * ref: LibUtilsCuda/culaut/xprojectionmatrix.hxx:93-105 */
ECCOR_API void eccor_source_position(const double *P, float *C)
{
    double Q[16], R[16];
    int i, j;
    for (i = 0; i < 3; i++)
        for (j = 0; j < 4; j++) R[j + 4 * i] = P[i + 3 * j];
    for (j = 0; j < 4; j++) R[j + 4 * 3] = 0;
    or_sqqr(4, R, Q);
    for (i = 0; i < 4; i++) C[i] = (float)(Q[i + 4 * 3] / Q[3 + 4 * 3]);
}

/* ------------------------------------------------------------------------------------------ */
/* E5: default object radius                                                                   */
/* ------------------------------------------------------------------------------------------ */

static void or_cross(const double *a, const double *b, double *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
static double or_det3(const double *a, const double *b, const double *c) /* columns */
{
    return a[0] * (b[1] * c[2] - b[2] * c[1]) - b[0] * (a[1] * c[2] - a[2] * c[1]) +
           c[0] * (a[1] * b[2] - a[2] * b[1]);
}

/* Camera centre, normalised to w = 1 when |w| > 1e-12.  The reference takes the SVD null space
 * (Eigen, absent here); any f64 null space agrees to ~1e-13 -- here: signed 3x3 minors.
 * ref: LibProjectiveGeometry/ProjectionMatrix.cpp:70-76 */
ECCOR_API void eccor_camera_center(const double *P, double *C)
{
    const double *c0 = P, *c1 = P + 3, *c2 = P + 6, *c3 = P + 9;
    C[0] = or_det3(c1, c2, c3);
    C[1] = -or_det3(c0, c2, c3);
    C[2] = or_det3(c0, c1, c3);
    C[3] = -or_det3(c0, c1, c2);
    if (C[3] < -1e-12 || C[3] > 1e-12) {
        C[0] /= C[3]; C[1] /= C[3]; C[2] /= C[3]; C[3] = 1.0;
    }
}

/* ref: LibProjectiveGeometry/ProjectionMatrix.cpp:104-112 (getCameraFocalLengthPx) */
ECCOR_API void eccor_focal_length_px(const double *P, double *fu, double *fv)
{
    double m1[3] = {P[0], P[3], P[6]}, m2[3] = {P[1], P[4], P[7]}, m3[3] = {P[2], P[5], P[8]};
    double U[3], V[3], t[3], n;
    or_cross(m3, m2, U); n = sqrt(U[0] * U[0] + U[1] * U[1] + U[2] * U[2]);
    U[0] /= n; U[1] /= n; U[2] /= n;
    or_cross(m3, m1, V); n = sqrt(V[0] * V[0] + V[1] * V[1] + V[2] * V[2]);
    V[0] /= n; V[1] /= n; V[2] /= n;
    or_cross(V, m3, t); *fu = m1[0] * t[0] + m1[1] * t[1] + m1[2] * t[2];
    or_cross(U, m3, t); *fv = m2[0] * t[0] + m2[1] * t[1] + m2[2] * t[2];
}

/* ref: LibEpipolarConsistency/EpipolarConsistency.cpp:35-47 (estimateObjectRadius) */
ECCOR_API double eccor_object_radius(const double *P, int n_u, int n_v)
{
    double fu, fv, C[4], fov, a, b, sid;
    eccor_focal_length_px(P, &fu, &fv);
    a = fabs(atan(0.5 * n_u / fu));
    b = fabs(atan(0.5 * n_v / fv));
    fov = a > b ? a : b;
    eccor_camera_center(P, C);
    sid = sqrt(C[0] * C[0] + C[1] * C[1] + C[2] * C[2]);
    return sin(fov) * sid;
}

/* ------------------------------------------------------------------------------------------ */
/* E2: pair geometry                                                                           */
/* ------------------------------------------------------------------------------------------ */

/* ref: LibEpipolarConsistency/EpipolarConsistencyCommon.hxx:52-79 (get_ij) */
ECCOR_API void eccor_get_ij(int ij, int n, int *pi, int *pj)
{
    int i = 0, k = ij + 1;
    while (k > n - i - 1) { i++; k -= (n - i); }
    *pi = i; *pj = k + i;
}

/* ref: EpipolarConsistencyCommon.hxx:82-90 (shiftOriginAndNormlaize) */
static void or_shift_origin_and_normalize(float x, float y, float *Ki)
{
    float s0;
    int i;
    Ki[2] += x * Ki[0] + y * Ki[1];
    Ki[5] += x * Ki[3] + y * Ki[4];
    s0 = sqrtf(Ki[0] * Ki[0] + Ki[1] * Ki[1]);
    for (i = 0; i < 6; i++) Ki[i] /= s0;
}

/* C(3x2) = A(3x4) * B(4x2), column-major, sum starts at 0 and adds s = 0..3 in order.
 * ref: EpipolarConsistencyCommon.hxx:39-50 (xgemm<float,3,4,2>) */
static void or_gemm_3_4_2(const float *A, const float *B, float *C)
{
    int i, j, s;
    for (i = 0; i < 3; i++)
        for (j = 0; j < 2; j++) {
            float sum = 0;
            for (s = 0; s < 4; s++) sum += A[s * 3 + i] * B[j * 4 + s];
            C[j * 3 + i] = sum;
        }
}

/* ref: EpipolarConsistencyCommon.hxx:93-149 (computeK01).  K0[6] baseline distance,
 * K0[7] view angle, K1[6] dkappa, K1[7] kappa_max. */
ECCOR_API void eccor_computeK01(float n_x2, float n_y2, const float *C0, const float *C1,
                                const float *P0invT, const float *P1invT, float object_radius_mm,
                                float num_samples, float dkappa, float *K0, float *K1)
{
    int i;
    if (C0 == C1) {
        for (i = 0; i < 8; i++) K0[i] = 0;
        for (i = 0; i < 8; i++) K1[i] = 0;
        return;
    }
    {
        float B01 = C0[0] * C1[1] - C0[1] * C1[0];
        float B02 = C0[0] * C1[2] - C0[2] * C1[0];
        float B03 = C0[0] * C1[3] - C0[3] * C1[0];
        float B12 = C0[1] * C1[2] - C0[2] * C1[1];
        float B13 = C0[1] * C1[3] - C0[3] * C1[1];
        float B23 = C0[2] * C1[3] - C0[3] * C1[2];
        const float s2 = sqrtf(B12 * B12 + B02 * B02 + B01 * B01);
        const float s3 = sqrtf(B03 * B03 + B13 * B13 + B23 * B23);
        float K[8];
        const float Pi = 3.14159265359f;
        K[0] = +B12 / s2; K[1] = -B02 / s2; K[2] = +B01 / s2; K[3] = 0;
        K[4] = (-B01 * B13 - B02 * B23) / (s2 * s3);
        K[5] = (+B01 * B03 - B12 * B23) / (s2 * s3);
        K[6] = (+B02 * B03 + B12 * B13) / (s2 * s3);
        K[7] = -s2 / s3;
        or_gemm_3_4_2(P0invT, K, K0);
        or_gemm_3_4_2(P1invT, K, K1);
        or_shift_origin_and_normalize(n_x2, n_y2, K0);
        or_shift_origin_and_normalize(n_x2, n_y2, K1);
        K0[6] = s2 / s3;
        K0[7] = -2.0f * or_atan2f(-0.5f * s3, s2 / s3);
        if (K0[6] <= object_radius_mm) K1[7] = 0.5f * Pi;
        else K1[7] = or_asinf(object_radius_mm / K0[6]);
        if (dkappa <= 0.f) K1[6] = 2.f * K1[7] / num_samples;
        else K1[6] = dkappa;
    }
}

/* ref: EpipolarConsistencyCommon.hxx:152-171 (lineToSampleDtr).  line[0] <- angle/Pi in [0,1],
 * line[1] <- distance in [0,1]; returns 1 when the (alpha+Pi, -t) periodicity was used. */
ECCOR_API int eccor_line_to_sample_dtr(float *line, float range_t)
{
    const float Pi = 3.14159265359f;
    float length = sqrtf(line[0] * line[0] + line[1] * line[1]);
    line[0] = or_atan2f(line[1], line[0]) / Pi;
    if (line[0] < 0) line[0] += 2;
    line[1] = -(line[2] / length) / range_t + 0.5f;
    if (line[0] > 1) {
        line[0] = line[0] - 1.f;
        line[1] = 1.f - line[1];
        return 1;
    }
    return 0;
}

/* ------------------------------------------------------------------------------------------ */
/* Normative sampling rule replacing CUDA texture hardware                      */
/* ------------------------------------------------------------------------------------------ */

static inline int or_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* Un-normalised coordinates, linear filter, clamp addressing; img is row-major, x fastest.
 * Models cudaTextureObject_t built at ref: LibUtilsCuda/CudaBindlessTexture.cpp:25-39. */
ECCOR_API float eccor_tex2d(const float *img, int W, int H, float x, float y)
{
    float xb = x - 0.5f, yb = y - 0.5f;
    float fi = floorf(xb), fj = floorf(yb);
    float fx = xb - fi, fy = yb - fj;
    int i = (int)fi, j = (int)fj;
    int i0 = or_clampi(i, 0, W - 1), i1 = or_clampi(i + 1, 0, W - 1);
    int j0 = or_clampi(j, 0, H - 1), j1 = or_clampi(j + 1, 0, H - 1);
    float T00 = img[(size_t)j0 * W + i0], T10 = img[(size_t)j0 * W + i1];
    float T01 = img[(size_t)j1 * W + i0], T11 = img[(size_t)j1 * W + i1];
    float r0 = (1.f - fx) * T00 + fx * T10;
    float r1 = (1.f - fx) * T01 + fx * T11;
    return (1.f - fy) * r0 + fy * r1;
}

/* The CONTRACTED statement of the same rule (eccor_set_radon_contract(1), Radon intermediate only): what a compiler
 * that fuses a*b+c does with the lerp written as T00 + fx*(T10 - T00) -- three rounded differences and three fmaf,
 * 6 operations instead of 11.  The reference's GPU build never executes the unfused form either: it interpolates in
 * texture hardware (ref: LibUtilsCuda/CudaBindlessTexture.cpp:25-39) and nvcc contracts the position arithmetic
 * (ref: RadonIntermediate.cu:118-123).  The product's ECC_RADON_FMA mode is held to THIS function bit for bit. */
static float or_tex2d_contract(const float *img, int W, int H, float x, float y)
{
    float xb = x - 0.5f, yb = y - 0.5f;
    float fi = floorf(xb), fj = floorf(yb);
    float fx = xb - fi, fy = yb - fj;
    int i = (int)fi, j = (int)fj;
    int i0 = or_clampi(i, 0, W - 1), i1 = or_clampi(i + 1, 0, W - 1);
    int j0 = or_clampi(j, 0, H - 1), j1 = or_clampi(j + 1, 0, H - 1);
    float T00 = img[(size_t)j0 * W + i0], T10 = img[(size_t)j0 * W + i1];
    float T01 = img[(size_t)j1 * W + i0], T11 = img[(size_t)j1 * W + i1];
    float r0 = fmaf(fx, T10 - T00, T00);
    float r1 = fmaf(fx, T11 - T01, T01);
    return fmaf(fy, r1 - r0, r0);
}

/* Normalised coordinates (dtr textures, ref: RadonIntermediate.cpp:192). */
ECCOR_API float eccor_tex2d_norm(const float *img, int W, int H, float s, float t)
{
    return eccor_tex2d(img, W, H, s * (float)W, t * (float)H);
}

/* ------------------------------------------------------------------------------------------ */
/* R1: Radon intermediate                                                                      */
/* ------------------------------------------------------------------------------------------ */

/* ref: RadonIntermediate.cu:18-29 (sort4) */
static void or_sort4(float *v)
{
    int i, j;
    for (j = 0; j < 3; j++)
        for (i = 0; i < 3; i++)
            if (v[i] > v[i + 1]) { float tmp = v[i]; v[i] = v[i + 1]; v[i + 1] = tmp; }
}

/* 0: every expression of the sampling loop unfused (normative, the CPU reading of the source); 1: the loop body
 * contracted -- positions fmaf(t, d, o), texel rule or_tex2d_contract.  The per-bin set-up (line, clipping, bounds
 * test) and the accumulation are the same rounded operations in both. */
static int g_radon_contract = 0;
ECCOR_API void eccor_set_radon_contract(int on) { g_radon_contract = on ? 1 : 0; }
ECCOR_API int eccor_get_radon_contract(void) { return g_radon_contract; }

/* One Radon bin.  filter: 0 Derivative, 1 Ramp (line integral; the filter follows in eccor_radon), 2 None; post: 0/1/2.
 * ref: RadonIntermediate.cu:32-143 (radonDerivative<derivative>); *fetches += #bilinear fetches. */
static float or_radon_bin(const float *img, int W, int H, int n_alpha, int n_t, int ix, int iy,
                          int filter, int post, long long *fetches)
{
    const float Pi = 3.14159265359f; /* __constant__ float Pi, RadonIntermediate.cu:8 */
    const float n_u = (float)W, n_v = (float)H;
    float l[3], o[2], d[2], ts[4], t, t_max, sum = 0;
    const float step = .66f;
    long long nf = 0;
    float x_rel = (ix / (float)n_alpha - 0.5f);
    float y_rel = (iy / (float)n_t - 0.5f);
    float diag = sqrtf(n_u * n_u + n_v * n_v);
    float alpha = x_rel * Pi;
    float tau = y_rel * diag;
    l[0] = -or_sinf(alpha);
    l[1] = or_cosf(alpha);
    l[2] = -tau;
    l[2] += -0.5f * n_u * l[0] - 0.5f * n_v * l[1];
    o[0] = -l[2] * l[0];
    o[1] = -l[2] * l[1];
    d[0] = l[1];
    d[1] = -l[0];
    ts[0] = (1.f - o[0]) / d[0];
    ts[1] = (n_u - 1.f - o[0]) / d[0];
    ts[2] = (1.f - o[1]) / d[1];
    ts[3] = (n_v - 1.f - o[1]) / d[1];
    if (d[0] * d[0] < 1e-12f) ts[0] = -(ts[1] = 1e10f);
    if (d[1] * d[1] < 1e-12f) ts[2] = -(ts[3] = 1e10f);
    or_sort4(ts);
    t = ts[1];
    t_max = ts[2];
    {
        float u = o[0] + t * d[0], v = o[1] + t * d[1];
        int inb = (u <= n_u && v <= n_v && u >= 0 && v >= 0);
        if (!inb || t_max <= t) return 0.f;
    }
    o[0] += .5f;
    o[1] += .5f;
    if (filter != 0) {
        if (g_radon_contract)
            for (; t <= t_max; t += step) {
                sum += or_tex2d_contract(img, W, H, fmaf(t, d[0], o[0]), fmaf(t, d[1], o[1]));
                nf++;
            }
        else
            for (; t <= t_max; t += step) {
                sum += eccor_tex2d(img, W, H, o[0] + t * d[0], o[1] + t * d[1]);
                nf++;
            }
        if (fetches) *fetches += nf;
        return sum * step;
    } else {
        float sumo = 0, result;
        o[0] -= .5f * d[1];
        o[1] += .5f * d[0];
        if (g_radon_contract)
            for (; t <= t_max; t += step) {
                const float x = fmaf(t, d[0], o[0]), y = fmaf(t, d[1], o[1]);
                sum += or_tex2d_contract(img, W, H, x, y);
                sumo += or_tex2d_contract(img, W, H, x + d[1], y - d[0]);
                nf += 2;
            }
        else
            for (; t <= t_max; t += step) {
                sum += eccor_tex2d(img, W, H, o[0] + t * d[0], o[1] + t * d[1]);
                sumo += eccor_tex2d(img, W, H, o[0] + t * d[0] + d[1], o[1] + t * d[1] - d[0]);
                nf += 2;
            }
        if (fetches) *fetches += nf;
        result = (sum - sumo) * step;
        if (post == 1) return result < 0 ? -sqrtf(-result) : sqrtf(result);
        if (post == 2) return result < 0 ? -or_logf(-result + 1) : or_logf(result + 1);  /* correctly rounded, like every elementary function here */
        return result;
    }
}

/* Ramp filter along t (Filter::Ramp), ref: RadonIntermediate.cu:173-237 (apply1DRampFilter).
 * The reference runs, per angle column, an unnormalised real-to-complex FFT of the n_t values, multiplies
 * bin k = 0..n_t/2 by the FLOAT factor k*scale, scale = -0.5f/(n_t*n_theta), n_theta = n_t/2+1
 * (ramp_filter1D, :173-183, :219), and transforms back with an unnormalised complex-to-real FFT whose
 * input is Hermitian-extended (bins k > n_t/2 carry the weight of n_t-k).  cuFFT's float round-off is
 * not reproducible on a CPU; the oracle evaluates the SAME linear map exactly: a circular convolution
 *   y[t] = sum_s x[s] * h[(t-s) mod n_t],   h[m] = sum_{k=0}^{n_t-1} w_k cos(2 pi k m / n_t),
 *   w_k = (float)min(k, n_t-k) * scale  (the float factor of ramp_filter1D),
 * with h and the sum over s = 0..n_t-1 (in this order, unfused) in binary64, rounded once to float.
 * h2 receives 2*n_t doubles, h2[m] = h[m mod n_t] (so that h2[t - s + n_t] needs no modulo). */
ECCOR_API void eccor_ramp_kernel(int n_t, double *h2)
{
    const int n_theta = n_t / 2 + 1;
    const float scale = -0.5f / (n_t * n_theta);
    double *c = (double *)malloc(sizeof(double) * (size_t)n_t);
    int m, r;
    for (r = 0; r < n_t; r++) c[r] = cos(6.283185307179586476925286766559 * (double)r / (double)n_t);
#pragma omp parallel for schedule(static)
    for (m = 0; m < n_t; m++) {
        double acc = 0.0;
        int k;
        for (k = 0; k < n_t; k++) {
            int kk = k <= n_t - k ? k : n_t - k;
            float w = kk * scale;
            acc += (double)w * c[((long long)k * m) % n_t]; /* argument reduced exactly */
        }
        h2[m] = acc;
        h2[m + n_t] = acc;
    }
    free(c);
}

/* In place on an n_t x n_alpha, alpha-fast array. */
ECCOR_API void eccor_ramp_filter(float *dtr, int n_alpha, int n_t)
{
    double *h2 = (double *)malloc(sizeof(double) * 2 * (size_t)n_t);
    int ix;
    eccor_ramp_kernel(n_t, h2);
#pragma omp parallel for schedule(dynamic, 4)
    for (ix = 0; ix < n_alpha; ix++) {
        float *x = (float *)malloc(sizeof(float) * (size_t)n_t);
        int t, s;
        for (t = 0; t < n_t; t++) x[t] = dtr[(size_t)t * n_alpha + ix];
        for (t = 0; t < n_t; t++) {
            double acc = 0.0;
            for (s = 0; s < n_t; s++) acc += (double)x[s] * h2[t - s + n_t];
            dtr[(size_t)t * n_alpha + ix] = (float)acc;
        }
        free(x);
    }
    free(h2);
}

/* Full Radon intermediate, output n_t rows x n_alpha columns, alpha fastest (idx = iy*n_alpha+ix).
 * ref: RadonIntermediate.cu:149-170 (computeDerivLineIntegrals); filter == 1 appends the ramp filter. */
ECCOR_API void eccor_radon(const float *img, int n_u, int n_v, int n_alpha, int n_t, int filter,
                           int post, float *out, long long *fetches)
{
    long long total = 0;
    int iy;
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : total)
    for (iy = 0; iy < n_t; iy++) {
        int ix;
        long long f = 0;
        for (ix = 0; ix < n_alpha; ix++)
            out[(size_t)iy * n_alpha + ix] =
                or_radon_bin(img, n_u, n_v, n_alpha, n_t, ix, iy, filter, post, &f);
        total += f;
    }
    if (fetches) *fetches = total;
    if (filter == 1) eccor_ramp_filter(out, n_alpha, n_t);
}

/* Selected bins only (bins[k] = iy*n_alpha+ix): spot checks at full problem sizes. */
ECCOR_API void eccor_radon_bins(const float *img, int n_u, int n_v, int n_alpha, int n_t,
                                int filter, int post, const int *bins, int n_bins, float *out)
{
    int k;
#pragma omp parallel for schedule(dynamic, 16)
    for (k = 0; k < n_bins; k++)
        out[k] = or_radon_bin(img, n_u, n_v, n_alpha, n_t, bins[k] % n_alpha, bins[k] / n_alpha,
                              filter, post, 0);
}

/* ------------------------------------------------------------------------------------------ */
/* E3/E4: pair consistency                                                                     */
/* ------------------------------------------------------------------------------------------ */

/* Sensitivity probe (NOT the normative path): variant 1 evaluates the line -> (angle, distance)
 * mapping in binary64 and rounds the two texture coordinates to float.  Tests use the distance
 * between variant 0 and variant 1 as the fp32 "noise floor" of the pair values. */
/* probe bits for variant 1: re-introduce single fp32 roundings of the normative path one at a time
 * (1 float constant Pi, 2 float sin/cos, 4 float line, 8 float length, 16 float atan2/Pi,
 * 32 float angle after +2, 64 float distance); 127 ~ the normative path. */
static int g_probe = 0;
ECCOR_API void eccor_set_probe(int bits) { g_probe = bits; }

/* eccor_tex2d's rule (clamp addressing, linear filter) at a binary64 position with binary64 weights (probe bit 128). */
static double or_tex2d_f64(const float *img, int W, int H, double x, double y)
{
    double xb = x - 0.5, yb = y - 0.5;
    double fi = floor(xb), fj = floor(yb);
    double fx = xb - fi, fy = yb - fj;
    int i = (int)fi, j = (int)fj;
    int i0 = or_clampi(i, 0, W - 1), i1 = or_clampi(i + 1, 0, W - 1);
    int j0 = or_clampi(j, 0, H - 1), j1 = or_clampi(j + 1, 0, H - 1);
    double T00 = img[(size_t)j0 * W + i0], T10 = img[(size_t)j0 * W + i1];
    double T01 = img[(size_t)j1 * W + i0], T11 = img[(size_t)j1 * W + i1];
    double r0 = (1.0 - fx) * T00 + fx * T10;
    double r1 = (1.0 - fx) * T01 + fx * T11;
    return (1.0 - fy) * r0 + fy * r1;
}

static float or_redundancy_f64(const float *K, const float *dtr, int n_alpha, int n_t,
                               float range_t, double x0, double x1, int is_derivative)
{
    const double Pi = (g_probe & 1) ? (double)3.14159265359f : 3.14159265358979323846;
    double l0, l1, l2, len, a, d;
    int moved = 0;
    if (g_probe & 2) { x0 = (float)x0; x1 = (float)x1; }
    l0 = K[0] * x0 + K[3] * x1; l1 = K[1] * x0 + K[4] * x1; l2 = K[2] * x0 + K[5] * x1;
    if (g_probe & 4) {
        l0 = (float)((float)(K[0] * (float)x0) + (float)(K[3] * (float)x1));
        l1 = (float)((float)(K[1] * (float)x0) + (float)(K[4] * (float)x1));
        l2 = (float)((float)(K[2] * (float)x0) + (float)(K[5] * (float)x1));
    }
    len = sqrt(l0 * l0 + l1 * l1);
    if (g_probe & 8) len = (float)len;
    a = atan2(l1, l0) / Pi;
    if (g_probe & 16) a = (float)((float)atan2(l1, l0) / (float)Pi);
    if (a < 0) a += 2;
    if (g_probe & 32) a = (float)a;
    d = -(l2 / len) / (double)range_t + 0.5;
    if (g_probe & 64) d = (float)((float)(-(float)(l2 / len) / range_t) + 0.5f);
    if (a > 1) { a -= 1; d = 1 - d; moved = 1; }
    if (g_probe & 128) { /* texel position and bilinear weights in binary64 too: no rounding of the sample coordinates */
        double v = or_tex2d_f64(dtr, n_alpha, n_t, a * n_alpha, d * n_t);
        return (float)(is_derivative && moved ? -v : v);
    }
    if (is_derivative && moved) return -eccor_tex2d_norm(dtr, n_alpha, n_t, (float)a, (float)d);
    return +eccor_tex2d_norm(dtr, n_alpha, n_t, (float)a, (float)d);
}

/* ref: EpipolarConsistencyRadonIntermediate.cu:71-84 (getRedundancy) */
static float or_redundancy(const float *K, const float *dtr, int n_alpha, int n_t, float range_t,
                           float x0, float x1, int is_derivative)
{
    float line[3];
    int moved;
    line[0] = K[0] * x0 + K[3] * x1;
    line[1] = K[1] * x0 + K[4] * x1;
    line[2] = K[2] * x0 + K[5] * x1;
    moved = eccor_line_to_sample_dtr(line, range_t);
    if (is_derivative && moved) return -eccor_tex2d_norm(dtr, n_alpha, n_t, line[0], line[1]);
    return +eccor_tex2d_norm(dtr, n_alpha, n_t, line[0], line[1]);
}

typedef struct {
    int n_u, n_v, n_alpha, n_t;
    float step_alpha, step_t;
    float object_radius_mm, dkappa;
    int is_derivative;
    int use_corr;
} eccor_params;

/* One pair: K01 (launcher arguments of ref: ...RadonIntermediate.cu:320-338) then the kappa loop
 * of ref: ...RadonIntermediate.cu:257-270 + :87-113.  Returns the pair value (float), i.e.
 * sum_k ((vp^2+vm^2)*K0[6])*dkappa; the sum itself is carried in double (atomics in the ref). */
static float or_pair(const eccor_params *p, const float *C0, const float *C1, const float *P0invT,
                     const float *P1invT, const float *dtr0, const float *dtr1, float *K01_out,
                     long long *n_kappa)
{
    float K0[8], K1[8];
    float image_diagonal = p->n_t * p->step_t * 2.f;
    float range_t = p->n_t * p->step_t;
    float dkappa, kappa_max;
    double acc = 0.0;
    double mom[5] = {0, 0, 0, 0, 0}; /* x, y, xx, yy, xy (use_corr) */
    int k, k_limit;
    const float Pi = 3.14159265359f;
    eccor_computeK01(p->n_u * 0.5f, p->n_v * 0.5f, C0, C1, P0invT, P1invT, p->object_radius_mm,
                     image_diagonal, p->dkappa, K0, K1);
    if (K01_out) { memcpy(K01_out, K0, 32); memcpy(K01_out + 8, K1, 32); }
    dkappa = K1[6];
    kappa_max = K1[7];
    /* launch bound on idx_y: grid.y*256 threads, ref: ...RadonIntermediate.cu:348-358 */
    {
        int max_num_samples = p->dkappa <= 0.0f ? (int)image_diagonal : (int)(Pi * 0.5f / p->dkappa);
        k_limit = ((max_num_samples + 255) / 256) * 256;
    }
    for (k = 0; k < k_limit; k++) {
        float kappa = dkappa * 0.5f + dkappa * k;
        float x0, x1, vp, vm, consistency;
        if (kappa >= kappa_max) break;
        if (g_variant == 1) {
            double c = cos((double)kappa), s = sin((double)kappa);
            vp = or_redundancy_f64(K0, dtr0, p->n_alpha, p->n_t, range_t, c, s, p->is_derivative) -
                 or_redundancy_f64(K1, dtr1, p->n_alpha, p->n_t, range_t, c, s, p->is_derivative);
            vm = or_redundancy_f64(K0, dtr0, p->n_alpha, p->n_t, range_t, -c, s, p->is_derivative) -
                 or_redundancy_f64(K1, dtr1, p->n_alpha, p->n_t, range_t, -c, s, p->is_derivative);
            consistency = (vp * vp + vm * vm) * K0[6];
            acc += (double)(consistency * dkappa);
            continue;
        }
        x0 = or_cosf(kappa);
        x1 = or_sinf(kappa);
        if (p->use_corr) {
            /* ref: ...RadonIntermediate.cu:116-149 (consistencyForPlusMinusKappa_XCORR); the "1/n" the
             * launcher passes is kappa_max/kappa (:211,274) -- kept as written. */
            float one_over_n = kappa_max / kappa;
            float xp = or_redundancy(K0, dtr0, p->n_alpha, p->n_t, range_t, x0, x1, p->is_derivative);
            float yp = or_redundancy(K1, dtr1, p->n_alpha, p->n_t, range_t, x0, x1, p->is_derivative);
            float xm, ym;
            x0 *= -1;
            xm = or_redundancy(K0, dtr0, p->n_alpha, p->n_t, range_t, x0, x1, p->is_derivative);
            ym = or_redundancy(K1, dtr1, p->n_alpha, p->n_t, range_t, x0, x1, p->is_derivative);
            mom[0] += (double)(one_over_n * (xp + xm));
            mom[1] += (double)(one_over_n * (yp + ym));
            mom[2] += (double)(one_over_n * (xp * xp + xm * xm));
            mom[3] += (double)(one_over_n * (yp * yp + ym * ym));
            mom[4] += (double)(one_over_n * (xp * yp + xm * ym));
            continue;
        }
        vp = or_redundancy(K0, dtr0, p->n_alpha, p->n_t, range_t, x0, x1, p->is_derivative) -
             or_redundancy(K1, dtr1, p->n_alpha, p->n_t, range_t, x0, x1, p->is_derivative);
        x0 *= -1;
        vm = or_redundancy(K0, dtr0, p->n_alpha, p->n_t, range_t, x0, x1, p->is_derivative) -
             or_redundancy(K1, dtr1, p->n_alpha, p->n_t, range_t, x0, x1, p->is_derivative);
        consistency = (vp * vp + vm * vm) * K0[6];
        acc += (double)(consistency * dkappa);
    }
    if (n_kappa) *n_kappa += k;
    if (p->use_corr) {
        /* host epilogue, ref: ...RadonIntermediate.cpp:127-131 (cc, un-centred) and :199-210: cost = (1 - cc) * 1 */
        float xx = (float)mom[2], yy = (float)mom[3], xy = (float)mom[4];
        float corr = (float)((double)xy / (sqrt((double)xx) * sqrt((double)yy)));
        return (1.0f - corr) * 1.0f;
    }
    return (float)acc;
}

/* All-pairs evaluate.  Ps: n x 12 doubles (3x4 column-major each).  dtrs: n pointers to n_t x n_alpha
 * floats (alpha fastest).  cost: n x n floats in/out (index i + j*n, only i<j written) or NULL.
 * pair_values: n(n-1)/2 floats in get_ij order or NULL.  K01s: 16 floats/pair or NULL.
 * Returns sum/n_pairs in double.
 * ref: EpipolarConsistencyRadonIntermediate.cpp:134-163 (pre-compute) + :166-225 (evaluate). */
ECCOR_API double eccor_evaluate_all(int n, const double *Ps, const float *const *dtrs, int n_u,
                                    int n_v, int n_alpha, int n_t, double object_radius_mm,
                                    double dkappa, int is_derivative, float *cost,
                                    float *pair_values, float *K01s, long long *n_kappa_total)
{
    eccor_params p;
    float *Cs = (float *)malloc(sizeof(float) * 4 * n);
    float *PinvTs = (float *)malloc(sizeof(float) * 12 * n);
    int n_pairs = n * (n - 1) / 2, ij, v;
    float *vals = (float *)malloc(sizeof(float) * (n_pairs > 0 ? n_pairs : 1));
    double diagonal = sqrt((double)n_v * n_v + (double)n_u * n_u);
    double sum = 0;
    long long nk = 0;
    p.n_u = n_u; p.n_v = n_v; p.n_alpha = n_alpha; p.n_t = n_t;
    p.step_alpha = (float)(3.1415926535897931 / n_alpha); /* ref: RadonIntermediate.cpp:204-206 */
    p.step_t = (float)(diagonal / n_t);
    p.object_radius_mm = (float)(object_radius_mm > 0 ? object_radius_mm
                                                       : eccor_object_radius(Ps, n_u, n_v));
    p.dkappa = (float)dkappa;
    p.is_derivative = is_derivative;
    p.use_corr = g_use_corr;
    for (v = 0; v < n; v++) {
        eccor_pinvT(Ps + 12 * v, PinvTs + 12 * v);
        eccor_source_position(Ps + 12 * v, Cs + 4 * v);
    }
#pragma omp parallel for schedule(dynamic, 8) reduction(+ : nk)
    for (ij = 0; ij < n_pairs; ij++) {
        int i, j;
        long long c = 0;
        eccor_get_ij(ij, n, &i, &j);
        vals[ij] = or_pair(&p, Cs + 4 * i, Cs + 4 * j, PinvTs + 12 * i, PinvTs + 12 * j, dtrs[i],
                           dtrs[j], K01s ? K01s + 16 * ij : 0, &c);
        nk += c;
    }
    for (ij = 0; ij < n_pairs; ij++) {
        int i, j;
        eccor_get_ij(ij, n, &i, &j);
        if (cost) cost[i + j * n] = vals[ij];
        if (pair_values) pair_values[ij] = vals[ij];
        sum += vals[ij]; /* weights are all 1, ref: ...RadonIntermediate.cu:254, .cpp:216-224 */
    }
    if (n_kappa_total) *n_kappa_total = nk;
    free(Cs); free(PinvTs); free(vals);
    return sum / n_pairs;
}

/* Index-list evaluate: idx4[4p..4p+3] = (P0, P1, dtr0, dtr1); out: n_pairs floats.
 * ref: EpipolarConsistencyRadonIntermediate.cpp:267-322 and .cu:152-211 (without the
 * idx_x>num_pairs off-by-one, SURVEY.md E3'). */
ECCOR_API double eccor_evaluate_pairs(int n_P, const double *Ps, int n_dtr, const float *const *dtrs,
                                      int n_u, int n_v, int n_alpha, int n_t,
                                      double object_radius_mm, double dkappa, int is_derivative,
                                      const int *idx4, int n_pairs, float *out, float *K01s)
{
    eccor_params p;
    float *Cs = (float *)malloc(sizeof(float) * 4 * n_P);
    float *PinvTs = (float *)malloc(sizeof(float) * 12 * n_P);
    double diagonal = sqrt((double)n_v * n_v + (double)n_u * n_u);
    double sum = 0;
    int q, v;
    (void)n_dtr;
    p.n_u = n_u; p.n_v = n_v; p.n_alpha = n_alpha; p.n_t = n_t;
    p.step_alpha = (float)(3.1415926535897931 / n_alpha);
    p.step_t = (float)(diagonal / n_t);
    p.object_radius_mm = (float)(object_radius_mm > 0 ? object_radius_mm
                                                       : eccor_object_radius(Ps, n_u, n_v));
    p.dkappa = (float)dkappa;
    p.is_derivative = is_derivative;
    p.use_corr = g_use_corr;
    for (v = 0; v < n_P; v++) {
        eccor_pinvT(Ps + 12 * v, PinvTs + 12 * v);
        eccor_source_position(Ps + 12 * v, Cs + 4 * v);
    }
#pragma omp parallel for schedule(dynamic, 8)
    for (q = 0; q < n_pairs; q++) {
        const int *t = idx4 + 4 * q;
        out[q] = or_pair(&p, Cs + 4 * t[0], Cs + 4 * t[1], PinvTs + 12 * t[0], PinvTs + 12 * t[1],
                         dtrs[t[2]], dtrs[t[3]], K01s ? K01s + 16 * q : 0, 0);
    }
    for (q = 0; q < n_pairs; q++) sum += out[q];
    free(Cs); free(PinvTs);
    return sum / n_pairs;
}

/* E7: evaluateForImagePair -- the redundant signals of one pair over kappa in (-kappa_max, kappa_max).
 * ref: EpipolarConsistencyRadonIntermediate.cpp:324-393 and RadonIntermediate.h:86-108 (sample, tex2D).
 * The reference's host code is "visualization only" and visibly unfinished; NOT a parity
 * target against the reference.  Kept as written: K01 with num_samples = sqrtf(n_u*n_u+n_v*n_v) (:349), the
 * fp32-accumulated kappa loop (:367), cosf/sinf and the line products (:370-375).  Evident intent
 * implemented instead of the code as written: (1) the fold's sign for derivative dtrs is applied (sample()'s
 * flip branch is unreachable after lineToSampleDtr has folded the angle); (2) sampling uses the metric's own
 * texel rule (normalised coordinates) rather than the host image's (n-1)*s scaling;
 * (3) ecc ACCUMULATES (v0-v1)^2*dkappa (the reference assigns, :389).  P^+T and C come from E1 (QR), the
 * reference takes them from Eigen's SVD here -- same quantities to ~1e-13.
 * out arrays hold `capacity` entries each (radon0/radon1: 2 per sample = (a, d)); returns the number of
 * samples (which may exceed capacity: then only the first `capacity` are stored). */
ECCOR_API int eccor_evaluate_for_image_pair(const double *P0, const double *P1, const float *dtr0,
                                            const float *dtr1, int n_u, int n_v, int n_alpha, int n_t,
                                            double object_radius_mm, double dkappa_user,
                                            int derivative0, int derivative1, int capacity, float *rs0,
                                            float *rs1, float *kappas, float *radon0, float *radon1,
                                            float *K01, double *ecc_out)
{
    float C0[4], C1[4], P0invT[12], P1invT[12], K0[8], K1[8];
    double diagonal = sqrt((double)n_v * n_v + (double)n_u * n_u);
    float step_t = (float)(diagonal / n_t);
    float range_t = step_t * n_t; /* ref: RadonIntermediate.h:90 */
    float dkappa, kappa_max, kappa;
    double ecc = 0;
    int n = 0;
    eccor_pinvT(P0, P0invT);
    eccor_pinvT(P1, P1invT);
    eccor_source_position(P0, C0);
    eccor_source_position(P1, C1);
    eccor_computeK01(n_u * 0.5f, n_v * 0.5f, C0, C1, P0invT, P1invT, (float)object_radius_mm,
                     sqrtf((float)(n_u * n_u + n_v * n_v)), (float)dkappa_user, K0, K1);
    if (K01) { memcpy(K01, K0, 32); memcpy(K01 + 8, K1, 32); }
    dkappa = K1[6];
    kappa_max = K1[7];
    if (!(dkappa > 0.f)) { if (ecc_out) *ecc_out = 0; return 0; }
    for (kappa = -kappa_max + 0.5f * dkappa; kappa < kappa_max; kappa += dkappa) {
        float x0 = or_cosf(kappa), x1 = or_sinf(kappa);
        float line0[3] = {K0[0] * x0 + K0[3] * x1, K0[1] * x0 + K0[4] * x1, K0[2] * x0 + K0[5] * x1};
        float line1[3] = {K1[0] * x0 + K1[3] * x1, K1[1] * x0 + K1[4] * x1, K1[2] * x0 + K1[5] * x1};
        int m0 = eccor_line_to_sample_dtr(line0, range_t);
        int m1 = eccor_line_to_sample_dtr(line1, range_t);
        float v0 = eccor_tex2d_norm(dtr0, n_alpha, n_t, line0[0], line0[1]);
        float v1 = eccor_tex2d_norm(dtr1, n_alpha, n_t, line1[0], line1[1]);
        if (derivative0 && m0) v0 = -v0;
        if (derivative1 && m1) v1 = -v1;
        if (n < capacity) {
            if (rs0) rs0[n] = v0;
            if (rs1) rs1[n] = v1;
            if (kappas) kappas[n] = kappa;
            if (radon0) { radon0[2 * n] = line0[0]; radon0[2 * n + 1] = line0[1]; }
            if (radon1) { radon1[2 * n] = line1[0]; radon1[2 * n + 1] = line1[1]; }
        }
        ecc += (double)((v0 - v1) * (v0 - v1) * dkappa);
        n++;
    }
    if (ecc_out) *ecc_out = ecc;
    return n;
}

/* ------------------------------------------------------------------------------------------ */
/* (f-1) projection pre-processing, the step in front of R1                                    */
/* ------------------------------------------------------------------------------------------ */

/* ref: LibEpipolarConsistency/Gui/PreProccess.cpp:8-13 (weighting, the double overload used there) */
static double or_weighting_d(double x)
{
    double xx;
    if (x < -1.0 || x > 1.0) return 0;
    xx = x * x;
    return 1.0 - 2 * xx + xx * xx;
}

typedef struct {
    int process;              /* 0: skip process(), only the cosine weighting (if P given) */
    int normalize;            /* Intensity/Normalize */
    double bias, scale;       /* Intensity/Bias, Intensity/Scale */
    int apply_log;            /* Intensity/Apply Minus Logarithm */
    double gaussian_sigma;    /* Lowpass Filter/Gaussian Sigma (default 1.84) */
    int half_kernel_width;    /* Lowpass Filter/Half Kernel Width (default 5) */
    int flip_u, flip_v;
    int zero[4];              /* left, right, bottom, top (default 1) */
    int feather[4];           /* default 16 */
    int n_blanks;
    const int *blanks;        /* n_blanks x 4: x0, y0, x1, y1 */
} eccor_preprocess_params;

/* ref: HeaderOnly/NRRD/nrrd_lowpass.hxx:19-33 (gaussianKernel): 2k+1 taps, normalised over all of them */
ECCOR_API void eccor_gaussian_kernel(double sigma, int k, double *kernel)
{
    int n = 2 * k + 1, x, i;
    double sum = 0;
    for (x = -k; x <= k; x++) {
        double v = exp(-0.5 * pow(x / sigma, 2));
        sum += v;
        kernel[x + k] = v;
    }
    for (i = 0; i < n; i++) kernel[i] /= sum;
}

/* In place on one n_u x n_v float image (row-major, u fastest).
 * ref: Gui/PreProccess.cpp:57-144 (PreProccess::process), step by step in its order:
 * intensity (normalise / scale+bias / -log / zero negatives, NaN, Inf), border zero + feather on the four
 * sides (left and top start at b = 0 and zero b <= zero[.], right and bottom start at b = 1 -- kept as
 * written), blanks, flips, Gaussian low-pass (HeaderOnly/NRRD/nrrd_lowpass.hxx:45-79: both passes run
 * o = -k .. k-1, i.e. the last tap is dropped, both use kernelx, sums in double, clamp addressing).
 * std::log on a float is logf; taken correctly rounded like every elementary function of this oracle.
 * Not replicated: out-of-bounds writes of the reference when a border band or a blank exceeds the image
 * (bands and blanks are clipped to the image; the blank's y < img.size(0) bound, :117, is kept AND clipped). */
ECCOR_API void eccor_preprocess(float *img, int n_u, int n_v, const eccor_preprocess_params *p)
{
    const int l = n_u * n_v;
    int i, x, y, b, q;
    if (!p->process) return;
    {
        float scale = (float)p->scale, bias = (float)p->bias;
        if (p->normalize) {
            float max = img[0];
            for (i = 0; i < l; i++)
                if (img[i] > max) max = img[i];
            bias = 0;
            scale = (float)p->scale / max;
        }
        for (i = 0; i < l; i++) {
            float pixel = img[i] * scale + bias;
            if (p->apply_log) pixel = (float)-(g_variant == 2 ? logf(pixel) : (float)log((double)pixel));
            if (pixel < 0 || isnan(pixel) || isinf(pixel)) pixel = 0;
            img[i] = pixel;
        }
    }
    /* left */
    for (y = 0; y < n_v; y++)
        for (b = 0; b < p->zero[0] + p->feather[0] && b < n_u; b++)
            img[b + (size_t)y * n_u] *= b <= p->zero[0] ? 0 : (float)or_weighting_d(1 - (float)(b - p->zero[0]) / p->feather[0]);
    /* right */
    for (y = 0; y < n_v; y++)
        for (b = 1; b <= p->zero[1] + p->feather[1] && b <= n_u; b++)
            img[(n_u - b) + (size_t)y * n_u] *= b <= p->zero[1] ? 0 : (float)or_weighting_d(1 - (float)(b - p->zero[1]) / p->feather[1]);
    /* bottom */
    for (b = 1; b <= p->zero[2] + p->feather[2] && b <= n_v; b++)
        for (x = 0; x < n_u; x++)
            img[x + (size_t)(n_v - b) * n_u] *= b <= p->zero[2] ? 0 : (float)or_weighting_d(1 - (float)(b - p->zero[2]) / p->feather[2]);
    /* top */
    for (b = 0; b < p->zero[3] + p->feather[3] && b < n_v; b++)
        for (x = 0; x < n_u; x++)
            img[x + (size_t)b * n_u] *= b <= p->zero[3] ? 0 : (float)or_weighting_d(1 - (float)(b - p->zero[3]) / p->feather[3]);
    /* blanks */
    for (q = 0; q < p->n_blanks; q++) {
        const int *bl = p->blanks + 4 * q;
        for (y = bl[1] > 0 ? bl[1] : 0; y < n_u && y < bl[3] && y < n_v; y++)
            for (x = bl[0] > 0 ? bl[0] : 0; x < n_u && x < bl[2]; x++) img[x + (size_t)y * n_u] = 0;
    }
    /* flips */
    if (p->flip_u)
        for (y = 0; y < n_v; y++)
            for (x = 0; x < n_u / 2; x++) {
                float t = img[x + (size_t)y * n_u];
                img[x + (size_t)y * n_u] = img[(n_u - 1 - x) + (size_t)y * n_u];
                img[(n_u - 1 - x) + (size_t)y * n_u] = t;
            }
    if (p->flip_v)
        for (y = 0; y < n_v / 2; y++)
            for (x = 0; x < n_u; x++) {
                float t = img[x + (size_t)y * n_u];
                img[x + (size_t)y * n_u] = img[x + (size_t)(n_v - 1 - y) * n_u];
                img[x + (size_t)(n_v - 1 - y) * n_u] = t;
            }
    /* low-pass */
    if (p->gaussian_sigma > 0 && p->half_kernel_width > 1) {
        const int k = p->half_kernel_width;
        double *kernel = (double *)malloc(sizeof(double) * (2 * k + 1));
        float *work = (float *)malloc(sizeof(float) * (size_t)l);
        int o;
        eccor_gaussian_kernel(p->gaussian_sigma, k, kernel);
        for (y = 0; y < n_v; y++)
            for (x = 0; x < n_u; x++) {
                double sum = 0;
                for (o = -k; o < k; o++) {
                    int xo = x + o < 0 ? 0 : (x + o > n_u - 1 ? n_u - 1 : x + o);
                    sum += img[xo + (size_t)y * n_u] * kernel[o + k];
                }
                work[x + (size_t)y * n_u] = (float)sum;
            }
        for (x = 0; x < n_u; x++)
            for (y = 0; y < n_v; y++) {
                double sum = 0;
                for (o = -k; o < k; o++) {
                    int yo = y + o < 0 ? 0 : (y + o > n_v - 1 ? n_v - 1 : y + o);
                    sum += work[x + (size_t)yo * n_u] * kernel[o + k];
                }
                img[x + (size_t)y * n_u] = (float)sum;
            }
        free(kernel);
        free(work);
    }
}

/* Intrinsics used by the cosine weighting: K(0,0), K(0,2), K(1,2) of P = K [R|t] with K upper triangular,
 * positive diagonal, K(2,2) = 1.  The reference gets K from Eigen's Householder QR of the row-permuted
 * transpose (ref: LibProjectiveGeometry/ProjectionMatrix.cpp:25-58, projectionMatrixDecomposition); Eigen is
 * absent here, this is the same RQ factorisation by Gram-Schmidt on the rows of M = P(:,0:3) in binary64
 * (agrees to ~1e-13 relative, then cast to float as the caller does, Gui/PreProccess.cpp:153-155). */
ECCOR_API void eccor_intrinsics(const double *P, float *sdd_px, float *ppu, float *ppv)
{
    double m1[3] = {P[0], P[3], P[6]}, m2[3] = {P[1], P[4], P[7]}, m3[3] = {P[2], P[5], P[8]};
    double K22 = sqrt(m3[0] * m3[0] + m3[1] * m3[1] + m3[2] * m3[2]);
    double r3[3] = {m3[0] / K22, m3[1] / K22, m3[2] / K22};
    double K12 = m2[0] * r3[0] + m2[1] * r3[1] + m2[2] * r3[2];
    double v[3] = {m2[0] - K12 * r3[0], m2[1] - K12 * r3[1], m2[2] - K12 * r3[2]};
    double K11 = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    double r2[3] = {v[0] / K11, v[1] / K11, v[2] / K11};
    double K02 = m1[0] * r3[0] + m1[1] * r3[1] + m1[2] * r3[2];
    double K01 = m1[0] * r2[0] + m1[1] * r2[1] + m1[2] * r2[2];
    double w[3] = {m1[0] - K02 * r3[0] - K01 * r2[0], m1[1] - K02 * r3[1] - K01 * r2[1],
                   m1[2] - K02 * r3[2] - K01 * r2[2]};
    double K00 = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    *sdd_px = (float)(K00 / K22);
    *ppu = (float)(K02 / K22);
    *ppv = (float)(K12 / K22);
}

/* ref: Gui/PreProccess.cpp:146-166 (apply_weight_cos_principal_ray); P all zero -> no-op (:149) */
ECCOR_API void eccor_cos_weight(float *img, int n_u, int n_v, const double *P)
{
    float sdd_px, ppu, ppv;
    int u, v, z = 1;
    for (u = 0; u < 12; u++) z = z && P[u] == 0;
    if (z) return;
    eccor_intrinsics(P, &sdd_px, &ppu, &ppv);
    for (v = 0; v < n_v; v++)
        for (u = 0; u < n_u; u++) {
            float pou = (float)u - ppu;
            float pov = (float)v - ppv;
            float cos_weight = sdd_px / sqrtf(pou * pou + pov * pov + sdd_px * sdd_px);
            img[u + (size_t)v * n_u] *= cos_weight;
        }
}

/* ------------------------------------------------------------------------------------------ */
/* (f-4) MetricDirect: ECC straight from the projection images, no Radon intermediate          */
/* ------------------------------------------------------------------------------------------ */

/* (P^+)^T E for a plane E (4-vector): the epipolar line of plane E in the image of P.  The reference forms
 * P^+ with Eigen's JacobiSVD (ref: LibProjectiveGeometry/SingularValueDecomposition.cpp:10-25; absent here).
 * Same quantity by modified Gram-Schmidt on the rows of P in binary64: P = L Q (L lower triangular, Q with
 * orthonormal rows), (P^+)^T = L^-T Q.  Works on P itself (condition ~3e5), not on P P^T (~1e11). */
typedef struct { double Q[3][4]; double L[3][3]; } or_rowqr;

static void or_row_qr(const double *P, or_rowqr *f)
{
    int i, j, k;
    double v[4];
    memset(f, 0, sizeof(*f));
    for (i = 0; i < 3; i++) {
        for (k = 0; k < 4; k++) v[k] = P[i + 3 * k];
        for (j = 0; j < i; j++) {
            double dot = 0;
            for (k = 0; k < 4; k++) dot += v[k] * f->Q[j][k];
            f->L[i][j] = dot;
            for (k = 0; k < 4; k++) v[k] -= dot * f->Q[j][k];
        }
        {
            double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
            f->L[i][i] = n;
            for (k = 0; k < 4; k++) f->Q[i][k] = v[k] / n;
        }
    }
}

static void or_plane_to_line(const or_rowqr *f, const double *E, double *l)
{
    double y[3];
    int i, k;
    for (i = 0; i < 3; i++) {
        y[i] = 0;
        for (k = 0; k < 4; k++) y[i] += f->Q[i][k] * E[k];
    }
    /* solve L^T l = y (upper triangular) */
    l[2] = y[2] / f->L[2][2];
    l[1] = (y[1] - f->L[2][1] * l[2]) / f->L[1][1];
    l[0] = (y[0] - f->L[1][0] * l[1] - f->L[2][0] * l[2]) / f->L[0][0];
}

/* ref: LibProjectiveGeometry/ProjectiveGeometry.hxx:188-200 (join of two points) */
static void or_join_points(const double *A, const double *B, double *L)
{
    L[0] = A[0] * B[1] - A[1] * B[0];
    L[1] = A[0] * B[2] - A[2] * B[0];
    L[2] = A[0] * B[3] - A[3] * B[0];
    L[3] = A[1] * B[2] - A[2] * B[1];
    L[4] = A[1] * B[3] - A[3] * B[1];
    L[5] = A[2] * B[3] - A[3] * B[2];
}

/* ref: ProjectiveGeometry.hxx:216-224 (join of a line and a point -> plane) */
static void or_join_line_point(const double *L, const double *X, double *E)
{
    E[0] = +X[1] * L[5] - X[2] * L[4] + X[3] * L[3];
    E[1] = -X[0] * L[5] + X[2] * L[2] - X[3] * L[1];
    E[2] = +X[0] * L[4] - X[1] * L[2] + X[3] * L[0];
    E[3] = -X[0] * L[3] + X[1] * L[1] - X[2] * L[0];
}

/* One epipolar line integral (derivative form) straight from an image.
 * ref: LibEpipolarConsistency/EpipolarConsistencyDirect.cu:31-125 (kernel_computeLineIntegrals, fbcc_d == 0):
 * lines in pixel coordinates (origin at pixel (0,0)), Hessian normal form; clipping as in R1; step 0.4 px; two
 * parallel lines half a pixel to either side of the line, each sample multiplied by the step before it is added.
 * Deviation: the reference's launcher passes n_u for BOTH image sizes (:137); the evident
 * intent (n_u, n_v) is implemented -- identical for square images. */
static float or_direct_line_integral(const float *img, int n_u, int n_v, const float *line)
{
    float l[3] = {line[0], line[1], line[2]};
    float o[2] = {-l[2] * l[0], -l[2] * l[1]};
    float d[2] = {l[1], -l[0]};
    float ts[4], t_min, t_max, t, sump = 0, summ = 0;
    const float step = 0.4f;
    ts[0] = (1 - o[0]) / d[0];
    ts[1] = (n_u - 1 - o[0]) / d[0];
    ts[2] = (1 - o[1]) / d[1];
    ts[3] = (n_v - 1 - o[1]) / d[1];
    if (d[0] * d[0] < 1e-12) ts[0] = -(ts[1] = 1e10f);
    if (d[1] * d[1] < 1e-12) ts[2] = -(ts[3] = 1e10f);
    or_sort4(ts);
    t_min = ts[1];
    t_max = ts[2];
    {
        float u = o[0] + t_min * d[0], v = o[1] + t_min * d[1];
        if (!(u <= n_u && v <= n_v && u >= 0 && v >= 0)) return 0.f;
    }
    o[0] += .5f;
    o[1] += .5f;
    l[0] *= 0.5f;
    l[1] *= 0.5f;
    for (t = t_min; t <= t_max; t += step) {
        float u = o[0] + t * d[0];
        float v = o[1] + t * d[1];
        sump += eccor_tex2d(img, n_u, n_v, u + l[0], v + l[1]) * step;
        summ += eccor_tex2d(img, n_u, n_v, u - l[0], v - l[1]) * step;
    }
    return sump - summ;
}

/* ---- rectified fan-beam consistency (FBCC) weighting, ref: RectifiedFBCC.h + ...Direct.cpp:133-196 ---- */

/* ref: RectifiedFBCC.h:18-90 (LinePerspectivity: a, b, c, d as floats; transform, derivative in float) */
typedef struct { float a, b, c, d; float t_prime_ak, d_l_kappa_C_sq; } or_fbcc_info;

static float or_phi_transform(const or_fbcc_info *f, float t) { return (f->a * t + f->b) / (f->c * t + f->d); }
static float or_phi_derivative(const or_fbcc_info *f, float t)
{
    return (f->a * f->d - f->b * f->c) / (f->c * f->c * t * t + 2 * f->c * f->d * t + f->d * f->d);
}

/* ref: ProjectiveGeometry.hxx:202-214 (meet of two planes -> line) and :226-235 (meet of a line and a plane) */
static void or_meet_planes(const double *A, const double *B, double *L)
{
    L[0] = A[2] * B[3] - A[3] * B[2];
    L[1] = A[3] * B[1] - A[1] * B[3];
    L[2] = A[1] * B[2] - A[2] * B[1];
    L[3] = A[0] * B[3] - A[3] * B[0];
    L[4] = A[2] * B[0] - A[0] * B[2];
    L[5] = A[0] * B[1] - A[1] * B[0];
}
static void or_meet_line_plane(const double *L, const double *P, double *X)
{
    X[0] = -P[1] * L[0] - P[2] * L[1] - P[3] * L[2];
    X[1] = +P[0] * L[0] - P[2] * L[3] - P[3] * L[4];
    X[2] = +P[0] * L[1] + P[1] * L[3] - P[3] * L[5];
    X[3] = +P[0] * L[2] + P[1] * L[4] + P[2] * L[5];
}
/* ref: ProjectiveGeometry.hxx:75-91 / :38-54 (dehomogenize) */
static void or_dehom3(double *X)
{
    if (X[3] > 1e-12 || X[3] < -1e-12) { X[0] /= X[3]; X[1] /= X[3]; X[2] /= X[3]; X[3] = 1; }
    else { double n; X[3] = 0; n = sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]); X[0] /= n; X[1] /= n; X[2] /= n; }
}
static void or_dehom2(double *x)
{
    if (x[2] > 1e-11 || x[2] < -1e-11) { x[0] /= x[2]; x[1] /= x[2]; x[2] = 1; }
    else { double n; x[2] = 0; n = sqrt(x[0] * x[0] + x[1] * x[1]); x[0] /= n; x[1] /= n; }
}

/* Pair-level part: the rectifying homography H = P_E * centralProjectionToPlane(C, E) * P^+ of one view
 * (ref: ...Direct.cpp:133-151, ProjectiveGeometry.hxx:333-342).  H is 3x3 row-major here. */
static void or_fbcc_homography(const double *P, const double *C, const double *U, const double *V,
                               const double *E, double *H)
{
    or_rowqr f;
    double Linv[3][3], Pinv[4][3], CP[4][4], T[3][4], PE[3][4];
    int i, j, k;
    or_row_qr(P, &f);
    /* L^-1 (lower triangular), then P^+ = Q^T L^-1 */
    memset(Linv, 0, sizeof(Linv));
    for (i = 0; i < 3; i++) {
        Linv[i][i] = 1.0 / f.L[i][i];
        for (j = 0; j < i; j++) {
            double sum = 0;
            for (k = j; k < i; k++) sum += f.L[i][k] * Linv[k][j];
            Linv[i][j] = -sum / f.L[i][i];
        }
    }
    for (i = 0; i < 4; i++)
        for (j = 0; j < 3; j++) {
            double sum = 0;
            for (k = 0; k < 3; k++) sum += f.Q[k][i] * Linv[k][j];
            Pinv[i][j] = sum;
        }
    CP[0][0] = +C[1] * E[1] + C[2] * E[2] + C[3] * E[3]; CP[0][1] = -C[0] * E[1]; CP[0][2] = -C[0] * E[2]; CP[0][3] = -C[0] * E[3];
    CP[1][0] = -C[1] * E[0]; CP[1][1] = +C[0] * E[0] + C[2] * E[2] + C[3] * E[3]; CP[1][2] = -C[1] * E[2]; CP[1][3] = -C[1] * E[3];
    CP[2][0] = -C[2] * E[0]; CP[2][1] = -C[2] * E[1]; CP[2][2] = +C[0] * E[0] + C[3] * E[3] + C[1] * E[1]; CP[2][3] = -C[2] * E[3];
    CP[3][0] = -C[3] * E[0]; CP[3][1] = -C[3] * E[1]; CP[3][2] = -C[3] * E[2]; CP[3][3] = +C[0] * E[0] + C[1] * E[1] + C[2] * E[2];
    memset(PE, 0, sizeof(PE));
    for (k = 0; k < 3; k++) { PE[0][k] = U[k]; PE[1][k] = V[k]; }
    PE[2][3] = 1.0; /* pixel_spacing */
    for (i = 0; i < 3; i++)
        for (j = 0; j < 4; j++) {
            double sum = 0;
            for (k = 0; k < 4; k++) sum += PE[i][k] * CP[k][j];
            T[i][j] = sum;
        }
    for (i = 0; i < 3; i++)
        for (j = 0; j < 3; j++) {
            double sum = 0;
            for (k = 0; k < 4; k++) sum += T[i][k] * Pinv[k][j];
            H[3 * i + j] = sum;
        }
}

/* Line-level part (ref: ...Direct.cpp:153-191): l is the epipolar line (float, as uploaded), dvec the baseline
 * direction, E the virtual detector plane. */
static void or_fbcc_line_info(const double *P, const double *C, const double *H, const double *dvec,
                              const double *E, const float *lf, or_fbcc_info *out)
{
    double l[3] = {lf[0], lf[1], lf[2]}, Ek[4], EB[4], M[6], Ak[4], ak[3], diff, dist = 0, t_ak;
    double a, b, c, d;
    int k;
    for (k = 0; k < 4; k++) Ek[k] = P[0 + 3 * k] * l[0] + P[1 + 3 * k] * l[1] + P[2 + 3 * k] * l[2]; /* P^T l */
    EB[0] = dvec[0]; EB[1] = dvec[1]; EB[2] = dvec[2];
    EB[3] = -(dvec[0] * C[0] + dvec[1] * C[1] + dvec[2] * C[2]);
    or_meet_planes(EB, Ek, M);
    or_meet_line_plane(M, E, Ak);
    or_dehom3(Ak);
    for (k = 0; k < 4; k++) { diff = Ak[k] - C[k]; dist += diff * diff; }
    {
        float d_px = (float)(sqrt(dist) / 1.0);
        out->d_l_kappa_C_sq = d_px * d_px;
    }
    for (k = 0; k < 3; k++) ak[k] = P[k + 0] * Ak[0] + P[k + 3] * Ak[1] + P[k + 6] * Ak[2] + P[k + 9] * Ak[3];
    or_dehom2(ak);
    /* ref: RectifiedFBCC.h:46-56 (LinePerspectivity(H, l)) */
    a = H[0] * l[1] - H[3] * l[0];
    b = H[2] - H[0] * l[0] * l[2];
    c = H[6] * l[1] - H[7] * l[0];
    d = H[8] - H[6] * l[0] * l[2] - H[7] * l[1] * l[2];
    out->a = (float)a; out->b = (float)b; out->c = (float)c; out->d = (float)d;
    if (out->a * out->d - out->b * out->c < 0) { out->a *= -1; out->b *= -1; }
    t_ak = l[1] * ak[0] / ak[2] - l[0] * ak[1] / ak[2]; /* project_to_line, :33-35 */
    out->t_prime_ak = or_phi_transform(out, (float)t_ak);
}

/* ref: EpipolarConsistencyDirect.cu:87-101 (the fbcc_d branch of kernel_computeLineIntegrals) */
static float or_direct_line_integral_fbcc(const float *img, int n_u, int n_v, const float *line,
                                          const or_fbcc_info *fbcc)
{
    float l[3] = {line[0], line[1], line[2]};
    float o[2] = {-l[2] * l[0], -l[2] * l[1]};
    float d[2] = {l[1], -l[0]};
    float ts[4], t_min, t_max, t, sum = 0;
    const float step = 0.4f;
    ts[0] = (1 - o[0]) / d[0];
    ts[1] = (n_u - 1 - o[0]) / d[0];
    ts[2] = (1 - o[1]) / d[1];
    ts[3] = (n_v - 1 - o[1]) / d[1];
    if (d[0] * d[0] < 1e-12) ts[0] = -(ts[1] = 1e10f);
    if (d[1] * d[1] < 1e-12) ts[2] = -(ts[3] = 1e10f);
    or_sort4(ts);
    t_min = ts[1];
    t_max = ts[2];
    {
        float u = o[0] + t_min * d[0], v = o[1] + t_min * d[1];
        if (!(u <= n_u && v <= n_v && u >= 0 && v >= 0)) return 0.f;
    }
    o[0] += .5f;
    o[1] += .5f;
    for (t = t_min; t <= t_max; t += step) {
        float u_prime = or_phi_transform(fbcc, t) - fbcc->t_prime_ak;
        float fbcc_weight = or_phi_derivative(fbcc, t) / sqrtf(u_prime * u_prime + fbcc->d_l_kappa_C_sq);
        sum += step * eccor_tex2d(img, n_u, n_v, o[0] + t * d[0], o[1] + t * d[1]) * fbcc_weight;
    }
    return sum;
}

static int g_direct_fbcc = 0;
ECCOR_API void eccor_set_direct_fbcc(int v) { g_direct_fbcc = v; }

/* ref: EpipolarConsistencyDirect.cpp:67-219 (computeForImagePair; fbcc via eccor_set_direct_fbcc) with computeEpipolarLines
 * (:23-65) and estimateAngularRange (EpipolarConsistency.cpp:49-59).  object_radius_mm <= 0: the larger of the
 * two views' estimates (:88-90).  Output arrays hold `capacity` entries (nullable); lines01: 6 floats per kappa.
 * Returns n_lines; *metric = sum (v0-v1)^2 dkappa (float difference and square, double sum, :206-208). */
static int or_direct_pair_body(const double *P0, const double *P1, const float *img0, const float *img1,
                               int n_u, int n_v, double dkappa, double object_radius_mm, int n_user_kappas,
                               const float *user_kappas, int n_user_lines, const float *user_lines, int capacity,
                               float *v0s, float *v1s, float *kappas, float *lines01, double *metric)
{
    const double Pi = 3.14159265358979323846264338327950288419716939937510582;
    double C0[4], C1[4], B[6], E0[4], E90[4], origin3[4] = {0, 0, 0, 1};
    double mom, dir, baseline_dist, k_first, k_second, n0, n90, acc = 0;
    or_rowqr f0, f1;
    int n_lines, i;
    eccor_camera_center(P0, C0);
    eccor_camera_center(P1, C1);
    or_join_points(C0, C1, B);
    if (object_radius_mm <= 0) {
        double a = eccor_object_radius(P0, n_u, n_v), b = eccor_object_radius(P1, n_u, n_v);
        object_radius_mm = a > b ? a : b;
    }
    /* ref: ProjectiveGeometry.hxx:238-268 (moment, direction, distance to origin) */
    mom = sqrt(B[3] * B[3] + B[1] * B[1] + B[0] * B[0]);
    dir = sqrt(B[2] * B[2] + B[4] * B[4] + B[5] * B[5]);
    baseline_dist = mom / dir;
    if (baseline_dist <= object_radius_mm) { k_first = -0.5 * Pi; k_second = 0.5 * Pi; }
    else { double km = fabs(asin(object_radius_mm / baseline_dist)); k_first = -km; k_second = km; }
    if (dkappa <= 0) {
        double diag = sqrt((double)(n_u * n_u + n_v * n_v));
        dkappa = 0.5 * (k_second - k_first) / diag;
    }
    {
        double nl = (k_second - k_first) / dkappa;
        n_lines = nl >= 0 ? (nl < 2147483000.0 ? (int)nl : 2147483000) : 0; /* NaN (coincident source positions): no lines */
    }
    if (user_kappas) n_lines = n_user_kappas; /* ref: :105-106, a non-empty `kappas` is taken as the grid */
    if (user_lines) n_lines = n_user_lines;
    or_join_line_point(B, origin3, E0);
    or_join_line_point(B, E0, E90);
    n0 = sqrt(E0[0] * E0[0] + E0[1] * E0[1] + E0[2] * E0[2]);
    n90 = sqrt(E90[0] * E90[0] + E90[1] * E90[1] + E90[2] * E90[2]);
    for (i = 0; i < 4; i++) { E0[i] /= n0; E90[i] /= n90; }
    or_row_qr(P0, &f0);
    or_row_qr(P1, &f1);
    double dvec[3] = {-B[2], -B[4], -B[5]}, mvec[3] = {B[3], -B[1], B[0]}, U[3], V[3], Eplane[4], H0[9], H1[9];
    if (g_direct_fbcc) {
        /* virtual detector plane spanned by the baseline direction and its moment (ref: :133-141) */
        for (i = 0; i < 3; i++) { U[i] = dvec[i] / dir; V[i] = mvec[i] / mom; }
        or_cross(U, V, Eplane);
        Eplane[3] = 0;
        or_fbcc_homography(P0, C0, U, V, Eplane, H0);
        or_fbcc_homography(P1, C1, U, V, Eplane, H1);
    }
    float *dv = (float *)malloc(sizeof(float) * 2 * (size_t)(n_lines > 0 ? n_lines : 1));
#pragma omp parallel for schedule(dynamic, 16)
    for (i = 0; i < n_lines; i++) {
        float kf = user_kappas && i < n_user_kappas ? user_kappas[i] : (float)(k_first + dkappa * i);
        double kappa = kf, c = cos(kappa), s = sin(kappa), E[4], l0[3], l1[3], nn;
        float lf[6], v0, v1;
        int k;
        if (user_lines) {
            memcpy(lf, user_lines + 6 * (size_t)i, sizeof(lf));
        } else {
            for (k = 0; k < 4; k++) E[k] = c * E0[k] + s * E90[k];
            or_plane_to_line(&f0, E, l0);
            or_plane_to_line(&f1, E, l1);
            nn = sqrt(l0[0] * l0[0] + l0[1] * l0[1]);
            for (k = 0; k < 3; k++) lf[k] = (float)(l0[k] / nn);
            nn = sqrt(l1[0] * l1[0] + l1[1] * l1[1]);
            for (k = 0; k < 3; k++) lf[3 + k] = (float)(l1[k] / nn);
        }
        if (g_direct_fbcc) {
            or_fbcc_info i0, i1;
            or_fbcc_line_info(P0, C0, H0, dvec, Eplane, lf, &i0);
            or_fbcc_line_info(P1, C1, H1, dvec, Eplane, lf + 3, &i1);
            v0 = or_direct_line_integral_fbcc(img0, n_u, n_v, lf, &i0);
            v1 = or_direct_line_integral_fbcc(img1, n_u, n_v, lf + 3, &i1);
        } else {
            v0 = or_direct_line_integral(img0, n_u, n_v, lf);
            v1 = or_direct_line_integral(img1, n_u, n_v, lf + 3);
        }
        if (i < capacity) {
            if (v0s) v0s[i] = v0;
            if (v1s) v1s[i] = v1;
            if (kappas) kappas[i] = kf;
            if (lines01) memcpy(lines01 + 6 * (size_t)i, lf, sizeof(lf));
        }
        dv[2 * i] = v0;
        dv[2 * i + 1] = v1;
    }
    /* ref: :205-208, the host sums in line order (deterministic here too) */
    for (i = 0; i < n_lines; i++) acc += (dv[2 * i] - dv[2 * i + 1]) * (dv[2 * i] - dv[2 * i + 1]) * dkappa;
    free(dv);
    if (metric) *metric = acc;
    return n_lines;
}

ECCOR_API int eccor_direct_pair(const double *P0, const double *P1, const float *img0, const float *img1,
                                int n_u, int n_v, double dkappa, double object_radius_mm, int capacity,
                                float *v0s, float *v1s, float *kappas, float *lines01, double *metric)
{
    return or_direct_pair_body(P0, P1, img0, img1, n_u, n_v, dkappa, object_radius_mm, 0, NULL, 0, NULL, capacity, v0s, v1s,
                               kappas, lines01, metric);
}

/* The same with a caller's grid and / or a caller's lines.  user_kappas (n_user_kappas floats, or NULL): taken as the plane
 * angles (ref: EpipolarConsistencyDirect.cpp:105-117); dkappa of the metric is unchanged.  user_lines (6 floats per line:
 * image 0's line, image 1's; or NULL): used INSTEAD of the lines of the plane angles -- clipping, the 0.4-px loop and the
 * line-level fan-beam weighting run on them as on lines computed here.  With both, the counts must agree and the angles are
 * only reported.  With lines alone the reported angles are the automatic grid's.  Returns n_lines, or -1 for such a
 * mismatch or a negative count. */
ECCOR_API int eccor_direct_pair_with(const double *P0, const double *P1, const float *img0, const float *img1,
                                     int n_u, int n_v, double dkappa, double object_radius_mm, int n_user_kappas,
                                     const float *user_kappas, int n_user_lines, const float *user_lines, int capacity,
                                     float *v0s, float *v1s, float *kappas, float *lines01, double *metric)
{
    if (!user_kappas) n_user_kappas = 0;
    if (!user_lines) n_user_lines = 0;
    if (n_user_kappas < 0 || n_user_lines < 0) return -1;
    if (user_kappas && user_lines && n_user_kappas != n_user_lines) return -1;
    return or_direct_pair_body(P0, P1, img0, img1, n_u, n_v, dkappa, object_radius_mm, n_user_kappas, user_kappas,
                               n_user_lines, user_lines, capacity, v0s, v1s, kappas, lines01, metric);
}

ECCOR_API void eccor_set_num_threads(int n)
{
#ifdef _OPENMP
    if (n > 0) omp_set_num_threads(n);
#else
    (void)n;
#endif
}

ECCOR_API int eccor_num_threads(void)
{
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}
