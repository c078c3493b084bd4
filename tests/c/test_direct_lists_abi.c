/* ecc_direct_evaluate_pairs, ecc_direct_evaluate_pose_deltas, ecc_direct_pose_pairs_bound and ecc_debug_set_direct_batch of
 * include/ecc_hip.h from C99 (gcc -std=c99 -pedantic -Wall -Wextra -Werror, linked against libecc_hip.so by
 * tests/test_direct_lists_abi.py).
 *   test_direct_lists_abi nodevice                 the argument errors that need no device
 *   test_direct_lists_abi <file> <n> <n_u> <n_v>   <file>: n x 12 float64 matrices (column-major), then n x n_v x n_u float32
 *                                                  pixels; prints the results as hexadecimal floats, which the test compares
 *                                                  with the Python calls' bits */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ecc_hip.h"

#define CHECK(call)                                                                     \
    do {                                                                                \
        int rc_ = (call);                                                               \
        if (rc_ != ECC_OK) {                                                            \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, ecc_last_error());      \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

static int nodevice(void)
{
    const int32_t idx4[4] = {0, 1, 0, 1}, off[2] = {0, 1}, views[1] = {0};
    double P[12] = {0}, out[1] = {-1.0};
    int64_t n = -1;
    if (ecc_direct_evaluate_pairs(NULL, idx4, 1, NULL, 1, out, out) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (!strstr(ecc_last_error(), "null")) return 1;
    if (ecc_direct_evaluate_pose_deltas(NULL, 1, off, views, P, out, NULL, NULL) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (ecc_direct_pose_pairs_bound(NULL, 1, off, &n) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (ecc_debug_set_direct_batch(NULL, 3) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (out[0] != -1.0 || n != -1) return 1; /* nothing written */
    printf("nodevice ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && strcmp(argv[1], "nodevice") == 0) return nodevice();
    if (argc != 5) return 2;
    const int n = atoi(argv[2]), n_u = atoi(argv[3]), n_v = atoi(argv[4]);
    if (n < 5) return 2;
    const size_t n_px = (size_t)n * (size_t)n_u * (size_t)n_v;
    double* Ps = (double*)malloc(sizeof(double) * 12 * (size_t)(n + 1));
    float* images = (float*)malloc(sizeof(float) * n_px);
    FILE* f = fopen(argv[1], "rb");
    if (!Ps || !images || !f) return 2;
    if (fread(Ps, sizeof(double), 12 * (size_t)n, f) != 12 * (size_t)n || fread(images, sizeof(float), n_px, f) != n_px) return 2;
    fclose(f);
    for (int k = 0; k < 12; ++k) Ps[12 * n + k] = 0.5 * (Ps[12 * 3 + k] + Ps[12 * 4 + k]); /* row n: a candidate for view 3 */

    ecc_ctx* ctx = NULL;
    ecc_direct* d = NULL;
    CHECK(ecc_ctx_create(0, NULL, &ctx));
    CHECK(ecc_direct_create(ctx, n, images, 0, n_u, n_v, &d));
    CHECK(ecc_direct_set_projections(d, Ps, n + 1));

    /* the list of one moved view (ref: Gui/SingleImageMotion.h): view 3 against every other view, then with the candidate row */
    int32_t* idx4 = (int32_t*)malloc(sizeof(int32_t) * 4 * 2 * (size_t)(n - 1));
    double* values = (double*)malloc(sizeof(double) * 2 * (size_t)(n - 1));
    int64_t q = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (int i = 0; i < n; ++i) {
            if (i == 3) continue;
            /* ascending image indices, as the pose batch lists them */
            idx4[4 * q + (i < 3)] = pass ? n : 3;
            idx4[4 * q + (i > 3)] = i;
            idx4[4 * q + 2 + (i < 3)] = 3;
            idx4[4 * q + 2 + (i > 3)] = i;
            ++q;
        }
    const int64_t segments[3] = {0, n - 1, 2 * (n - 1)};
    double sums[2] = {0, 0}, whole = 0, again[2] = {0, 0};
    CHECK(ecc_direct_evaluate_pairs(d, idx4, q, segments, 2, values, sums));
    CHECK(ecc_direct_evaluate_pairs(d, idx4, q, NULL, 0, NULL, &whole));
    CHECK(ecc_debug_set_direct_batch(d, 2));
    CHECK(ecc_direct_evaluate_pairs(d, idx4, q, segments, 2, NULL, again));
    CHECK(ecc_debug_set_direct_batch(d, 0));
    if (again[0] != sums[0] || again[1] != sums[1]) return 1;
    printf("segment_sums %a %a\nwhole %a\nfirst_value %a\nlast_value %a\n", sums[0], sums[1], whole, values[0], values[q - 1]);

    /* two poses: view 3 with the candidate; views 1 and 3 with each other's matrices */
    const int32_t off[3] = {0, 1, 3}, moved[3] = {3, 1, 3};
    double moved_Ps[36], pose_sums[2] = {0, 0};
    memcpy(moved_Ps, Ps + 12 * n, sizeof(double) * 12);
    memcpy(moved_Ps + 12, Ps + 12 * 3, sizeof(double) * 12);
    memcpy(moved_Ps + 24, Ps + 12 * 1, sizeof(double) * 12);
    int64_t bound = 0;
    CHECK(ecc_direct_pose_pairs_bound(d, 2, off, &bound));
    if (bound != (n - 1) + (2 * (n - 1) - 1)) return 1;
    double* terms = (double*)malloc(sizeof(double) * (size_t)bound);
    int32_t* tuples = (int32_t*)malloc(sizeof(int32_t) * 4 * (size_t)bound);
    CHECK(ecc_direct_evaluate_pose_deltas(d, 2, off, moved, moved_Ps, pose_sums, terms, tuples));
    printf("pose_sums %a %a\npose_pairs %lld\nlast_tuple %d %d %d %d\n", pose_sums[0], pose_sums[1], (long long)bound,
           (int)tuples[4 * (bound - 1)], (int)tuples[4 * (bound - 1) + 1], (int)tuples[4 * (bound - 1) + 2], (int)tuples[4 * (bound - 1) + 3]);
    if (pose_sums[0] != sums[1]) return 1; /* pose 0 is the second segment: the same pairs in the same order */

    /* a refusal leaves the metric usable */
    idx4[1] = idx4[0];
    if (ecc_direct_evaluate_pairs(d, idx4, q, NULL, 0, NULL, &whole) != ECC_ERR_INVALID_ARGUMENT || !strstr(ecc_last_error(), "P0 == P1")) return 1;
    double total = 0;
    CHECK(ecc_direct_evaluate(d, NULL, &total));
    printf("evaluate %a\nok\n", total);
    free(terms); free(tuples); free(values); free(idx4);
    CHECK(ecc_direct_destroy(d));
    CHECK(ecc_ctx_destroy(ctx));
    free(Ps); free(images);
    return 0;
}
