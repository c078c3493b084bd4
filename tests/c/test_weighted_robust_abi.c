/* ecc_metric_evaluate_weighted_robust, ecc_metric_evaluate_weighted_robust_pairs and ecc_host_weighted_robust_scale of
 * include/ecc_hip.h from C99 (gcc -std=c99 -pedantic -Wall -Wextra -Werror, linked against libecc_hip.so by
 * tests/test_weighted_robust_abi.py): the prototypes are C, a null metric is an argument error with a message whatever the other
 * arguments are, nothing is written, the scale is the median rule of the header, and nothing needs a device. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "ecc_hip.h"

int main(void)
{
    int (*all_call)(ecc_metric*, int, float, double*, double*, double*, float*) = ecc_metric_evaluate_weighted_robust;
    int (*pairs_call)(ecc_metric*, const int32_t*, int, int, float, double*, double*, double*, float*) = ecc_metric_evaluate_weighted_robust_pairs;
    double (*scale_call)(const float*, int64_t, double) = ecc_host_weighted_robust_scale;
    const int32_t idx[8] = {0, 1, 0, 1, 1, 2, 1, 2};
    /* rows {c, u, k, r}: sqrt(r / u) = 3, - (r = 0), 1, 2, 5, - (u = 0) -> the live rows sorted: 1 2 3 5 */
    const float rows[24] = {7.f, 1.f,  1.f, 9.f,  7.f, 1.f,   1.f, 0.f,   7.f, 0.25f, 0.f, 0.25f,
                            7.f, 0.5f, 0.f, 2.f,  7.f, 0.0625f, 0.f, 1.5625f,  7.f, 0.f,   0.f, 3.f};
    double value = -1.0, coverage = -1.0, mass = -1.0;
    float terms[8];
    int k;
    for (k = 0; k < 8; ++k) terms[k] = -1.0f;
    if (all_call(NULL, ECC_LOSS_HUBER, 1.0f, &value, &coverage, &mass, terms) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (strlen(ecc_last_error()) == 0) return 2;
    if (all_call(NULL, 7, -1.0f, NULL, NULL, NULL, NULL) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (pairs_call(NULL, idx, 2, ECC_LOSS_TRUNCATED, 1.0f, &value, &coverage, &mass, terms) != ECC_ERR_INVALID_ARGUMENT) return 4;
    if (strlen(ecc_last_error()) == 0) return 4;
    if (pairs_call(NULL, NULL, 0, ECC_LOSS_GEMAN_MCCLURE, 1.0f, NULL, NULL, NULL, NULL) != ECC_ERR_INVALID_ARGUMENT) return 4;
    if (pairs_call(NULL, idx, 0, ECC_LOSS_HUBER, 1.0f, &value, NULL, NULL, NULL) != ECC_ERR_INVALID_ARGUMENT) return 4;
    if (value != -1.0 || coverage != -1.0 || mass != -1.0) return 5; /* nothing written */
    for (k = 0; k < 8; ++k)
        if (terms[k] != -1.0f) return 5;
    if (scale_call(rows, 6, 1.0) != 2.5) return 6;       /* even count: the mean of the two middle values */
    if (scale_call(rows, 4, 2.0) != 4.0) return 6;       /* 1 2 3: the middle one, times k */
    if (scale_call(rows + 4, 1, 1.0) != 0.0) return 7;   /* r == 0 */
    if (scale_call(rows + 20, 1, 1.0) != 0.0) return 7;  /* u == 0 */
    if (scale_call(NULL, 0, 1.0) != 0.0) return 7;
    if (fabs(scale_call(rows + 16, 1, 1.4826) - 5.0 * 1.4826) > 1e-14) return 8;
    printf("weighted robust abi ok\n");
    return 0;
}
