/* ecc_metric_evaluate_variance_robust, its index-list, pose-delta and transform forms and ecc_host_variance_robust_scale of
 * include/ecc_hip.h from C99 (gcc -std=c99 -pedantic -Wall -Wextra -Werror, linked against libecc_hip.so by
 * tests/test_variance_robust_abi.py): the prototypes are C, a null metric is an argument error with a message whatever the other
 * arguments are, nothing is written, the host helper computes, and nothing needs a device. */
#include <stdio.h>
#include <string.h>

#include "ecc_hip.h"

int main(void)
{
    int (*all)(ecc_metric*, int, float, float, double*, double*, double*, float*) = ecc_metric_evaluate_variance_robust;
    int (*list)(ecc_metric*, const int32_t*, int, int, float, float, double*, double*, double*, float*) = ecc_metric_evaluate_variance_robust_pairs;
    int (*poses)(ecc_metric*, int, const int32_t*, const int32_t*, const double*, int, float, float, double*, double*, double*) =
        ecc_metric_evaluate_variance_robust_pose_deltas;
    int (*transforms)(ecc_metric*, int, int, const double*, int, float, float, double*, double*, double*, float*) =
        ecc_metric_evaluate_variance_robust_transforms;
    double (*scale)(const float*, int64_t, double) = ecc_host_variance_robust_scale;
    double value = -1.0, mean_weight = -1.0, inlier_mass = -1.0;
    float pairs[8];
    const int32_t idx4[4] = {0, 1, 0, 1}, off[2] = {0, 1}, views[1] = {0};
    double P[12], T[16];
    /* r = 4, 0, 9, 16: the live roots are 2, 3, 4 */
    const float rows[16] = {0.0f, 1.0f, 1.0f, 4.0f, 0.0f, 1.0f, 1.0f, 0.0f, 0.0f, 1.0f, 1.0f, 9.0f, 0.0f, 1.0f, 1.0f, 16.0f};
    int k;
    for (k = 0; k < 8; ++k) pairs[k] = -1.0f;
    for (k = 0; k < 12; ++k) P[k] = 0.0;
    for (k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.0 : 0.0;
    if (all(NULL, ECC_LOSS_TRUNCATED, 2.0f, 1.0f, &value, &mean_weight, &inlier_mass, pairs) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (strlen(ecc_last_error()) == 0) return 2;
    if (all(NULL, 7, -1.0f, 0.0f, NULL, NULL, NULL, NULL) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (list(NULL, idx4, 1, ECC_LOSS_HUBER, 2.0f, 1.0f, &value, &mean_weight, &inlier_mass, pairs) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (poses(NULL, 1, off, views, P, ECC_LOSS_GEMAN_MCCLURE, 2.0f, 1.0f, &value, &mean_weight, &inlier_mass) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (transforms(NULL, 1, 1, T, ECC_LOSS_TRUNCATED, 2.0f, 1.0f, &value, &mean_weight, &inlier_mass, pairs) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (strlen(ecc_last_error()) == 0) return 4;
    if (value != -1.0 || mean_weight != -1.0 || inlier_mass != -1.0) return 5; /* nothing written */
    for (k = 0; k < 8; ++k)
        if (pairs[k] != -1.0f) return 5;
    if (scale(rows, 4, 2.0) != 6.0) return 6;           /* odd count of live rows: the middle one */
    if (scale(rows, 3, 1.0) != 2.5) return 6;           /* even: the mean of the two middle ones */
    if (scale(rows + 4, 1, 1.0) != 0.0) return 7;       /* no live row */
    if (scale(NULL, 4, 1.0) != 0.0 || scale(rows, 0, 1.0) != 0.0) return 7;
    printf("variance robust abi ok\n");
    return 0;
}
