/* ecc_metric_evaluate_variance, its index-list, pose-delta and transform forms and ecc_host_variance_floor of include/ecc_hip.h from
 * C99 (gcc -std=c99 -pedantic -Wall -Wextra -Werror, linked against libecc_hip.so by tests/test_variance_abi.py): the prototypes
 * are C, a null metric is an argument error with a message whatever the other arguments are, nothing is written, the host helper
 * computes and refuses, and nothing needs a device. */
#include <stdio.h>
#include <string.h>

#include "ecc_hip.h"

int main(void)
{
    int (*all)(ecc_metric*, float, double*, double*, float*) = ecc_metric_evaluate_variance;
    int (*list)(ecc_metric*, const int32_t*, int, float, double*, double*, float*) = ecc_metric_evaluate_variance_pairs;
    int (*poses)(ecc_metric*, int, const int32_t*, const int32_t*, const double*, float, double*, double*) = ecc_metric_evaluate_variance_pose_deltas;
    int (*transforms)(ecc_metric*, int, int, const double*, float, double*, double*, float*) = ecc_metric_evaluate_variance_transforms;
    int (*host_floor)(const float*, int64_t, double, float*) = ecc_host_variance_floor;
    double value = -1.0, mean_weight = -1.0;
    float pairs[6];
    const int32_t idx4[4] = {0, 1, 0, 1}, off[2] = {0, 1}, views[1] = {0};
    double P[12], T[16];
    const float v[6] = {0.0f, 4.0f, -1.0f, 1.0f, 2.0f, 8.0f};
    float f = -1.0f;
    int k;
    for (k = 0; k < 6; ++k) pairs[k] = -1.0f;
    for (k = 0; k < 12; ++k) P[k] = 0.0;
    for (k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.0 : 0.0;
    if (all(NULL, 1.0f, &value, &mean_weight, pairs) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (strlen(ecc_last_error()) == 0) return 2;
    if (all(NULL, 1.0f, NULL, NULL, NULL) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (list(NULL, idx4, 1, 1.0f, &value, &mean_weight, pairs) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (poses(NULL, 1, off, views, P, 1.0f, &value, &mean_weight) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (transforms(NULL, 1, 1, T, 1.0f, &value, &mean_weight, pairs) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (strlen(ecc_last_error()) == 0) return 4;
    if (value != -1.0 || mean_weight != -1.0) return 5; /* nothing written */
    for (k = 0; k < 6; ++k)
        if (pairs[k] != -1.0f) return 5;
    /* the positive entries are 1, 2, 4, 8: the median is 3 */
    if (host_floor(v, 6, 0.5, &f) != ECC_OK || f != 1.5f) return 6;
    if (host_floor(v, 1, 0.5, &f) != ECC_ERR_INVALID_ARGUMENT || f != 1.5f) return 7;
    if (host_floor(NULL, 6, 0.5, &f) != ECC_ERR_INVALID_ARGUMENT || host_floor(v, 6, 0.5, NULL) != ECC_ERR_INVALID_ARGUMENT) return 7;
    if (host_floor(v, -1, 0.5, &f) != ECC_ERR_INVALID_ARGUMENT || host_floor(v, 6, 0.0, &f) != ECC_ERR_INVALID_ARGUMENT) return 7;
    printf("variance abi ok\n");
    return 0;
}
