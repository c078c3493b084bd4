/* ecc_metric_evaluate_weighted_pairs and ecc_metric_evaluate_weighted_pose_deltas of include/ecc_hip.h from C99 (gcc -std=c99
 * -pedantic -Wall -Wextra -Werror, linked against libecc_hip.so by tests/test_weighted_poses_abi.py): the prototypes are C, a null
 * metric is an argument error with a message whatever the other arguments are, nothing is written, and nothing needs a device. */
#include <stdio.h>
#include <string.h>

#include "ecc_hip.h"

int main(void)
{
    int (*pairs_call)(ecc_metric*, const int32_t*, int, double*, double*, float*) = ecc_metric_evaluate_weighted_pairs;
    int (*poses_call)(ecc_metric*, int, const int32_t*, const int32_t*, const double*, double*, double*) = ecc_metric_evaluate_weighted_pose_deltas;
    const int32_t idx[8] = {0, 1, 0, 1, 1, 2, 1, 2};
    const int32_t off[3] = {0, 1, 2}, views[2] = {0, 1};
    double Ps[24];
    double value = -1.0, coverage = -1.0, values[2] = {-1.0, -1.0}, coverages[2] = {-1.0, -1.0};
    float terms[4];
    int k;
    for (k = 0; k < 24; ++k) Ps[k] = 0.0;
    for (k = 0; k < 4; ++k) terms[k] = -1.0f;
    if (pairs_call(NULL, idx, 2, &value, &coverage, terms) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (strlen(ecc_last_error()) == 0) return 2;
    if (pairs_call(NULL, NULL, 0, NULL, NULL, NULL) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (pairs_call(NULL, idx, 0, &value, NULL, NULL) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (poses_call(NULL, 2, off, views, Ps, values, coverages) != ECC_ERR_INVALID_ARGUMENT) return 4;
    if (strlen(ecc_last_error()) == 0) return 4;
    if (poses_call(NULL, 0, NULL, NULL, NULL, NULL, NULL) != ECC_ERR_INVALID_ARGUMENT) return 4;
    if (poses_call(NULL, 2, off, views, Ps, values, NULL) != ECC_ERR_INVALID_ARGUMENT) return 4;
    if (value != -1.0 || coverage != -1.0) return 5; /* nothing written */
    for (k = 0; k < 4; ++k)
        if (terms[k] != -1.0f) return 5;
    for (k = 0; k < 2; ++k)
        if (values[k] != -1.0 || coverages[k] != -1.0) return 5;
    printf("weighted poses abi ok\n");
    return 0;
}
