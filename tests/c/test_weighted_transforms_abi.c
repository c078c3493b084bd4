/* ecc_metric_evaluate_weighted_transforms of include/ecc_hip.h from C99 (gcc -std=c99 -pedantic -Wall -Wextra -Werror, linked
 * against libecc_hip.so by tests/test_weighted_transforms_abi.py): the prototype is C, a null metric is an argument error with a
 * message whatever the other arguments are, nothing is written, and nothing needs a device. */
#include <stdio.h>
#include <string.h>

#include "ecc_hip.h"

int main(void)
{
    int (*call)(ecc_metric*, int, int, const double*, double*, double*, float*) = ecc_metric_evaluate_weighted_transforms;
    double Ts[32];
    double values[2] = {-1.0, -1.0}, coverages[2] = {-1.0, -1.0};
    float terms[8];
    int k;
    for (k = 0; k < 32; ++k) Ts[k] = (k % 5 == 0) ? 1.0 : 0.0;
    for (k = 0; k < 8; ++k) terms[k] = -1.0f;
    if (call(NULL, 1, 2, Ts, values, coverages, terms) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (strlen(ecc_last_error()) == 0 || strstr(ecc_last_error(), "null") == NULL) return 2;
    if (call(NULL, 1, 0, NULL, NULL, NULL, NULL) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (call(NULL, 0, -1, Ts, values, NULL, NULL) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (strstr(ecc_last_error(), "null") == NULL) return 3; /* the null metric comes first */
    if (call(NULL, 1, 2, NULL, NULL, NULL, NULL) != ECC_ERR_INVALID_ARGUMENT) return 4;
    for (k = 0; k < 2; ++k)
        if (values[k] != -1.0 || coverages[k] != -1.0) return 5; /* nothing written */
    for (k = 0; k < 8; ++k)
        if (terms[k] != -1.0f) return 5;
    printf("weighted transforms abi ok\n");
    return 0;
}
