/* ecc_metric_evaluate_weighted of include/ecc_hip.h from C99 (gcc -std=c99 -pedantic -Wall -Wextra -Werror, linked against
 * libecc_hip.so by tests/test_weighted_abi.py): the prototype is C, a null metric is an argument error with a message whatever the
 * other arguments are, nothing is written, and nothing needs a device. */
#include <stdio.h>
#include <string.h>

#include "ecc_hip.h"

int main(void)
{
    int (*call)(ecc_metric*, double*, double*, float*) = ecc_metric_evaluate_weighted;
    double value = -1.0, coverage = -1.0;
    float pairs[6];
    int k;
    for (k = 0; k < 6; ++k) pairs[k] = -1.0f;
    if (call(NULL, &value, &coverage, pairs) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (strlen(ecc_last_error()) == 0) return 2;
    if (call(NULL, NULL, NULL, NULL) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (call(NULL, &value, NULL, NULL) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (call(NULL, NULL, &coverage, pairs) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (strlen(ecc_last_error()) == 0) return 4;
    if (value != -1.0 || coverage != -1.0) return 5; /* nothing written */
    for (k = 0; k < 6; ++k)
        if (pairs[k] != -1.0f) return 5;
    printf("weighted abi ok\n");
    return 0;
}
