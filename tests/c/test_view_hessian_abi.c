/* ecc_metric_evaluate_view_hessian of include/ecc_hip.h from C99 (gcc -std=c99 -pedantic -Wall -Wextra -Werror, linked against
 * libecc_hip.so by tests/test_view_hessian_abi.py): the prototype is C, a null metric, two null outputs and a channel count out of
 * range are argument errors with a message, and nothing needs a device. */
#include <stdio.h>
#include <string.h>

#include "ecc_hip.h"

int main(void)
{
    int (*call)(ecc_metric*, int, double*, double*) = ecc_metric_evaluate_view_hessian;
    double hessian[4] = {-1.0, -1.0, -1.0, -1.0}, blocks[10];
    int k;
    for (k = 0; k < 10; ++k) blocks[k] = -1.0;
    if (call(NULL, 2, hessian, blocks) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (strlen(ecc_last_error()) == 0) return 2;
    if (call(NULL, 2, NULL, NULL) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (call(NULL, 0, hessian, NULL) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (call(NULL, 5, NULL, blocks) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (strlen(ecc_last_error()) == 0) return 4;
    for (k = 0; k < 10; ++k)
        if (blocks[k] != -1.0 || hessian[k & 3] != -1.0) return 5; /* nothing written */
    if (ECC_VIEW_HESSIAN_MAX_CHANNELS != 4 || ECC_VIEW_HESSIAN_MAX_DIM != 8192) return 6;
    printf("view hessian abi ok\n");
    return 0;
}
