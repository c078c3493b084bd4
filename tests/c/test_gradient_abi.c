/* The gradient entry points of include/ecc_hip.h from C99 (gcc -std=c99 -pedantic -Wall -Wextra -Werror, linked against
 * libecc_hip.so by tests/test_gradient_abi.py): the prototypes are C, a null metric is an argument error with a message, and
 * nothing needs a device. */
#include <stdio.h>
#include <string.h>

#include "ecc_hip.h"

int main(void)
{
    int (*gradient)(ecc_metric*, int, int, const double*, const double*, const double*, double*, double*, double*) =
        ecc_metric_evaluate_gradient;
    int (*last_path)(const ecc_metric*, int*) = ecc_metric_last_gradient_path;
    int (*launch_switch)(ecc_metric*, int) = ecc_debug_set_gradient_launch;
    double P[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}, h = 0.5, value = -1.0, grad = -1.0, probes[2] = {-1.0, -1.0};
    int path = -1;
    if (gradient(NULL, 0, 1, P, P, &h, &value, &grad, probes) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (strlen(ecc_last_error()) == 0) return 2;
    if (value != -1.0 || grad != -1.0 || probes[0] != -1.0) return 3; /* nothing written */
    if (last_path(NULL, &path) != ECC_ERR_INVALID_ARGUMENT || path != -1) return 4;
    if (launch_switch(NULL, 0) != ECC_ERR_INVALID_ARGUMENT) return 5;
    printf("gradient abi ok\n");
    return 0;
}
