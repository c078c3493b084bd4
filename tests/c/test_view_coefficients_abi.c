/* ecc_metric_evaluate_view_coefficients of include/ecc_hip.h from C99 (gcc -std=c99 -pedantic -Wall -Wextra -Werror, linked
 * against libecc_hip.so by tests/test_view_coefficients_abi.py): the prototype is C, a null metric, a null value and null
 * coefficients are argument errors with a message, and nothing needs a device. */
#include <stdio.h>
#include <string.h>

#include "ecc_hip.h"

int main(void)
{
    int (*call)(ecc_metric*, int, const float*, double*, double*, float*) = ecc_metric_evaluate_view_coefficients;
    const float coeffs[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    double value = -1.0, grad[4] = {-1.0, -1.0, -1.0, -1.0};
    float pairs[5] = {-1.0f, -1.0f, -1.0f, -1.0f, -1.0f};
    if (call(NULL, 2, coeffs, &value, grad, pairs) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (strlen(ecc_last_error()) == 0) return 2;
    if (call(NULL, 2, coeffs, NULL, NULL, NULL) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (call(NULL, 2, NULL, &value, NULL, NULL) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (strlen(ecc_last_error()) == 0) return 4;
    if (value != -1.0 || grad[0] != -1.0 || pairs[0] != -1.0f) return 5; /* nothing written */
    if (ECC_VIEW_COEFF_MAX_CHANNELS != 4) return 6;
    printf("view coefficients abi ok\n");
    return 0;
}
