/* ecc_metric_evaluate_gram of include/ecc_hip.h from C99 (gcc -std=c99 -pedantic -Wall -Wextra -Werror, linked against
 * libecc_hip.so by tests/test_gram_abi.py): the prototype is C, a null metric and a null result are argument errors with a
 * message, and nothing needs a device. */
#include <stdio.h>
#include <string.h>

#include "ecc_hip.h"

int main(void)
{
    int (*gram_call)(ecc_metric*, int, float*, double*) = ecc_metric_evaluate_gram;
    double G[ECC_GRAM_MAX_CHANNELS * ECC_GRAM_MAX_CHANNELS];
    float pairs[3] = {-1.0f, -1.0f, -1.0f};
    int k;
    for (k = 0; k < ECC_GRAM_MAX_CHANNELS * ECC_GRAM_MAX_CHANNELS; ++k) G[k] = -1.0;
    if (gram_call(NULL, 2, pairs, G) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (strlen(ecc_last_error()) == 0) return 2;
    if (gram_call(NULL, 2, NULL, NULL) != ECC_ERR_INVALID_ARGUMENT) return 3;
    if (strlen(ecc_last_error()) == 0) return 4;
    if (G[0] != -1.0 || pairs[0] != -1.0f) return 5; /* nothing written */
    if (ECC_GRAM_MAX_CHANNELS != 4) return 6;
    printf("gram abi ok\n");
    return 0;
}
