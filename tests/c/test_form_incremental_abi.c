/* ecc_metric_set_form_incremental / ecc_metric_last_form_base_pairs from C99 (gcc -std=c99 -pedantic -Wall -Wextra -Werror): the
 * prototypes of include/ecc_hip.h as a C compiler sees them, and the argument errors that need no device. */
#include <stdio.h>
#include <string.h>

#include "ecc_hip.h"

int main(void)
{
    int (*set_mode)(ecc_metric*, int) = ecc_metric_set_form_incremental;
    int (*last)(const ecc_metric*, int64_t*) = ecc_metric_last_form_base_pairs;
    int64_t pairs = -7;
    int enable;
    for (enable = -1; enable <= 2; ++enable) {
        if (set_mode(NULL, enable) != ECC_ERR_INVALID_ARGUMENT || !strstr(ecc_last_error(), "null")) {
            printf("set_form_incremental(NULL, %d): %s\n", enable, ecc_last_error());
            return 1;
        }
    }
    if (last(NULL, &pairs) != ECC_ERR_INVALID_ARGUMENT || !strstr(ecc_last_error(), "null") || pairs != -7) {
        printf("last_form_base_pairs(NULL, &pairs): %s\n", ecc_last_error());
        return 1;
    }
    if (last(NULL, NULL) != ECC_ERR_INVALID_ARGUMENT || !strstr(ecc_last_error(), "null")) {
        printf("last_form_base_pairs(NULL, NULL): %s\n", ecc_last_error());
        return 1;
    }
    printf("form incremental abi ok\n");
    return 0;
}
