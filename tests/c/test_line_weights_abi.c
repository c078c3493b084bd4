/* The line-weight calls of include/ecc_hip.h from C99 (gcc -std=c99 -pedantic -Wall -Wextra -Werror, linked against libecc_hip.so by
 * tests/test_line_weights_abi.py): the prototypes and the config struct are C, ecc_line_weights_defaults writes {0, 1, 1.0f}, a null
 * context is an argument error with a message whatever the other arguments are, nothing is written, and nothing needs a device. */
#include <stdio.h>
#include <string.h>

#include "ecc_hip.h"

int main(void)
{
    void (*defaults)(ecc_line_weights_config*) = ecc_line_weights_defaults;
    int (*stack)(ecc_ctx*, const float*, int, int, int, int, int, int, const ecc_line_weights_config*, ecc_dtr**) = ecc_radon_line_weights;
    int (*into)(ecc_ctx*, const float*, int, int, int, int, int, const ecc_line_weights_config*, float*) = ecc_radon_line_weights_into;
    int (*from)(ecc_ctx*, const ecc_dtr*, const ecc_line_weights_config*, ecc_dtr**) = ecc_dtr_line_weights;
    ecc_line_weights_config cfg;
    float image[4] = {0.0f, 1.0f, 0.0f, 0.0f};
    float slab[4] = {-1.0f, -1.0f, -1.0f, -1.0f};
    ecc_dtr* out[2];
    ecc_dtr* const untouched = (ecc_dtr*)slab;
    int k;
    cfg.dilate_px = 7;
    cfg.guard_bins = 7;
    cfg.zero_at_px = 7.0f;
    defaults(&cfg);
    if (cfg.dilate_px != 0 || cfg.guard_bins != 1 || cfg.zero_at_px != 1.0f) return 1;
    defaults(NULL);
    out[0] = out[1] = untouched;
    if (stack(NULL, image, 0, 1, 2, 2, 4, 4, &cfg, out) != ECC_ERR_INVALID_ARGUMENT) return 2;
    if (strstr(ecc_last_error(), "context") == NULL) return 3;
    if (stack(NULL, NULL, 0, 0, 0, 0, 0, 0, NULL, NULL) != ECC_ERR_INVALID_ARGUMENT) return 2;
    if (strstr(ecc_last_error(), "context") == NULL) return 3;
    if (into(NULL, image, 1, 2, 2, 4, 4, &cfg, slab) != ECC_ERR_INVALID_ARGUMENT) return 4;
    if (strstr(ecc_last_error(), "context") == NULL) return 5;
    if (into(NULL, NULL, 0, 0, 0, 0, 0, NULL, NULL) != ECC_ERR_INVALID_ARGUMENT) return 4;
    if (from(NULL, NULL, &cfg, out) != ECC_ERR_INVALID_ARGUMENT) return 6;
    if (strstr(ecc_last_error(), "context") == NULL) return 7;
    if (from(NULL, NULL, NULL, NULL) != ECC_ERR_INVALID_ARGUMENT) return 6;
    if (out[0] != untouched || out[1] != untouched) return 8; /* nothing written */
    for (k = 0; k < 4; ++k)
        if (slab[k] != -1.0f) return 8;
    printf("line weights abi ok\n");
    return 0;
}
