// ecc_variance_host.h -- the host half of the variance form (include/ecc_hip.h: ecc_host_variance_floor), as a plain header without
// HIP includes so that tests/c/variance_host.cpp builds it alone, under the sanitizers.
#ifndef ECC_VARIANCE_HOST_H
#define ECC_VARIANCE_HOST_H

#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace ecc_variance_host {

enum { OK = 0, INVALID_ARGUMENT = 1 };  // == ECC_OK, ECC_ERR_INVALID_ARGUMENT (ecc_variance.hip asserts it)

// *floor = (float)(fraction x the median of the strictly positive finite entries of v[0 .. count)); an even number of them: the
// mean of the two middle ones.  INVALID_ARGUMENT (nothing written): a null pointer, count < 0, a fraction not in (0, infinity), no
// positive finite entry.
inline int variance_floor(const float* v, int64_t count, double fraction, float* floor)
{
    if (!v || !floor || count < 0) return INVALID_ARGUMENT;
    if (!(fraction > 0.0) || !std::isfinite(fraction)) return INVALID_ARGUMENT;
    std::vector<float> positive;
    for (int64_t k = 0; k < count; ++k)
        if (v[k] > 0.0f && std::isfinite(v[k])) positive.push_back(v[k]);
    if (positive.empty()) return INVALID_ARGUMENT;
    const size_t h = positive.size() / 2;
    std::nth_element(positive.begin(), positive.begin() + h, positive.end());
    double median = (double)positive[h];
    if (!(positive.size() & 1)) median = ((double)*std::max_element(positive.begin(), positive.begin() + h) + median) / 2.0;
    *floor = (float)(fraction * median);
    return OK;
}

}  // namespace ecc_variance_host

#endif
