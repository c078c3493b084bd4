// ecc_variance_robust_host.h -- the host half of the variance-robust form (include/ecc_hip.h: ecc_host_variance_robust_scale), as a
// plain header without HIP includes so that tests/c/variance_robust_host.cpp builds it alone, under the sanitizers.
#ifndef ECC_VARIANCE_ROBUST_HOST_H
#define ECC_VARIANCE_ROBUST_HOST_H

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace ecc_variance_robust_host {

// k x the median of sqrt((double)r_q) over the rows {c, u, k, r} (4 floats each) with r_q > 0; an even number of them: the mean of
// the two middle values; no such row (or a null pointer, or n_pairs <= 0): 0.0.  r_q is the pair's mean squared studentised
// residual, so the figure is what "one sigma" measures on the data: V is the line variance only up to a constant factor.
inline double variance_robust_scale(const float* pair_terms, int64_t n_pairs, double k)
{
    std::vector<double> rms;
    if (pair_terms)
        for (int64_t q = 0; q < n_pairs; ++q) {
            const float r = pair_terms[(size_t)q * 4 + 3];
            if (r > 0.f) rms.push_back(std::sqrt((double)r));
        }
    if (rms.empty()) return 0.0;
    std::sort(rms.begin(), rms.end());
    const size_t h = rms.size() / 2;
    return k * (rms.size() & 1 ? rms[h] : (rms[h - 1] + rms[h]) / 2.0);
}

}  // namespace ecc_variance_robust_host

#endif
