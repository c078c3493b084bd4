// ecc_histogram_host.h -- the host half of the residual histograms (include/ecc_hip.h: ecc_host_histogram_quantile), as a plain
// header without HIP includes so that tests/c/histogram_host.cpp builds it alone, under the sanitizers.
#ifndef ECC_HISTOGRAM_HOST_H
#define ECC_HISTOGRAM_HOST_H

#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <limits>

namespace ecc_histogram_host {

// The q-quantile of the binned quantity from one row of counts (or the caller's sum of rows): bin k holds [k width, (k + 1) width),
// the last bin everything from (n_bins - 1) width up.  The crossing of the cumulative count with q x total, linearly interpolated
// inside its bin; +infinity when it lies in the overflow bin (the caller widens); 0.0 for an empty row (or a null pointer or
// n_bins < 1); NaN for q outside [0, 1] (or NaN), for a width that is not finite and > 0.  The total is added in float64: exact
// below 2^53 samples.
inline double histogram_quantile(const uint64_t* counts, int n_bins, double width, double q)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (!(q >= 0.0 && q <= 1.0) || !(width > 0.0) || !std::isfinite(width)) return nan;
    if (!counts || n_bins < 1) return 0.0;
    double total = 0.0;
    for (int k = 0; k < n_bins; ++k) total += (double)counts[k];
    if (total == 0.0) return 0.0;
    const double target = q * total;
    double below = 0.0;  // the samples of the bins in front of k
    for (int k = 0; k < n_bins; ++k) {
        const double c = (double)counts[k];
        if (c > 0.0 && below + c >= target) {
            if (k == n_bins - 1) return std::numeric_limits<double>::infinity();
            return ((double)k + (target - below) / c) * width;
        }
        below += c;
    }
    return std::numeric_limits<double>::infinity();  // (rounding of q x total above the total: the last bin's case)
}

}  // namespace ecc_histogram_host

#endif
