// The host half of the residual histograms (csrc/ecc_histogram_host.h: the quantile of a row of counts) as a stand-alone program for
// the sanitizers -- no HIP, no device, no library:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I epipolarconsistency_amd/csrc
//       tests/c/histogram_host.cpp -o /tmp/histogram_host && /tmp/histogram_host
// (one command line, from the repository's root) prints "histogram host ok" and exits with 0; any other exit code names the failed
// check.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "ecc_histogram_host.h"

using ecc_histogram_host::histogram_quantile;

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // four bins of width 0.5, the last one the overflow bin: 10 samples in [0, 0.5), 30 in [0.5, 1), 40 in [1, 1.5), 20 beyond
    const std::vector<uint64_t> row = {10, 30, 40, 20};
    if (histogram_quantile(row.data(), 4, 0.5, 0.0) != 0.0) return 1;             // the lower edge of the first occupied bin
    if (histogram_quantile(row.data(), 4, 0.5, 0.05) != 0.25) return 1;           // half way through bin 0
    if (histogram_quantile(row.data(), 4, 0.5, 0.1) != 0.5) return 1;             // the crossing at an edge belongs to the bin below it
    if (histogram_quantile(row.data(), 4, 0.5, 0.25) != 0.75) return 1;           // 15 of the 30 samples of bin 1
    if (histogram_quantile(row.data(), 4, 0.5, 0.5) != 1.125) return 1;           // 10 of the 40 samples of bin 2
    if (histogram_quantile(row.data(), 4, 0.5, 0.8) != 1.5) return 1;             // the last edge itself
    if (histogram_quantile(row.data(), 4, 0.5, 0.81) != inf) return 2;            // in the overflow bin: the caller widens
    if (histogram_quantile(row.data(), 4, 0.5, 1.0) != inf) return 2;
    // the width scales the answer and nothing else
    if (histogram_quantile(row.data(), 4, 2.0, 0.5) != 4.5) return 3;
    // empty bins in front of and between the occupied ones; q = 0 is the lower edge of the first occupied bin
    const std::vector<uint64_t> gaps = {0, 0, 8, 0, 0, 8, 0, 0};
    if (histogram_quantile(gaps.data(), 8, 1.0, 0.0) != 2.0) return 4;
    if (histogram_quantile(gaps.data(), 8, 1.0, 0.25) != 2.5) return 4;
    if (histogram_quantile(gaps.data(), 8, 1.0, 0.5) != 3.0) return 4;            // the upper edge of bin 2, not somewhere in the gap
    if (histogram_quantile(gaps.data(), 8, 1.0, 0.75) != 5.5) return 4;
    if (histogram_quantile(gaps.data(), 8, 1.0, 1.0) != 6.0) return 4;
    // everything in the overflow bin; one bin only (it IS the overflow bin)
    const std::vector<uint64_t> over = {0, 0, 0, 5};
    if (histogram_quantile(over.data(), 4, 1.0, 0.0) != inf || histogram_quantile(over.data(), 4, 1.0, 0.5) != inf) return 5;
    const uint64_t single[1] = {3};
    if (histogram_quantile(single, 1, 1.0, 0.5) != inf) return 5;
    // an empty row, a null pointer, no bins: 0.0, and nothing is read
    const std::vector<uint64_t> none(64, 0);
    if (histogram_quantile(none.data(), 64, 1.0, 0.5) != 0.0) return 6;
    if (histogram_quantile(nullptr, 64, 1.0, 0.5) != 0.0 || histogram_quantile(row.data(), 0, 1.0, 0.5) != 0.0) return 6;
    if (histogram_quantile(row.data(), -4, 1.0, 0.5) != 0.0) return 6;
    // q outside [0, 1] or NaN, a width that is not finite and > 0: NaN, before anything is read
    const double bad_q[] = {-1e-9, 1.0 + 1e-9, -inf, inf, nan};
    for (double q : bad_q)
        if (!std::isnan(histogram_quantile(row.data(), 4, 0.5, q)) || !std::isnan(histogram_quantile(nullptr, 4, 0.5, q))) return 7;
    const double bad_w[] = {0.0, -1.0, inf, nan};
    for (double w : bad_w)
        if (!std::isnan(histogram_quantile(row.data(), 4, w, 0.5))) return 7;
    // counts beyond 2^32 (a sum of rows of a large scan): the total and the target are float64, exact below 2^53
    const uint64_t big = (uint64_t)1 << 40;
    const std::vector<uint64_t> large = {big, 3 * big, 0, 0};
    if (histogram_quantile(large.data(), 4, 1.0, 0.25) != 1.0 || histogram_quantile(large.data(), 4, 1.0, 0.625) != 1.5) return 8;
    // a full-size row: 1024 bins of one sample each, the median is the edge between bins 511 and 512
    const std::vector<uint64_t> flat(1024, 1);
    if (histogram_quantile(flat.data(), 1024, 0.125, 0.5) != 64.0) return 9;
    if (histogram_quantile(flat.data(), 1024, 0.125, 1023.0 / 1024.0) != 1023 * 0.125) return 9;
    std::printf("histogram host ok\n");
    return 0;
}
