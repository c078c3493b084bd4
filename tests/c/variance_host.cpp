// The host half of the variance form (csrc/ecc_variance_host.h: the floor from the fields) as a stand-alone program for the
// sanitizers -- no HIP, no device, no library:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I epipolarconsistency_amd/csrc
//       tests/c/variance_host.cpp -o /tmp/variance_host && /tmp/variance_host
// (one command line, from the repository's root) prints "variance host ok" and exits with 0; any other exit code names the failed check.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "ecc_variance_host.h"

using ecc_variance_host::INVALID_ARGUMENT;
using ecc_variance_host::OK;
using ecc_variance_host::variance_floor;

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    float f = -1.0f;
    // odd and even counts of positive entries, among zeros, negatives and non-finite entries that do not count
    const std::vector<float> odd = {0.0f, 5.0f, -2.0f, 1.0f, inf, 3.0f, nan, -inf};
    if (variance_floor(odd.data(), (int64_t)odd.size(), 1.0, &f) != OK || f != 3.0f) return 1;
    const std::vector<float> even = {8.0f, 0.0f, 1.0f, 4.0f, 2.0f};
    if (variance_floor(even.data(), (int64_t)even.size(), 0.5, &f) != OK || f != 1.5f) return 2;
    if (variance_floor(even.data(), 1, 1e-3, &f) != OK || f != (float)(1e-3 * 8.0)) return 3;
    // the two middle values are added in float64: no overflow next to FLT_MAX
    const float big = std::numeric_limits<float>::max();
    const std::vector<float> huge = {big, big};
    if (variance_floor(huge.data(), 2, 0.25, &f) != OK || f != (float)(0.25 * (double)big)) return 4;
    // a long field: the median of 1 .. 100001 is 50001
    std::vector<float> ramp(100001);
    for (size_t k = 0; k < ramp.size(); ++k) ramp[k] = (float)((k * 7919u) % ramp.size() + 1);
    if (variance_floor(ramp.data(), (int64_t)ramp.size(), 1.0, &f) != OK || f != 50001.0f) return 5;
    // refusals write nothing
    f = -1.0f;
    const std::vector<float> none = {0.0f, -1.0f, nan, inf};
    if (variance_floor(none.data(), (int64_t)none.size(), 1.0, &f) != INVALID_ARGUMENT) return 6;
    if (variance_floor(even.data(), 0, 1.0, &f) != INVALID_ARGUMENT) return 6;
    if (variance_floor(nullptr, 3, 1.0, &f) != INVALID_ARGUMENT || variance_floor(even.data(), 3, 1.0, nullptr) != INVALID_ARGUMENT) return 7;
    if (variance_floor(even.data(), -1, 1.0, &f) != INVALID_ARGUMENT) return 7;
    for (double bad : {0.0, -1.0, (double)inf, (double)nan})
        if (variance_floor(even.data(), 3, bad, &f) != INVALID_ARGUMENT) return 8;
    if (f != -1.0f) return 9;
    std::printf("variance host ok\n");
    return 0;
}
