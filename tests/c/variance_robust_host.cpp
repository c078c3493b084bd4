// The host half of the variance-robust form (csrc/ecc_variance_robust_host.h: the scale from the pair rows) as a stand-alone program
// for the sanitizers -- no HIP, no device, no library:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I epipolarconsistency_amd/csrc
//       tests/c/variance_robust_host.cpp -o /tmp/variance_robust_host && /tmp/variance_robust_host
// (one command line, from the repository's root) prints "variance robust host ok" and exits with 0; any other exit code names the
// failed check.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "ecc_variance_robust_host.h"

using ecc_variance_robust_host::variance_robust_scale;

namespace {

// rows {c, u, k, r} whose last column is rs
std::vector<float> rows_of(const std::vector<float>& rs)
{
    std::vector<float> rows;
    for (float r : rs) {
        rows.push_back(0.5f), rows.push_back(1.0f), rows.push_back(1.0f), rows.push_back(r);
    }
    return rows;
}

}  // namespace

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // odd and even counts of live rows among rows with r == 0, r < 0 and r NaN, which do not count
    const std::vector<float> odd = rows_of({4.0f, 0.0f, 16.0f, -1.0f, 9.0f, nan});
    if (variance_robust_scale(odd.data(), 6, 1.0) != 3.0) return 1;
    if (variance_robust_scale(odd.data(), 6, 2.0) != 6.0) return 1;
    const std::vector<float> even = rows_of({25.0f, 1.0f, 0.0f, 4.0f, 9.0f});
    if (variance_robust_scale(even.data(), 5, 1.0) != 2.5) return 2;
    if (variance_robust_scale(even.data(), 1, 0.5) != 2.5) return 2;   // one live row: itself
    // the root and the mean of the two middle values are float64: no overflow next to FLT_MAX, an infinite r stays infinite
    const float big = std::numeric_limits<float>::max();
    const std::vector<float> huge = rows_of({big, big});
    if (variance_robust_scale(huge.data(), 2, 1.0) != std::sqrt((double)big)) return 3;
    const std::vector<float> with_inf = rows_of({1.0f, inf, 4.0f});
    if (variance_robust_scale(with_inf.data(), 3, 1.0) != 2.0) return 3;
    // a long list: r = q^2 for q = 1 .. 100001 in a scrambled order, the median root is 50001 (q^2 < 2^34 is not exact in float32:
    // compare with the root of the rounded square)
    std::vector<float> rs(100001);
    for (size_t q = 0; q < rs.size(); ++q) {
        const double v = (double)((q * 7919u) % rs.size() + 1);
        rs[q] = (float)(v * v);
    }
    const std::vector<float> ramp = rows_of(rs);
    if (variance_robust_scale(ramp.data(), (int64_t)rs.size(), 1.0) != std::sqrt((double)(float)(50001.0 * 50001.0))) return 4;
    // no live row, no rows, a null pointer, a negative count: 0.0, and nothing is read
    const std::vector<float> none = rows_of({0.0f, -4.0f, nan});
    if (variance_robust_scale(none.data(), 3, 1.0) != 0.0) return 5;
    if (variance_robust_scale(even.data(), 0, 1.0) != 0.0 || variance_robust_scale(even.data(), -3, 1.0) != 0.0) return 6;
    if (variance_robust_scale(nullptr, 5, 1.0) != 0.0) return 6;
    std::printf("variance robust host ok\n");
    return 0;
}
