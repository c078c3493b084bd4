// Driver for the host statement of the pair total's order (epipolarconsistency_amd/csrc/ecc_sum_order.h), CPU only.
//   (a) sum_on_host with one slice against the host sum the one-launch evaluation used before (small_sum_on_host of
//       ecc_evaluate.hip, a verbatim copy below: the witness), bit for bit, every count 0 .. 4096;
//   (b) sum_on_host with 1 and SLICES slices against a deliberately naive emulation of a sum workgroup written here (an array of
//       1024 lane accumulators per slice, an explicit shuffle-down tree), counts around every boundary of the order;
//   (c) slice_bounds cuts [0, n4) into consecutive, non-overlapping slices;
//   (d) slices() switches at SPLIT_MIN_COUNT, and only with the split form's scratch.
// Values: seeded, both signs, magnitudes over ~40 binades, so that a changed order of additions changes the bits.
// Built by tests/test_abi_and_host.py with -Wall -Werror and by scripts/sanitize.sh under -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../epipolarconsistency_amd/csrc/ecc_sum_order.h"

namespace {

int failures = 0;
void check(bool ok, const char* what, long long count, int slices)
{
    if (ok) return;
    if (++failures <= 20) std::printf("FAIL %s: count=%lld slices=%d\n", what, count, slices);
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// small_sum_on_host of ecc_evaluate.hip before the order moved into ecc_sum_order.h, verbatim (counts up to 4096).
double small_sum_on_host(const float* v, int64_t count)
{
    const int64_t n4 = count >> 2;
    double tot = 0.0;
    for (int w = 0; w < 16; ++w) {
        double a[64];
        for (int l = 0; l < 64; ++l) {
            const int64_t t = 64 * w + l;
            double acc = 0.0;
            if (t < n4) {
                const double a0 = 0.0 + (double)v[4 * t], a1 = 0.0 + (double)v[4 * t + 1], a2 = 0.0 + (double)v[4 * t + 2],
                             a3 = 0.0 + (double)v[4 * t + 3];
                acc = (a0 + a1) + (a2 + a3);
            }
            if (t == 0)
                for (int64_t k = n4 << 2; k < count; ++k) acc += (double)v[k];
            a[l] = acc;
        }
        for (int off = 32; off > 0; off >>= 1)
            for (int l = 0; l < off; ++l) a[l] += a[l + off];  // what lane 0 of __shfl_down's tree ends up with
        tot += a[0];
    }
    return tot;
}

// What the sum kernels do, thread by thread, with this file's own literals: slices of ceil(n4 / slices) float4, 1024 threads,
// four accumulators, the tail on thread 0 of the last slice, __shfl_down's tree on every lane (a lane past the wave's end
// keeps its own value), the 16 wave sums and then the slice sums in order.
double naive(const std::vector<float>& v, long long count, int slices)
{
    const long long n4 = count / 4, per = (n4 + slices - 1) / slices;
    std::vector<double> parts;
    for (int s = 0; s < slices; ++s) {
        const long long lo = s * per, hi = std::min(n4, lo + per);
        std::vector<double> lane(1024);
        for (int t = 0; t < 1024; ++t) {
            double a[4] = {0.0, 0.0, 0.0, 0.0};
            for (long long k = lo + t; k < hi; k += 1024)
                for (int c = 0; c < 4; ++c) a[c] += (double)v[(size_t)(4 * k + c)];
            lane[t] = (a[0] + a[1]) + (a[2] + a[3]);
        }
        if (s == slices - 1)
            for (long long k = 4 * n4; k < count; ++k) lane[0] += (double)v[(size_t)k];
        double part = 0.0;
        for (int w = 0; w < 16; ++w) {
            double* x = &lane[64 * w];
            for (int off = 32; off > 0; off /= 2) {
                double shifted[64];
                for (int l = 0; l < 64; ++l) shifted[l] = l + off < 64 ? x[l + off] : x[l];
                for (int l = 0; l < 64; ++l) x[l] += shifted[l];
            }
            part += x[0];
        }
        parts.push_back(part);
    }
    if (slices == 1) return parts[0];
    double tot = 0.0;
    for (double p : parts) tot += p;
    return tot;
}

}  // namespace

int main()
{
    const long long max_count = 79800 + 8;
    std::mt19937_64 rnd(20240607);
    std::vector<float> v((size_t)max_count);
    for (auto& x : v) {
        const double mant = 1.0 + (double)(rnd() >> 11) / 9007199254740992.0;
        x = (float)std::ldexp((rnd() & 1) ? mant : -mant, (int)(rnd() % 40) - 30);
    }
    // (a)
    for (long long count = 0; count <= 4096; ++count)
        check(same_bits(ecc_sum::sum_on_host(v.data(), count, 1), small_sum_on_host(v.data(), count)), "old host sum", count, 1);
    // (b)
    std::vector<long long> counts = {0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 32767, 32768, 32769, 79799, 79800, 79801};
    for (long long base : {4096LL, 8192LL, 4LL * 16, 4LL * 1024, 4LL * 1024 * 16, 4LL * 1024 * 16 + 4 * 16, 40LL * 1024, 32LL * 1024})
        for (long long d = -5; d <= 5; ++d)
            if (base + d >= 0) counts.push_back(base + d);
    long long sums = 0;
    for (long long count : counts)
        for (int slices : {1, 16}) {
            check(same_bits(ecc_sum::sum_on_host(v.data(), count, slices), naive(v, count, slices)), "naive emulation", count, slices);
            ++sums;
        }
    // (c)
    for (long long n4 = 0; n4 <= 20000; n4 += (n4 < 100 ? 1 : 37))
        for (int slices : {1, 16}) {
            long long end = 0;
            bool ok = true;
            for (int s = 0; s < slices; ++s) {
                long long lo, hi;
                ecc_sum::slice_bounds(n4, slices, s, &lo, &hi);
                if (lo < hi) {  // (a slice past the end is empty: lo >= hi)
                    ok = ok && lo == end;
                    end = hi;
                }
            }
            check(ok && end == n4, "slice bounds", 4 * n4, slices);
        }
    // (d)
    static_assert(ecc_sum::THREADS == 1024 && ecc_sum::SLICES == 16 && ecc_sum::SPLIT_MIN_COUNT == 32768, "the naive emulation's literals");
    check(ecc_sum::slices(32767, true) == 1 && ecc_sum::slices(32768, true) == 16, "slices", 32768, 16);
    check(ecc_sum::slices(32768, false) == 1 && ecc_sum::slices(79800, false) == 1, "slices without scratch", 32768, 1);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok: 4097 counts against the old host sum, %lld sums against the naive emulation\n", sums);
    return 0;
}
