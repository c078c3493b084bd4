// Driver for the grid -> all-pairs mapping of a pose batch (epipolarconsistency_amd/csrc/ecc_pose_scatter.h), CPU only.
//   (a) n = 2 .. 40, moved sets of 0, 1, 2, 4 and n views (adjacent views, view 0 and view n - 1 among them): the non-hole entries of
//       a pose hit exactly the get_ij positions of the pairs that contain a moved view, each such pair once, and the pair of two moved
//       views is taken from the column pose_list_kernel evaluates it in (the lower view's; the entry in the other column is a hole);
//   (b) the segmented sums' staging, emulated thread by thread with this file's own loops -- slices, chunks of STAGE_F4 float4 copied
//       from a random base column, the pose's entries put over them at position(), the tail in its own four slots, 1024 lane
//       accumulators that run across the chunks, the shuffle-down tree, wave sums and slice sums in order -- gives the bits of
//       ecc_sum::sum_on_host over the substituted array: counts with and without a tail, below and above SPLIT_MIN_COUNT, a slice
//       longer than one chunk in both forms.
// Built by tests/test_weighted_poses_abi.py with -Wall -Werror.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../epipolarconsistency_amd/csrc/ecc_pose_scatter.h"

namespace {

int failures = 0;
void check(bool ok, const char* what, int n, int c)
{
    if (ok) return;
    if (++failures <= 20) std::printf("FAIL %s: n=%d moved=%d\n", what, n, c);
}

// the pair order of ecc_get_ij, by enumeration: index[i][j], i < j
std::vector<std::vector<long long>> pair_index(int n)
{
    std::vector<std::vector<long long>> idx(n, std::vector<long long>(n, -1));
    long long q = 0;
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) idx[i][j] = q++;
    return idx;
}

std::vector<std::vector<int>> moved_sets(int n)
{
    std::vector<std::vector<int>> sets;
    sets.push_back({});
    for (int v : {0, n - 1, n / 2}) sets.push_back({v});
    if (n >= 2) {
        sets.push_back({0, 1});
        sets.push_back({0, n - 1});
        sets.push_back({n - 2, n - 1});
        if (n >= 4) sets.push_back({n / 2 - 1, n / 2});
        if (n >= 5) sets.push_back({1, n - 2});
    }
    if (n >= 4) {
        sets.push_back({0, 1, n - 2, n - 1});
        sets.push_back({0, 1, 2, 3});
        if (n >= 9) sets.push_back({1, n / 3, n / 2, n - 1});
    }
    std::vector<int> all(n);
    for (int v = 0; v < n; ++v) all[v] = v;
    sets.push_back(all);
    for (auto& s : sets) {
        std::sort(s.begin(), s.end());
        s.erase(std::unique(s.begin(), s.end()), s.end());
    }
    return sets;
}

void check_mapping(int n)
{
    const auto idx = pair_index(n);
    const long long n_pairs = (long long)n * (n - 1) / 2;
    for (const auto& M : moved_sets(n)) {
        const int c = (int)M.size();
        std::vector<int> hits((size_t)n_pairs, 0);
        std::vector<bool> is_moved(n, false);
        for (int v : M) is_moved[v] = true;
        for (int a = 0; a < c; ++a)
            for (int u = 0; u < n; ++u) {
                const long long ij = ecc_pose_scatter::position(u, a, M.data(), n);
                if (ij == ecc_pose_scatter::HOLE) {
                    // a hole is the moved view itself, or a partner that an EARLIER column moves
                    bool earlier = false;
                    for (int b = 0; b < a; ++b) earlier = earlier || M[b] == u;
                    check(u == M[a] || earlier, "a hole that is neither", n, c);
                    continue;
                }
                const int v = M[a], i = std::min(u, v), j = std::max(u, v);
                check(u != v && ij >= 0 && ij < n_pairs, "position out of range", n, c);
                if (u == v || ij < 0 || ij >= n_pairs) continue;
                check(ij == idx[i][j], "not the get_ij position of the pair", n, c);
                ++hits[(size_t)ij];
            }
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j)
                check(hits[(size_t)idx[i][j]] == ((is_moved[i] || is_moved[j]) ? 1 : 0), "pair not hit exactly once / hit without a moved view", n, c);
        // two moved views M[b] < M[a], b < a: pose_list_kernel makes entry (u = M[b], column a) the hole ("u < v when the pose moves u
        // as well: that pair belongs to u's column") and evaluates the pair at entry (u = M[a], column b), with both moved geometries
        for (int a = 0; a < c; ++a)
            for (int b = 0; b < a; ++b) {
                check(ecc_pose_scatter::position(M[a], b, M.data(), n) == idx[M[b]][M[a]], "pair of two moved views not in the column of the lower view", n, c);
                check(ecc_pose_scatter::position(M[b], a, M.data(), n) == ecc_pose_scatter::HOLE, "pair of two moved views in both columns", n, c);
            }
    }
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// Workgroup (slice) of the segmented sum, thread by thread.  vals: entry (u, a) at u * c + a.
double emulate(const std::vector<float>& base, long long count, int slices, int n, const std::vector<int>& M, const std::vector<float>& vals)
{
    const int T = ecc_sum::THREADS, F4 = ecc_pose_scatter::STAGE_F4, c = (int)M.size();
    const long long n4 = count / 4;
    double tot = 0.0;
    for (int slice = 0; slice < slices; ++slice) {
        long long lo, hi;
        ecc_sum::slice_bounds(n4, slices, slice, &lo, &hi);
        const bool owns_tail = slice == slices - 1;
        std::vector<float> stage(4 * (size_t)F4);
        float tail[4] = {0.f, 0.f, 0.f, 0.f};
        if (owns_tail)
            for (int t = 0; t < 4; ++t) tail[t] = 4 * n4 + t < count ? base[(size_t)(4 * n4 + t)] : 0.f;
        std::vector<double> acc(4 * (size_t)T, 0.0);
        bool first_chunk = true;
        for (long long c0 = lo; c0 < hi || first_chunk; c0 += F4) {
            const long long ce = std::min(hi, c0 + F4);
            for (long long k = 4 * c0; k < 4 * ce; ++k) stage[(size_t)(k - 4 * c0)] = base[(size_t)k];
            for (int e = 0; e < c * n; ++e) {
                const int a = e / n, u = e - a * n;
                const long long ij = ecc_pose_scatter::position(u, a, M.data(), n);
                if (ij == ecc_pose_scatter::HOLE) continue;
                if (ij >= 4 * c0 && ij < 4 * ce) stage[(size_t)(ij - 4 * c0)] = vals[(size_t)u * c + a];
                else if (owns_tail && first_chunk && ij >= 4 * n4) tail[ij - 4 * n4] = vals[(size_t)u * c + a];
            }
            for (int t = 0; t < T; ++t)
                for (long long k = c0 + t; k < ce; k += T)
                    for (int q = 0; q < 4; ++q) acc[4 * (size_t)t + q] += (double)stage[(size_t)(4 * (k - c0) + q)];
            first_chunk = false;
        }
        double part = 0.0;
        for (int w = 0; w < T / 64; ++w) {
            double lane[64];
            for (int l = 0; l < 64; ++l) {
                const size_t t = 64 * (size_t)w + l;
                lane[l] = (acc[4 * t] + acc[4 * t + 1]) + (acc[4 * t + 2] + acc[4 * t + 3]);
                if (owns_tail && t == 0)
                    for (long long k = 4 * n4; k < count; ++k) lane[l] += (double)tail[k - 4 * n4];
            }
            for (int off = 32; off > 0; off >>= 1)
                for (int l = 0; l < off; ++l) lane[l] += lane[l + off];
            part += lane[0];
        }
        tot += part;
    }
    return tot;
}

void check_sums(int n, std::mt19937& rng)
{
    const long long count = (long long)n * (n - 1) / 2;
    std::uniform_real_distribution<float> mant(0.5f, 1.0f);
    std::uniform_int_distribution<int> expo(-20, 20), sign(0, 1);
    auto draw = [&]() { return std::ldexp(mant(rng), expo(rng)) * (sign(rng) ? 1.f : -1.f); };
    std::vector<float> base((size_t)count);
    for (auto& v : base) v = draw();
    std::vector<std::vector<int>> sets = {{}, {n - 1}, {n / 2}};
    if (n >= 4) sets.push_back({0, 1, n / 2, n - 1});
    if (n >= 9) sets.push_back({2, 3, n - 2});
    for (const auto& M : sets) {
        const int c = (int)M.size();
        std::vector<float> vals((size_t)n * std::max(c, 1));
        for (auto& v : vals) v = draw();
        std::vector<float> subst(base);
        for (int a = 0; a < c; ++a)
            for (int u = 0; u < n; ++u) {
                const long long ij = ecc_pose_scatter::position(u, a, M.data(), n);
                if (ij != ecc_pose_scatter::HOLE) subst[(size_t)ij] = vals[(size_t)u * c + a];
            }
        for (int slices : {1, ecc_sum::SLICES}) {
            const double want = ecc_sum::sum_on_host(subst.data(), count, slices);
            const double got = emulate(base, count, slices, n, M, vals);
            check(same_bits(want, got), slices == 1 ? "chunked sum, one slice" : "chunked sum, sixteen slices", n, c);
            if (c > 0) check(!same_bits(want, ecc_sum::sum_on_host(base.data(), count, slices)), "the substitution changed nothing", n, c);
        }
    }
}

}  // namespace

int main()
{
    for (int n = 2; n <= 40; ++n) check_mapping(n);
    std::mt19937 rng(20240607u);
    // pairs: 3 (tail only), 36, 2 211 (tail 3), 8 385 (> one chunk of 8 192 in one slice, tail 1), 32 640 (below SPLIT_MIN_COUNT, no
    // tail), 32 896 / 33 153 (above it, without and with a tail), 134 940 (a sixteenth is longer than one chunk)
    const int ns[] = {3, 9, 67, 130, 256, 257, 258, 520};
    for (int n : ns) check_sums(n, rng);
    static_assert(ecc_pose_scatter::STAGE_F4 == 2048, "a chunk is 2 048 float4");
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok: 39 view counts mapped, %d pair counts summed\n", (int)(sizeof(ns) / sizeof(ns[0])));
    return 0;
}
