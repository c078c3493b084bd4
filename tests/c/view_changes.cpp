// Driver for the host-side change scan and pair-list builder of the metric's evaluation paths
// (epipolarconsistency_amd/csrc/ecc_view_changes.h), CPU only.  For n from 2 to 600 views (513 and 600: beyond the 512-view skip
// mask), full ranges, shard ranges and empty ranges, and 0, 1, 2 and n/4 changed views (views 0 and n - 1, adjacent views):
//   changed_views   finds exactly the views whose 12 doubles differ bitwise (-0.0 against 0.0 included), and stops after
//                   stop_after + 1 of them;
//   pairs_of_views  lists every pair of the range that contains a changed view once, with its slot, against brute-force
//                   enumeration, in the order of the loop the evaluation paths used before (a verbatim copy below).
// Optional argument: a file of further "n first count" lines (tests/test_abi_and_host.py writes the shards sharding.pair_range
// cuts).  Built by tests/test_abi_and_host.py with -Wall -Werror and by scripts/sanitize.sh under -fsanitize=address,undefined.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

#include "../../epipolarconsistency_amd/csrc/ecc_view_changes.h"

using ecc_view_changes::PairList;

namespace {

int failures = 0;
void check(bool ok, const char* what, int64_t n, int64_t first, int64_t count, size_t c)
{
    if (ok) return;
    if (++failures <= 20)
        std::printf("FAIL %s: n=%lld first=%lld count=%lld changed=%zu\n", what, (long long)n, (long long)first, (long long)count, c);
}

// The pair-list loop of launch_range / evaluate_cached before it moved into ecc_view_changes.h, verbatim.
void old_loop(int64_t n, int64_t first, int64_t count, const std::vector<int>& changed, std::vector<int32_t>& idx,
              std::vector<int32_t>& slots)
{
    std::vector<char> is_changed;
    is_changed.assign((size_t)n, 0);
    for (int v : changed) is_changed[v] = 1;
    idx.clear();
    slots.clear();
    for (int v : changed)
        for (int64_t u = 0; u < n; ++u) {
            if (u == v || (is_changed[u] && u < v)) continue;  // a pair of two changed views once
            const int64_t i = u < v ? u : v, j = u < v ? v : u;
            const int64_t ij = i * n - i * (i + 1) / 2 + (j - i - 1);  // get_ij order
            if (ij < first || ij >= first + count) continue;
            idx.insert(idx.end(), {(int32_t)i, (int32_t)j, (int32_t)i, (int32_t)j});
            slots.push_back((int32_t)(ij - first));
        }
}

void check_pairs(int64_t n, int64_t first, int64_t count, const std::vector<int>& changed, PairList* list)
{
    ecc_view_changes::pairs_of_views(n, first, count, changed, list);
    std::vector<int32_t> idx, slots;
    old_loop(n, first, count, changed, idx, slots);
    check(list->idx == idx && list->slots == slots, "order differs from the old loop", n, first, count, changed.size());
    // brute force: every pair {i < j} in get_ij order, in the range, with a changed view
    std::vector<char> is_changed((size_t)n, 0);
    for (int v : changed) is_changed[v] = 1;
    std::set<std::pair<int32_t, int32_t>> want;
    int64_t ij = 0;
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = i + 1; j < n; ++j, ++ij)
            if (ij >= first && ij < first + count && (is_changed[i] || is_changed[j])) want.insert({(int32_t)i, (int32_t)j});
    const size_t L = list->slots.size();
    bool ok = list->idx.size() == 4 * L && L == want.size();
    std::set<std::pair<int32_t, int32_t>> got;
    for (size_t q = 0; ok && q < L; ++q) {
        const int32_t* t = &list->idx[4 * q];
        const int64_t i = t[0], j = t[1];
        ok = i < j && t[2] == i && t[3] == j && got.insert({t[0], t[1]}).second &&
             list->slots[q] == i * n - i * (i + 1) / 2 + (j - i - 1) - first;
    }
    check(ok && got == want, "pairs differ from brute force", n, first, count, changed.size());
}

void check_scan(int64_t n, const std::vector<int>& changed, unsigned long long* state)
{
    std::vector<double> snap(12 * (size_t)n), cur;
    for (size_t k = 0; k < snap.size(); ++k) snap[k] = (double)(k % 97) - 48.0;  // zeros included
    cur = snap;
    for (int v : changed) {
        *state ^= *state << 13;
        *state ^= *state >> 7;
        *state ^= *state << 17;
        double& x = cur[12 * (size_t)v + *state % 12];
        x = x == 0.0 ? -0.0 : std::nextafter(x, 1e300);  // a difference in the bits only (-0.0 == 0.0), or the last bit
    }
    std::vector<int> out;
    ecc_view_changes::changed_views(cur.data(), snap.data(), n, &out);
    check(out == changed, "changed_views", n, 0, 0, changed.size());
    for (int64_t stop : {0, 1, 2, 16}) {
        ecc_view_changes::changed_views(cur.data(), snap.data(), n, &out, stop);
        const std::vector<int> want(changed.begin(), changed.begin() + std::min<int64_t>((int64_t)changed.size(), stop + 1));
        check(out == want, "changed_views stop_after", n, stop, 0, changed.size());
    }
}

}  // namespace

int main(int argc, char** argv)
{
    unsigned long long state = 88172645463325252ull;
    auto rnd = [&]() {
        state ^= state << 13;
        state ^= state >> 7;
        state ^= state << 17;
        return state;
    };
    std::vector<std::vector<int64_t>> extra;  // further ranges: n, first, count
    if (argc > 1) {
        FILE* f = std::fopen(argv[1], "r");
        if (!f) return std::printf("cannot open %s\n", argv[1]), 1;
        long long a, b, c;
        while (std::fscanf(f, "%lld %lld %lld", &a, &b, &c) == 3) extra.push_back({a, b, c});
        std::fclose(f);
    }
    PairList list;  // reused across calls, as the metric reuses its own
    int64_t lists = 0;
    for (int64_t n : {2, 3, 4, 5, 7, 8, 9, 31, 64, 100, 257, 512, 513, 600}) {
        const int64_t P = n * (n - 1) / 2;
        std::vector<std::pair<int64_t, int64_t>> ranges = {{0, P}, {0, 0}, {P / 2, 0}, {P, 0}};
        for (int64_t world : {2, 3, 8})
            for (int64_t r = 0; r < world; ++r) {  // sharding.pair_range
                const int64_t first = r * P / world;
                ranges.push_back({first, (r + 1) * P / world - first});
            }
        for (const auto& e : extra)
            if (e[0] == n) ranges.push_back({e[1], e[2]});
        std::vector<std::vector<int>> sets = {{}, {0}, {(int)n - 1}, {(int)(n / 2)}, {0, (int)n - 1}};
        if (n >= 3) sets.push_back({(int)(n / 3), (int)(n / 3) + 1});  // adjacent views
        std::vector<int> quarter;
        for (int64_t v = 0; v < n; ++v) quarter.push_back((int)v);
        for (int64_t k = n - 1; k > 0; --k) std::swap(quarter[k], quarter[rnd() % (k + 1)]);
        quarter.resize((size_t)(n / 4));
        std::sort(quarter.begin(), quarter.end());
        sets.push_back(quarter);
        for (const auto& changed : sets) {
            check_scan(n, changed, &state);
            for (const auto& r : ranges) {
                check_pairs(n, r.first, r.second, changed, &list);
                ++lists;
            }
        }
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok: %lld pair lists, %zu extra ranges\n", (long long)lists, extra.size());
    return 0;
}
