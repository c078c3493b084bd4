// Driver for the host-only part of MetricDirect's index lists and pose batches (epipolarconsistency_amd/csrc/
// ecc_direct_lists_host.h), CPU only.
//   (a) pose_pairs against a brute-force enumeration: every subset of the views of n = 1 .. 7 as the moved set, in a shuffled
//       order: the same pairs in ascending (i, j) order, each once, the slots of the candidates, the scratch left clean, and
//       the count pose_pairs_count promises;
//   (b) check_poses: the bound over a batch, and every refusal with its text (a view twice, out of range, offsets, 2^20);
//   (c) check_idx4 and check_offsets: accepted lists, and every refusal naming its entry.
// Built by tests/test_direct_pose_pairs.py with -Wall -Wextra -Werror and by scripts/sanitize.sh under
// -fsanitize=address,undefined.
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../../epipolarconsistency_amd/csrc/ecc_direct_lists_host.h"

namespace lists = ecc_direct_lists;

namespace {

int failures = 0;
void check(bool ok, const char* what, long long a = 0, long long b = 0)
{
    if (ok) return;
    if (++failures <= 20) std::printf("FAIL %s (%lld, %lld)\n", what, a, b);
}
bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

struct Tuple {
    int i, j, si, sj;
};

void pose_pairs_cases()
{
    std::mt19937 rng(4711);
    for (int n = 1; n <= 7; ++n) {
        std::vector<int> slot((size_t)n, -1), sorted;
        for (unsigned mask = 0; mask < (1u << n); ++mask) {
            std::vector<int32_t> views;
            for (int v = 0; v < n; ++v)
                if (mask >> v & 1) views.push_back(v);
            std::shuffle(views.begin(), views.end(), rng);
            std::vector<Tuple> got;
            const int64_t count = lists::pose_pairs(n, views.data(), (int)views.size(), slot, sorted,
                                                    [&](int i, int j, int si, int sj) { got.push_back(Tuple{i, j, si, sj}); });
            check(count == (int64_t)got.size() && count == lists::pose_pairs_count(n, (int64_t)views.size()), "count", n, mask);
            size_t at = 0;
            for (int i = 0; i < n; ++i)
                for (int j = i + 1; j < n; ++j) {
                    if (!(mask >> i & 1) && !(mask >> j & 1)) continue;
                    if (at >= got.size()) {
                        check(false, "too few pairs", n, mask);
                        continue;
                    }
                    const Tuple& t = got[at++];
                    check(t.i == i && t.j == j, "order", n, mask);
                    check((t.si >= 0) == (bool)(mask >> i & 1) && (t.sj >= 0) == (bool)(mask >> j & 1), "slot sign", n, mask);
                    check(t.si < 0 || views[(size_t)t.si] == i, "slot of i", n, mask);
                    check(t.sj < 0 || views[(size_t)t.sj] == j, "slot of j", n, mask);
                }
            check(at == got.size(), "too many pairs", n, mask);
            for (int v = 0; v < n; ++v) check(slot[(size_t)v] == -1, "scratch left dirty", n, mask);
        }
    }
}

void check_poses_cases()
{
    int64_t pairs = -1;
    const int32_t off[] = {0, 1, 3, 3, 4};
    const int32_t views[] = {3, 6, 2, 0};
    check(lists::check_poses(4, off, views, 8, &pairs).empty() && pairs == 7 + 13 + 0 + 7, "bound of a batch", pairs);
    pairs = -1;
    check(lists::check_poses(4, off, nullptr, 8, &pairs).empty() && pairs == 27, "bound without the views", pairs);
    const int32_t twice[] = {3, 2, 2, 0};
    check(has(lists::check_poses(4, off, twice, 8, &pairs), "pose 1 names view 2 twice"), "a view twice");
    const int32_t again[] = {3, 3, 2, 3};  // the same view in different poses is fine
    check(lists::check_poses(4, off, again, 8, &pairs).empty(), "the same view in two poses");
    const int32_t high[] = {3, 6, 8, 0}, low[] = {-1, 6, 2, 0};
    check(has(lists::check_poses(4, off, high, 8, &pairs), "pose 1: view index 8 out of range [0, 8)"), "view too high");
    check(has(lists::check_poses(4, off, low, 8, &pairs), "pose 0: view index -1 out of range"), "view negative");
    const int32_t down[] = {0, 2, 1, 3, 4}, late[] = {1, 2, 3, 3, 4};
    check(has(lists::check_poses(4, down, views, 8, &pairs), "pose offsets decrease at entry 2 (2 -> 1)"), "offsets decrease");
    check(has(lists::check_poses(4, late, views, 8, &pairs), "pose offsets do not start at 0 (1)"), "offsets start");
    const int32_t many[] = {0, 4};
    check(has(lists::check_poses(1, many, nullptr, 3, &pairs), "pose 0 moves 4 views of 3"), "more views than images");
    // 2^20: 149 797 poses of one view of 8 are 1 048 579 pairs
    std::vector<int32_t> offs(149798), vs(149797, 5);
    for (size_t k = 0; k < offs.size(); ++k) offs[k] = (int32_t)k;
    check(has(lists::check_poses(149797, offs.data(), vs.data(), 8, &pairs), "more than 2^20 pairs"), "2^20 over a batch");
    check(lists::check_poses(149796, offs.data(), vs.data(), 8, &pairs).empty() && pairs == 149796 * 7, "just below 2^20", pairs);
}

void check_lists_cases()
{
    const int32_t good[] = {0, 1, 0, 1, 9, 2, 3, 2, 2, 0, 7, 7};  // (an image may be paired with itself; a matrix may not)
    check(lists::check_idx4(good, 3, 10, 8).empty(), "a good list");
    check(lists::check_idx4(nullptr, 0, 10, 8).empty(), "an empty list");
    struct Case {
        int32_t t[4];
        const char* text;
    };
    const Case bad[] = {{{10, 1, 0, 1}, "entry 2: matrix index 10 out of range [0, 10)"}, {{0, -1, 0, 1}, "entry 2: matrix index -1"},
                        {{0, 1, 8, 1}, "entry 2: image index 8 out of range [0, 8)"}, {{0, 1, 0, -3}, "entry 2: image index -3"},
                        {{4, 4, 0, 1}, "entry 2: P0 == P1 (4)"}};
    for (const Case& c : bad) {
        int32_t list[12];
        for (int k = 0; k < 8; ++k) list[k] = good[k];
        for (int k = 0; k < 4; ++k) list[8 + k] = c.t[k];
        check(has(lists::check_idx4(list, 3, 10, 8), c.text), c.text);
    }
    check(has(lists::check_idx4(good, lists::MAX_PAIRS + 1, 10, 8), "more than 2^20 pairs"), "2^20 in a list");  // (before any entry is read)
    const int64_t fine[] = {0, 0, 2, 3, 3}, down[] = {0, 2, 1, 3}, shortof[] = {0, 1, 2}, late[] = {1, 3};
    check(lists::check_offsets(fine, 4, 3, "segment").empty(), "good offsets");
    check(has(lists::check_offsets(down, 3, 3, "segment"), "segment offsets decrease at entry 2 (2 -> 1)"), "segments decrease");
    check(has(lists::check_offsets(shortof, 2, 3, "segment"), "segment offsets end at 2, not at the list length 3"), "segments end");
    check(has(lists::check_offsets(late, 1, 3, "segment"), "segment offsets do not start at 0 (1)"), "segments start");
}

}  // namespace

int main()
{
    pose_pairs_cases();
    check_poses_cases();
    check_lists_cases();
    if (failures) {
        std::printf("direct_lists_host: %d failures\n", failures);
        return 1;
    }
    std::printf("direct_lists_host ok\n");
    return 0;
}
