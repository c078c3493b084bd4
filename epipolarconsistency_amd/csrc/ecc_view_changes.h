// ecc_view_changes.h -- which views of the current matrices differ from a kept set, and which pairs of a pair range contain
// such a view (host only, no HIP: compiled by tests/c/view_changes.cpp as well as by ecc_evaluate.hip).
//
// The evaluation paths that keep something between calls -- the per-pair records (record reuse), the pair values (the
// pose-delta mode), the device geometry, the one-launch path's patches -- redo only what belongs to the views whose 12 doubles
// changed BITWISE since, and the pairs of the range that contain one of them.
#ifndef ECC_VIEW_CHANGES_H
#define ECC_VIEW_CHANGES_H

#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

namespace ecc_view_changes {

// The views v of [0, n) whose 12 doubles in cur and snap differ bitwise, ascending, into *out.  The scan stops once *out holds
// more than stop_after views (a caller that takes at most stop_after of them learns "too many" from the size).
inline void changed_views(const double* cur, const double* snap, int64_t n, std::vector<int>* out,
                          int64_t stop_after = std::numeric_limits<int64_t>::max())
{
    out->clear();
    for (int64_t v = 0; v < n && (int64_t)out->size() <= stop_after; ++v)
        if (std::memcmp(cur + 12 * v, snap + 12 * v, sizeof(double) * 12) != 0) out->push_back((int)v);
}

struct PairList {
    std::vector<int32_t> idx;      // 4 per pair: i, j, i, j (matrices, then Radon intermediates; i < j)
    std::vector<int32_t> slots;    // per pair: its position in the range, ij - first
    std::vector<char> is_changed;  // scratch: per view, whether it is in `changed`
};

// The pairs {i, j} of [first, first + count) in get_ij order (ij = i n - i (i + 1) / 2 + j - i - 1) that contain a view of
// `changed` (ascending): per changed view v its partners u in ascending order, a pair of two changed views once (under the
// smaller of the two, i.e. skipped from the larger one).  The vectors of *out keep their capacity between calls.
inline void pairs_of_views(int64_t n, int64_t first, int64_t count, const std::vector<int>& changed, PairList* out)
{
    std::vector<char>& is_changed = out->is_changed;
    is_changed.assign((size_t)n, 0);
    for (int v : changed) is_changed[v] = 1;
    out->idx.clear();
    out->slots.clear();
    for (int v : changed)
        for (int64_t u = 0; u < n; ++u) {
            if (u == v || (is_changed[u] && u < v)) continue;  // a pair of two changed views once
            const int64_t i = u < v ? u : v, j = u < v ? v : u;
            const int64_t ij = i * n - i * (i + 1) / 2 + (j - i - 1);  // get_ij order
            if (ij < first || ij >= first + count) continue;
            out->idx.insert(out->idx.end(), {(int32_t)i, (int32_t)j, (int32_t)i, (int32_t)j});
            out->slots.push_back((int32_t)(ij - first));
        }
}

}  // namespace ecc_view_changes

#endif
