// ecc_direct_lists_host.h -- the host-only part of MetricDirect's index lists and pose batches: the checks of the lists and
// offsets a caller hands over, and the enumeration of the pairs a pose touches.  Plain C++ with no HIP in it, so that
// tests/c/direct_lists_host.cpp runs it under the sanitizers on a CPU (scripts/sanitize.sh).
#ifndef ECC_DIRECT_LISTS_HOST_H
#define ECC_DIRECT_LISTS_HOST_H

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace ecc_direct_lists {

constexpr int64_t MAX_PAIRS = 1 << 20;  // entries per call (the pose batch: over all its poses)

// Every check returns "" or the text of the refusal, naming the first offending entry.

// idx4: n_pairs tuples (P0, P1, I0, I1); P in [0, n_matrices), I in [0, n_images), P0 != P1
inline std::string check_idx4(const int32_t* idx4, int64_t n_pairs, int n_matrices, int n_images)
{
    if (n_pairs > MAX_PAIRS) return "more than 2^20 pairs in one call (" + std::to_string(n_pairs) + ")";
    for (int64_t q = 0; q < n_pairs; ++q) {
        const int32_t* t = idx4 + 4 * q;
        const std::string at = "entry " + std::to_string(q) + ": ";
        for (int s = 0; s < 2; ++s) {
            if (t[s] < 0 || t[s] >= n_matrices)
                return at + "matrix index " + std::to_string(t[s]) + " out of range [0, " + std::to_string(n_matrices) + ")";
            if (t[2 + s] < 0 || t[2 + s] >= n_images)
                return at + "image index " + std::to_string(t[2 + s]) + " out of range [0, " + std::to_string(n_images) + ")";
        }
        if (t[0] == t[1]) return at + "P0 == P1 (" + std::to_string(t[0]) + "): a pair needs two source positions";
    }
    return "";
}

// offsets: n + 1 entries, the first 0, non-decreasing, the last `total` (segments of a list, poses of a packed pose batch)
template <class Int>
inline std::string check_offsets(const Int* offsets, int64_t n, int64_t total, const char* what)
{
    if (offsets[0] != 0) return std::string(what) + " offsets do not start at 0 (" + std::to_string(offsets[0]) + ")";
    for (int64_t s = 0; s < n; ++s)
        if (offsets[s + 1] < offsets[s])
            return std::string(what) + " offsets decrease at entry " + std::to_string(s + 1) + " (" + std::to_string(offsets[s]) +
                   " -> " + std::to_string(offsets[s + 1]) + ")";
    if (total >= 0 && offsets[n] != total)
        return std::string(what) + " offsets end at " + std::to_string(offsets[n]) + ", not at the list length " + std::to_string(total);
    return "";
}

// The pairs (i < j < n_images) with at least one of m distinct moved views.
inline int64_t pose_pairs_count(int n_images, int64_t m) { return m * (n_images - 1) - m * (m - 1) / 2; }

// The packed pose lists: offsets as above (their end is the length of moved_views, which the caller vouches for), every pose
// with at most n_images views, each in [0, n_images) and named once; and at most MAX_PAIRS pairs in all.  moved_views may be
// null for the count alone (ecc_direct_pose_pairs_bound).
inline std::string check_poses(int n_poses, const int32_t* offsets, const int32_t* moved_views, int n_images, int64_t* n_pairs)
{
    std::string e = check_offsets(offsets, n_poses, -1, "pose");
    if (!e.empty()) return e;
    int64_t total = 0;
    std::vector<int> pose_of(moved_views ? (size_t)n_images : 0, -1);
    for (int k = 0; k < n_poses; ++k) {
        const int64_t m = (int64_t)offsets[k + 1] - offsets[k];
        if (m > n_images)
            return "pose " + std::to_string(k) + " moves " + std::to_string(m) + " views of " + std::to_string(n_images);
        for (int32_t q = offsets[k]; moved_views && q < offsets[k + 1]; ++q) {
            const int v = moved_views[q];
            if (v < 0 || v >= n_images)
                return "pose " + std::to_string(k) + ": view index " + std::to_string(v) + " out of range [0, " +
                       std::to_string(n_images) + ")";
            if (pose_of[(size_t)v] == k) return "pose " + std::to_string(k) + " names view " + std::to_string(v) + " twice";
            pose_of[(size_t)v] = k;
        }
        total += pose_pairs_count(n_images, m);
        if (total > MAX_PAIRS) return "more than 2^20 pairs in one call (reached at pose " + std::to_string(k) + ")";
    }
    *n_pairs = total;
    return "";
}

// The pairs of one pose in ascending (i, j) order, each once: emit(i, j, slot_i, slot_j) with slot = the position of the view
// in `views` (its candidate matrix) or -1 for a view that keeps its matrix.  `slot` is scratch of n_images entries, all -1 on
// entry and on return; `sorted` is scratch.  Returns the number of pairs (= pose_pairs_count).
template <class Emit>
inline int64_t pose_pairs(int n_images, const int32_t* views, int m, std::vector<int>& slot, std::vector<int>& sorted, Emit emit)
{
    sorted.assign(views, views + m);
    std::sort(sorted.begin(), sorted.end());
    for (int q = 0; q < m; ++q) slot[(size_t)views[q]] = q;
    int64_t count = 0;
    for (int i = 0; i < n_images; ++i) {
        if (slot[(size_t)i] >= 0) {
            for (int j = i + 1; j < n_images; ++j, ++count) emit(i, j, slot[(size_t)i], slot[(size_t)j]);
        } else {
            for (auto it = std::upper_bound(sorted.begin(), sorted.end(), i); it != sorted.end(); ++it, ++count)
                emit(i, *it, -1, slot[(size_t)*it]);
        }
    }
    for (int q = 0; q < m; ++q) slot[(size_t)views[q]] = -1;
    return count;
}

}  // namespace ecc_direct_lists

#endif
