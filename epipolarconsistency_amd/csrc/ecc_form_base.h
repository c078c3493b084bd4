// ecc_form_base.h -- whether the base columns a metric keeps between the pose-delta calls of the form families may serve the next
// call (ecc_metric_set_form_incremental).  Host only, no HIP: compiled by tests/c/form_base.cpp as well as by
// ecc_form_call.h.
//
// The five *_pose_deltas calls of ecc_form_call.h begin with the form's T columns over all n (n - 1) / 2 pairs of the current
// matrices.  A column entry is a function of the pair's two matrices, its Radon intermediates, the form's parameters and the
// launch's parameters only, so columns kept from the previous call are the current ones wherever none of these changed.  Key is
// everything but the matrices and the contents of the intermediates (whoever changes those drops the kept columns:
// ecc_metric_refresh_dtrs); decide() compares the keys and the matrices, view by view and bitwise:
//   MISS      nothing kept; a key field differs; the resolved mode is ECC_SAMPLING_REFERENCE (may_keep: under it nothing is ever
//             kept -- it reads the callers' slabs, which are "always current" without ecc_metric_refresh_dtrs); more than
//             limit(n) views differ; keeps_radius(changed) says the automatic object radius moved with view 0
//             -> everything is evaluated, as without the mode
//   HIT       no view differs -> nothing is evaluated
//   REFRESH   1 .. limit(n) views differ, *changed lists them ascending -> one pose grid of that many columns, scattered into the
//             kept columns (form_base_scatter_kernel.hip)
#ifndef ECC_FORM_BASE_H
#define ECC_FORM_BASE_H

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/ecc_hip.h"
#include "ecc_view_changes.h"

#ifndef ECC_POSE_BATCH_MAX_MOVED
#define ECC_POSE_BATCH_MAX_MOVED 32  // (ecc_pose_batches.h)
#endif

namespace ecc_form_base {

enum Kind { NONE = 0, WEIGHTED, ROBUST, WEIGHTED_ROBUST, VARIANCE, VARIANCE_ROBUST };

inline uint32_t bits_of(float x)
{
    uint32_t b;
    std::memcpy(&b, &x, sizeof(b));
    return b;
}

// What kept columns belong to, beside the matrices: the form and its parameters (floats bitwise: 0 where the form has none), the
// resolved sampling mode and the scalar parameters of the base's record launch (as RecordKey and ValueKey hold them), the sizes.
struct Key {
    int kind = NONE, T = 0, S = 0;
    int loss = 0;
    uint32_t delta = 0, floor = 0;
    int mode = ECC_SAMPLING_AUTO;  // resolved: never AUTO in a key that was taken
    uint32_t radius = 0, dkappa = 0, tol = 0;
    int use_corr = 0;
    int n_views = 0, n_dtrs = 0;
    bool operator==(const Key& o) const
    {
        return kind == o.kind && T == o.T && S == o.S && loss == o.loss && delta == o.delta && floor == o.floor && mode == o.mode &&
               radius == o.radius && dkappa == o.dkappa && tol == o.tol && use_corr == o.use_corr && n_views == o.n_views && n_dtrs == o.n_dtrs;
    }
};

enum Decision { MISS = 0, HIT = 1, REFRESH = 2 };

// Changed views a refresh takes: the pose batch's columns per pose, and a quarter of the views (as ecc_metric_set_incremental).
inline int64_t limit(int64_t n) { return std::min<int64_t>(ECC_POSE_BATCH_MAX_MOVED, n / 4); }

// Whether columns evaluated under `key` may be kept at all.
inline bool may_keep(const Key& key) { return key.kind != NONE && key.mode != ECC_SAMPLING_REFERENCE; }

// Base pairs a call evaluates: all of them on a miss, none on a hit, the pairs that contain one of c changed views on a refresh.
inline int64_t base_pairs(Decision d, int64_t n, int64_t c)
{
    if (d == HIT) return 0;
    return d == MISS ? n * (n - 1) / 2 : c * (n - 1) - c * (c - 1) / 2;
}

// kept_valid, kept_key, kept_Ps (12 kept_key.n_views doubles): what is kept; key, cur_Ps: the call.  max_changed: limit(n), or the
// caller's smaller bound.  keeps_radius(changed): false when the object radius of the call differs from the kept columns' although
// the keys agree (the caller's rule for a changed view 0 under the automatic radius).  *changed: the views of a REFRESH, ascending;
// unspecified otherwise.
template <class KeepsRadius>
Decision decide(bool kept_valid, const Key& kept_key, const double* kept_Ps, const Key& key, const double* cur_Ps, int64_t max_changed,
                KeepsRadius&& keeps_radius, std::vector<int>* changed)
{
    changed->clear();
    if (!kept_valid || !kept_Ps || !may_keep(key) || !(kept_key == key)) return MISS;
    ecc_view_changes::changed_views(cur_Ps, kept_Ps, key.n_views, changed, max_changed);
    if (changed->empty()) return HIT;
    if ((int64_t)changed->size() > max_changed) return MISS;
    return keeps_radius(*changed) ? REFRESH : MISS;
}

}  // namespace ecc_form_base

#endif
