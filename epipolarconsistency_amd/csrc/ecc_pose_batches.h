// ecc_pose_batches.h -- which poses of a pose-delta call go into which batch (host only, no HIP: compiled by
// tests/c/pose_batches.cpp as well as by ecc_poses.hip and, through ecc_form_call.h, the weighted and robust pose-delta calls).
//
// A call hands over poses as lists of moved views (off, views, moved_Ps: ecc_metric_evaluate_pose_deltas).  A batch is ONE record
// launch, ONE pair launch and ONE segmented sum over a grid of n x (its columns), a column per (pose, moved view); the packing rule
// says which poses a batch takes and where it ends, and is the same for every form of the batch.
#ifndef ECC_POSE_BATCHES_H
#define ECC_POSE_BATCHES_H

#include <cstddef>
#include <cstdint>
#include <vector>

#ifndef ECC_POSE_BATCH_MAX_MOVED
#define ECC_POSE_BATCH_MAX_MOVED 32  // moved views per pose the batch takes; a pose with more is evaluated the sequential way
#endif

namespace ecc_pose_batches {

// The poses of one batch, in the order of the call: off[0] = 0 ... off[K] = Q columns, the Q moved views and their matrices,
// and which pose of the call each of the K is.
struct Batch {
    std::vector<int32_t> off, views;
    std::vector<double> Ps;
    std::vector<int> pose;
};

// Walks the n_poses poses in order.  A pose with more than ECC_POSE_BATCH_MAX_MOVED moved views, or one for which
// keeps_radius(c, its views, its matrices) is false, goes into not_batched; every other pose joins the open batch, which is handed to
// run_batch(batch) -- and a new one opened -- before a pose that would take its columns past max_cols, once it holds max_poses
// poses, and at the end.  An empty batch is never run.  The first non-zero return of run_batch ends the walk and is returned.
template <class KeepsRadius, class RunBatch>
int pack(int n_poses, const int32_t* off, const int32_t* views, const double* moved_Ps, int64_t max_cols, size_t max_poses,
         KeepsRadius&& keeps_radius, RunBatch&& run_batch, std::vector<int>* not_batched)
{
    Batch b;
    auto flush = [&]() -> int {
        if (b.pose.empty()) return 0;
        const int e = run_batch(b);
        if (e) return e;
        b.pose.clear();
        b.off.assign(1, 0);
        b.views.clear();
        b.Ps.clear();
        return 0;
    };
    b.off.assign(1, 0);
    for (int k = 0; k < n_poses; ++k) {
        const int c = off[k + 1] - off[k];
        const int32_t* vk = views + off[k];
        const double* Pk = moved_Ps + 12 * (size_t)off[k];
        if (c > ECC_POSE_BATCH_MAX_MOVED || !keeps_radius(c, vk, Pk)) {
            not_batched->push_back(k);
            continue;
        }
        if ((int64_t)b.views.size() + c > max_cols || b.pose.size() >= max_poses) {
            const int rc = flush();
            if (rc) return rc;
        }
        b.pose.push_back(k);
        b.views.insert(b.views.end(), vk, vk + c);
        b.Ps.insert(b.Ps.end(), Pk, Pk + 12 * (size_t)c);
        b.off.push_back((int32_t)b.views.size());
    }
    return flush();
}

}  // namespace ecc_pose_batches

#endif
