// Driver for the packing rule of the pose batches (epipolarconsistency_amd/csrc/ecc_pose_batches.h), CPU only: which poses of a
// pose-delta call go into which batch, where a batch ends, and what is left to the sequential way.  For n = 2, 3, 5 and 40 views,
// poses with 0, 1, ECC_POSE_BATCH_MAX_MOVED and ECC_POSE_BATCH_MAX_MOVED + 1 moved views, poses that move view 0 under a radius
// predicate that answers false, column totals exactly on, one below and one above max_cols, small pose bounds, an empty call, calls
// in which nothing is batched and a batch function that fails:
//   against old_pack    the loop of evaluate_deltas (ecc_poses.hip) before it moved into the header, verbatim but for what it ran
//                       per batch: the same batches -- off, views, matrices, pose indices --, the same not_batched list, the same
//                       flush points, in the same order, the same return value;
//   on its own          every pose once, batched or not, in the order of the call; the matrices are the call's; no batch is empty,
//                       holds more than max_poses poses, or passes max_cols with more than one pose.
// max_cols and the pose bound are parameters here, so the boundaries are reached with tens of poses.  Built by
// tests/test_abi_and_host.py with -Wall -Werror.
#include <algorithm>
#include <cstdio>
#include <functional>

#include "../../epipolarconsistency_amd/csrc/ecc_pose_batches.h"

namespace {

struct Call {
    std::vector<int32_t> off{0}, views;
    std::vector<double> Ps;
    void add(int n, int c, int first_view, bool changes_radius)
    {
        for (int q = 0; q < c; ++q) {
            views.push_back(first_view + q);
            for (int e = 0; e < 12; ++e) Ps.push_back((changes_radius ? -1.0 : 1.0) * (double)(1000 * off.size() + 12 * q + e + 1));
        }
        off.push_back((int32_t)views.size());
        if (first_view + c > n) std::printf("bad case: view past n\n");
    }
    int n_poses() const { return (int)off.size() - 1; }
};

// the stand-in for pose_keeps_radius: a pose that moves view 0 to a matrix with a negative first entry changes the radius
bool keeps_radius(int c, const int32_t* views, const double* moved_Ps) { return c < 1 || views[0] != 0 || moved_Ps[0] > 0.0; }

struct Seen {
    std::vector<ecc_pose_batches::Batch> batches;
    std::vector<int> not_batched;
    int rc = 0;
};

// The packing loop of evaluate_deltas (ecc_poses.hip) before it moved into ecc_pose_batches.h, verbatim: run_batch and the means
// became run(b_off, b_views, b_Ps, b_pose), pose_keeps_radius(m, base_radius, ...) became keeps_radius(...), POSE_BATCH_MAX_POSES
// became max_poses.
int old_pack(int n_poses, const int32_t* off, const int32_t* views, const double* moved_Ps, int64_t max_cols, size_t max_poses,
             const std::function<int(const std::vector<int32_t>&, const std::vector<int32_t>&, const std::vector<double>&, const std::vector<int>&)>& run,
             std::vector<int>* not_batched)
{
    int rc = 0;
    std::vector<int32_t> b_off, b_views;
    std::vector<double> b_Ps, sums;
    std::vector<int> b_pose;
    auto flush = [&]() -> int {
        if (b_pose.empty()) return 0;
        sums.resize(b_pose.size());
        const int e = run(b_off, b_views, b_Ps, b_pose);
        if (e) return e;
        b_pose.clear();
        b_off.assign(1, 0);
        b_views.clear();
        b_Ps.clear();
        return 0;
    };
    b_off.assign(1, 0);
    for (int k = 0; k < n_poses; ++k) {
        const int c = off[k + 1] - off[k];
        const int32_t* vk = views + off[k];
        const double* Pk = moved_Ps + 12 * (size_t)off[k];
        if (c > ECC_POSE_BATCH_MAX_MOVED || !keeps_radius(c, vk, Pk)) {
            not_batched->push_back(k);
            continue;
        }
        if ((int64_t)b_views.size() + c > max_cols || b_pose.size() >= max_poses) {
            rc = flush();
            if (rc) return rc;
        }
        b_pose.push_back(k);
        b_views.insert(b_views.end(), vk, vk + c);
        b_Ps.insert(b_Ps.end(), Pk, Pk + 12 * (size_t)c);
        b_off.push_back((int32_t)b_views.size());
    }
    rc = flush();
    if (rc) return rc;
    return 0;
}

int failures = 0;
long long cases = 0, batches_seen = 0;
void check(bool ok, const char* what, const char* name, int64_t max_cols, size_t max_poses)
{
    if (ok) return;
    if (++failures <= 20) std::printf("FAIL %s: case %s, max_cols=%lld, max_poses=%zu\n", what, name, (long long)max_cols, max_poses);
}

// fail_at >= 0: the batch function returns 7 at that batch
void run_case(const char* name, const Call& call, int64_t max_cols, size_t max_poses, int fail_at = -1)
{
    ++cases;
    Seen want, got;
    want.rc = old_pack(
        call.n_poses(), call.off.data(), call.views.data(), call.Ps.data(), max_cols, max_poses,
        [&](const std::vector<int32_t>& o, const std::vector<int32_t>& v, const std::vector<double>& P, const std::vector<int>& pose) {
            if ((int)want.batches.size() == fail_at) return 7;
            want.batches.push_back({o, v, P, pose});
            return 0;
        },
        &want.not_batched);
    got.rc = ecc_pose_batches::pack(
        call.n_poses(), call.off.data(), call.views.data(), call.Ps.data(), max_cols, max_poses, keeps_radius,
        [&](const ecc_pose_batches::Batch& b) {
            if ((int)got.batches.size() == fail_at) return 7;
            got.batches.push_back(b);
            return 0;
        },
        &got.not_batched);
    batches_seen += (long long)got.batches.size();
    bool same = got.rc == want.rc && got.not_batched == want.not_batched && got.batches.size() == want.batches.size();
    for (size_t b = 0; same && b < got.batches.size(); ++b) {
        const ecc_pose_batches::Batch &x = got.batches[b], &y = want.batches[b];
        same = x.off == y.off && x.views == y.views && x.Ps == y.Ps && x.pose == y.pose;
    }
    check(same, "differs from the old loop", name, max_cols, max_poses);
    if (fail_at >= 0) {  // the failing batch ends the walk with its code; a call with no more than fail_at batches never meets it
        check(got.rc == 0 || (got.rc == 7 && (int)got.batches.size() == fail_at), "return value", name, max_cols, max_poses);
        return;
    }
    check(got.rc == 0, "return value", name, max_cols, max_poses);
    // on its own: a merge of the batched poses (in batch order) and not_batched gives 0 .. n_poses - 1
    std::vector<int> order;
    bool ok = true;
    for (const ecc_pose_batches::Batch& b : got.batches) {
        const size_t K = b.pose.size();
        ok = ok && K >= 1 && K <= max_poses && b.off.size() == K + 1 && b.off[0] == 0 && b.off[K] == (int32_t)b.views.size() &&
             b.Ps.size() == 12 * b.views.size() && ((int64_t)b.views.size() <= max_cols || K == 1);
        for (size_t q = 0; ok && q < K; ++q) {
            const int k = b.pose[q], c = call.off[k + 1] - call.off[k];
            ok = b.off[q + 1] - b.off[q] == c && c <= ECC_POSE_BATCH_MAX_MOVED &&
                 std::equal(b.views.begin() + b.off[q], b.views.begin() + b.off[q + 1], call.views.begin() + call.off[k]) &&
                 std::equal(b.Ps.begin() + 12 * b.off[q], b.Ps.begin() + 12 * b.off[q + 1], call.Ps.begin() + 12 * (size_t)call.off[k]) &&
                 keeps_radius(c, call.views.data() + call.off[k], call.Ps.data() + 12 * (size_t)call.off[k]);
            order.push_back(k);
        }
    }
    ok = ok && std::is_sorted(order.begin(), order.end()) && std::is_sorted(got.not_batched.begin(), got.not_batched.end());
    for (int k : got.not_batched) {
        const int c = call.off[k + 1] - call.off[k];
        ok = ok && (c > ECC_POSE_BATCH_MAX_MOVED || !keeps_radius(c, call.views.data() + call.off[k], call.Ps.data() + 12 * (size_t)call.off[k]));
    }
    order.insert(order.end(), got.not_batched.begin(), got.not_batched.end());
    std::sort(order.begin(), order.end());
    ok = ok && (int)order.size() == call.n_poses();
    for (size_t k = 0; ok && k < order.size(); ++k) ok = order[k] == (int)k;
    check(ok, "properties", name, max_cols, max_poses);
}

}  // namespace

int main()
{
    const int MM = ECC_POSE_BATCH_MAX_MOVED;
    const size_t bounds[] = {1, 2, 3, 7, 1000};
    unsigned long long state = 88172645463325252ull;
    auto rnd = [&]() {
        state ^= state << 13;
        state ^= state >> 7;
        state ^= state << 17;
        return state;
    };
    for (int n : {2, 3, 5, 40}) {
        const int big = std::min(n, MM), over = std::min(n, MM + 1);  // (a pose cannot move more views than there are)
        std::vector<int64_t> col_bounds = {1, 2, 5, 8, big, big + 1, 2 * big, 2 * big + 1, 64, 1 << 20};
        std::vector<std::pair<const char*, Call>> calls;
        calls.push_back({"empty call", Call()});
        {
            Call c;  // one pose of every size, moving view 0 or not, keeping the radius or not
            for (int count : {0, 1, big, over})
                for (int first : {0, 1})
                    for (bool changes : {false, true})
                        if (first + count <= n) c.add(n, count, first, changes);
            calls.push_back({"every size", c});
        }
        {
            Call c;  // nothing is batched: every pose changes the radius (or, at 40 views, moves too many)
            for (int k = 0; k < 9; ++k) c.add(n, k % 2 && over > MM ? over : 1, 0, true);
            calls.push_back({"nothing batched", c});
        }
        {
            Call c;  // nothing moved at all: poses without columns fill batches up to the pose bound only
            for (int k = 0; k < 20; ++k) c.add(n, 0, 0, false);
            calls.push_back({"no columns", c});
        }
        for (int64_t M : {(int64_t)8, (int64_t)big + 1, (int64_t)2 * big})
            for (int64_t lead : {M - 3, M - 2, M - 1}) {
                if (lead < 0 || n < 2) continue;
                Call c;  // `lead` poses of one view, then one of two: the total lands one below, on and one above M; then the same again
                for (int rep = 0; rep < 2; ++rep) {
                    for (int64_t k = 0; k < lead; ++k) c.add(n, 1, (int)(k % n), false);
                    c.add(n, 2, 0, false);
                    if (rep == 0) c.add(n, 1, 0, true);  // (left out of the batch, between two batched poses)
                }
                calls.push_back({"totals around max_cols", c});
                col_bounds.push_back(M);
            }
        for (int rep = 0; rep < 6; ++rep) {
            Call c;
            const int poses = 10 + (int)(rnd() % 50);
            for (int k = 0; k < poses; ++k) {
                const int pick = (int)(rnd() % 8);
                const int count = pick == 0 ? 0 : pick == 1 ? big : pick == 2 ? over : 1 + (int)(rnd() % std::min(n, 4));
                const int first = (int)(rnd() % (unsigned)(n - count + 1));
                c.add(n, count, rnd() % 3 ? first : 0, rnd() % 4 == 0);
            }
            calls.push_back({"random", c});
        }
        for (const auto& nc : calls)
            for (int64_t max_cols : col_bounds)
                for (size_t max_poses : bounds) {
                    run_case(nc.first, nc.second, max_cols, max_poses);
                    for (int fail_at : {0, 1}) run_case(nc.first, nc.second, max_cols, max_poses, fail_at);
                }
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok: %lld cases, %lld batches\n", cases, batches_seen);
    return 0;
}
