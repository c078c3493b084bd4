"""ecc_metric_evaluate_weighted_robust_pose_deltas on the GPU (csrc/ecc_weighted_robust_batches.hip, csrc/form_sums_kernel.hip): line
weights and the robust loss together for pose optimisers -- K poses that each move a few views as one record launch, one
weighted-robust pair launch and one segmented sum of the three columns {c, u, k} per batch.

The data, weights, poses and moved views are tests/test_gpu_weighted_poses.py's (_Scan: seven random intermediates and seven
weight_fields dealt to the views).  delta = weighted_robust_scale(the base's rows at delta = inf, 0.5) as a float32, so about half
the pairs have residuals beyond it.  The contract is BITS: values, coverages and inlier masses equal setProjectionMatrices +
evaluate_weighted_robust per pose on a second metric with batching off, whatever the number of pairs (both forms of the sum, with and
without a tail, several chunks per slice), the sampling mode, the loss, the moved views, the fallbacks and the batch splitting; with
delta = inf the results are evaluate_weighted_pose_deltas', with weights of one evaluate_robust_pose_deltas'; and nothing else the
metric returns moves."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_pose_batch import _perturb, _poses
from test_gpu_weighted_poses import _Scan, _moved_of

pytestmark = pytest.mark.gpu
INF = float("inf")
FLT_MAX = float(np.finfo(np.float32).max)


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _delta(s, m):
    """weighted_robust_scale of the rows at the metric's current matrices, k = 0.5, as the float32 the calls take"""
    return float(np.float32(s.E.weighted_robust_scale(m.evaluate_weighted_robust(0, INF, want_pairs=True)[3], 0.5)))


def _sequential(b, poses, loss, delta):
    out = [b.setProjectionMatrices(P).evaluate_weighted_robust(loss, delta) for P in poses]
    return tuple(np.array([o[q] for o in out]) for q in range(3))


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(_u64(g), _u64(w)) for g, w in zip(got, want))


def _shape(n):
    return dict(S=96 if n > 300 else 128, B=32 if n > 100 else 48)


# ---- (a) - (e) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,mode,loss", [(2, "polynomial", 0), (3, "auto", 1), (9, "auto", 2), (9, "polynomial", 0), (34, "per_sample", 1),
                                         (67, "polynomial", 2), (130, "auto", 0), (257, "polynomial", 1), (258, "auto", 2),
                                         (520, "polynomial", 0)])
def test_deltas_have_the_sequential_bits(gpu_ctx, n, mode, loss):
    """Pairs: 1; 3 (tail only); 36 (reference arithmetic under auto); 36; 561; 2 211 (tail 3); 8 385 (one slice, several chunks, tail
    1); 32 896 / 33 153 (sixteen slices, without and with a tail); 134 940 (a slice longer than one chunk).  Losses: Huber, truncated,
    Geman-McClure in turn."""
    s = _Scan(gpu_ctx, n, **_shape(n))
    ones = _Scan(gpu_ctx, n, per_view=[np.ones((s.B, s.B), np.float32)] * n, **_shape(n))
    try:
        K = 23 if n < 200 else (11 if n < 500 else 3)
        moved_of = _moved_of(n) if n < 500 else (lambda k: [[n - 1], [1, n // 2], []][k])
        poses, views, rows = _poses(s.P0, n, K, moved_of)
        a, b = s.metric(mode), s.metric(mode, batching=False)
        delta = _delta(s, a)
        assert 0.0 < delta < INF
        want = _sequential(b, poses, loss, delta)
        before = (a.evaluate(), a.evaluate_weighted_robust(loss, delta, want_pairs=True), a.evaluate_pose_deltas(views[:4], rows[:4]))
        got = a.evaluate_weighted_robust_pose_deltas(views, rows, loss, delta)
        # (a)
        assert len(got) == 3
        assert _same(got, want), (n, mode, loss, [np.flatnonzero(g != w) for g, w in zip(got, want)])
        # (a pose that moves view 0 changes the automatic object radius: evaluated the sequential way inside the call)
        assert K - sum(1 for vk in views if 0 in vk) <= a.last_batched_poses() <= K
        # (b) delta = inf, FLT_MAX: the weighted pose deltas' bits, every mass exactly 1
        weighted = a.evaluate_weighted_pose_deltas(views, rows)
        for d in (INF, FLT_MAX):
            at = a.evaluate_weighted_robust_pose_deltas(views, rows, loss, d)
            assert np.array_equal(_u64(at[0]), _u64(weighted[0])), (n, mode, d, at[0] - weighted[0])
            assert np.array_equal(_u64(at[1]), _u64(weighted[1])), (n, mode, d, at[1] - weighted[1])
            assert np.all(at[2] == 1.0), at[2]
        # (c) weights of one on the 2 n metric: the robust pose deltas of the n-metric over the same data, every coverage exactly 1
        wa = ones.metric(mode)
        ra = ones.E.MetricRadonIntermediate(gpu_ctx, ones.Ps, ones.data).setSampling(mode)
        ones.metrics.append(ra)
        robust = ra.evaluate_robust_pose_deltas(views, rows, loss, delta)
        at_one = wa.evaluate_weighted_robust_pose_deltas(views, rows, loss, delta)
        assert np.array_equal(_u64(at_one[0]), _u64(robust[0])), (n, mode, at_one[0] - robust[0])
        assert np.array_equal(_u64(at_one[2]), _u64(robust[1])), (n, mode, at_one[2] - robust[1])
        assert np.all(at_one[1] == 1.0), at_one[1]
        # (d) weights and loss are both seen
        if n >= 9:
            assert np.all(got[1] > 0.0) and np.all(got[1] < 1.0), got[1]
            assert np.all(got[2] > 0.0) and np.all(got[2] < 1.0), got[2]
            assert np.all(got[0] != weighted[0]), (got[0], weighted[0])
            assert len(set(got[0].tolist())) >= 3
        # (e) nothing else moved: evaluate(), the weighted-robust results with their rows, a pose batch made before the call
        after = (a.evaluate(), a.evaluate_weighted_robust(loss, delta, want_pairs=True), a.evaluate_pose_deltas(views[:4], rows[:4]))
        assert _u64(after[0])[()] == _u64(before[0])[()]
        assert _same(after[1][:3], before[1][:3]) and np.array_equal(_u32(after[1][3]), _u32(before[1][3]))
        assert np.array_equal(_u64(after[2]), _u64(before[2]))
        base_r = b.setProjectionMatrices(s.P0).evaluate_weighted_robust(loss, delta)
        assert _same(base_r, before[1][:3])     # the current matrices are still the base
        # a second call from a different base
        P1 = poses[5 % K]
        a.setProjectionMatrices(P1)
        poses2, views2, rows2 = _poses(P1, n, 6 if n < 500 else 2, lambda k: [(5 * k + 2) % n])
        assert _same(a.evaluate_weighted_robust_pose_deltas(views2, rows2, loss, delta), _sequential(b, poses2, loss, delta)), (n, mode)
    finally:
        ones.close()
        s.close()


# ---- fallbacks -----------------------------------------------------------------------------------------------------------------------
def test_fallbacks_inside_the_call(gpu_ctx):
    """33 moved views (more than the batch takes), view 0 moved under the automatic radius, batching off: the sequential way inside the
    call, the same bits, the base matrices current afterwards; a fixed radius batches view 0 too."""
    n, loss = 50, 0
    s = _Scan(gpu_ctx, n)
    try:
        lists = [list(range(1, 34)), [4], [0], [], [9, 30], [0, 7], [49]]
        poses, views, rows = _poses(s.P0, n, len(lists), lambda k: lists[k])
        a, b = s.metric("polynomial"), s.metric("polynomial", batching=False)
        delta = _delta(s, a)
        want = _sequential(b, poses, loss, delta)
        base = b.setProjectionMatrices(s.P0).evaluate_weighted_robust(loss, delta)
        got = a.evaluate_weighted_robust_pose_deltas(views, rows, loss, delta)
        assert _same(got, want), [g - w for g, w in zip(got, want)]
        # the two poses that move view 0 keep the radius only if it rounds to the base's float: the plain call decides the same way
        batched = a.last_batched_poses()
        a.evaluate_pose_deltas(views, rows)
        assert batched == a.last_batched_poses() and 4 <= batched <= 6
        assert _same(a.evaluate_weighted_robust(loss, delta), base)
        a.setObjectRadius(80.0)
        b.setObjectRadius(80.0)
        want_r = _sequential(b, poses, loss, delta)
        assert _same(a.evaluate_weighted_robust_pose_deltas(views, rows, loss, delta), want_r) and a.last_batched_poses() == 6   # all but the 33 views
        a.setPoseBatching(False)
        assert _same(a.evaluate_weighted_robust_pose_deltas(views, rows, loss, delta), want_r) and a.last_batched_poses() == 0
        assert _same(a.evaluate_weighted_robust(loss, delta), b.setProjectionMatrices(s.P0).evaluate_weighted_robust(loss, delta))
    finally:
        s.close()


def test_more_entries_than_one_batch_takes(gpu_ctx):
    """No hook makes a batch smaller than ECC_POSE_BATCH_MAX_ENTRIES (2^20), so: 8 200 poses of one moved view over 130 views are
    1 066 000 grid entries -- two batches (8 065 + 135 columns) over one base.  Every pose against the same poses in calls of one batch
    each; the poses around the cut and every 97th against the sequential call."""
    n, K, loss = 130, 8200, 2
    s = _Scan(gpu_ctx, n, B=32)
    try:
        rng = np.random.default_rng(2)
        moved = rng.integers(1, n, size=K).astype(np.int32)
        rows = np.stack([_perturb(s.P0[v], k % 97, int(v)) for k, v in enumerate(moved)])
        a, b = s.metric("polynomial"), s.metric("polynomial", batching=False)
        delta = _delta(s, a)
        got = a.evaluate_weighted_robust_pose_deltas_packed(np.arange(K + 1, dtype=np.int32), moved, rows, loss, delta)
        assert a.last_batched_poses() == K
        for lo in range(0, K, 4100):
            part = a.evaluate_weighted_robust_pose_deltas_packed(np.arange(4101, dtype=np.int32), moved[lo:lo + 4100], rows[lo:lo + 4100], loss, delta)
            assert _same(tuple(g[lo:lo + 4100] for g in got), part), lo
        cut = (1 << 20) // n
        which = sorted(set(range(0, K, 97)) | set(range(cut - 4, cut + 4)) | {K - 1})
        P = s.P0.copy()
        for k in which:
            P[moved[k]] = rows[k]
            want = b.setProjectionMatrices(P).evaluate_weighted_robust(loss, delta)
            P[moved[k]] = s.P0[moved[k]]
            assert all(_u64(got[q][k])[()] == _u64(want[q])[()] for q in range(3)), k
        assert np.all(got[1] < 1.0) and np.all(got[1] > 0.0) and np.all(got[2] < 1.0) and np.all(got[2] > 0.0)
    finally:
        s.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors(gpu_ctx):
    """Every documented error on a live metric, through the C call with its outputs preset: the code, and nothing written."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib
    n = 6
    s = _Scan(gpu_ctx, n)
    try:
        m = s.metric("polynomial")
        P0 = s.P0
        delta = _delta(s, m)
        base = m.evaluate()
        want = m.evaluate_weighted_robust_pose_deltas([[2]], [P0[3:4]], 0, delta)
        fn = _lib.lib().ecc_metric_evaluate_weighted_robust_pose_deltas

        def call(metric, off, views, Ps, loss, d, outputs=(True, True, True)):
            off, views = np.asarray(off, np.int32), np.asarray(views, np.int32)
            Ps = np.ascontiguousarray(Ps, np.float64)
            outs = [np.full(max(len(off) - 1, 1), -7.0) for _ in range(3)]
            rc = fn(metric._h, len(off) - 1, C.c_void_p(off.ctypes.data), C.c_void_p(views.ctypes.data) if len(views) else None,
                    C.c_void_p(Ps.ctypes.data) if len(views) else None, loss, d,
                    *[C.c_void_p(o.ctypes.data) if on else None for o, on in zip(outs, outputs)])
            return rc, outs

        def refused(code, *args, **kw):
            rc, outs = call(*args, **kw)
            assert rc == code, (rc, code, args[1:])
            assert all(np.all(o == -7.0) for o in outs), outs          # nothing written
        one_pose = ([0, 1], [2], P0[3:4])
        for loss, d in ((3, delta), (-1, delta), (0, 0.0), (0, -1.0), (0, float("nan"))):
            refused(1, m, *one_pose, loss, d)                             # loss outside 0..2, delta <= 0 or NaN
        refused(1, m, [0, 2], [2, 2], np.stack([P0[2], P0[2]]), 0, delta)  # not strictly ascending
        refused(1, m, [0, 2], [3, 1], P0[:2], 0, delta)
        refused(1, m, [0, 1], [n], P0[:1], 0, delta)                      # outside [0, n)
        refused(1, m, [0, 1], [-1], P0[:1], 0, delta)
        refused(1, m, *one_pose, 0, delta, outputs=(False, True, True))   # values is required
        assert _u64(m.evaluate())[()] == _u64(base)[()]
        rc, outs = call(m, *one_pose, 0, delta, outputs=(True, False, False))   # ... coverages and inlier_masses are not
        assert rc == 0 and _u64(outs[0][0])[()] == _u64(want[0][0])[()] and outs[1][0] == outs[2][0] == -7.0
        m.useCorrelation(True)
        refused(5, m, *one_pose, 0, delta)                                # ECC_ERR_UNSUPPORTED
        refused(1, m, *one_pose, 3, delta)                                # (the loss is checked before it)
        m.useCorrelation(False)
        assert _same(m.evaluate_weighted_robust_pose_deltas([[2]], [P0[3:4]], 0, delta), want)
        assert _u64(m.evaluate())[()] == _u64(base)[()]
        got = m.evaluate_weighted_robust_pose_deltas([], [], 0, delta)    # n_poses < 1: ECC_OK
        assert len(got) == 3 and all(len(g) == 0 for g in got)
        assert m.last_batched_poses() == 1                                # (the call before it; n_poses < 1 returns before the reset)
        here = m.evaluate_weighted_robust(0, delta)
        got = m.evaluate_weighted_robust_pose_deltas([[]], [np.zeros((0, 12))], 0, delta)   # a pose that moves nothing: the base
        assert all(_u64(got[q][0])[()] == _u64(here[q])[()] for q in range(3))
        for dtrs in (s.data, s.data + s.weights[:-1], s.data + s.weights + s.weights[:1]):   # n, 2 n - 1, 2 n + 1 intermediates
            bad = E.MetricRadonIntermediate(gpu_ctx, s.Ps, dtrs)
            s.metrics.append(bad)
            refused(1, bad, *one_pose, 0, delta)
        one = E.MetricRadonIntermediate(gpu_ctx, s.Ps[:1], [s.data[0], s.weights[0]])       # fewer than two views
        none = E.MetricRadonIntermediate(gpu_ctx, None, s.data + s.weights)                 # no matrices set
        s.metrics += [one, none]
        refused(1, one, [0, 1], [0], P0[:1], 0, delta)
        refused(1, none, [0, 1], [0], P0[:1], 0, delta)
    finally:
        s.close()
