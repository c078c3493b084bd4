"""ecc_metric_evaluate_robust_pose_deltas on the GPU (csrc/ecc_robust_batches.hip): the metric under a per-sample robust loss for pose
optimisers -- K poses that each move a few views as one record launch, one robust pair launch and one segmented sum per batch.

The data are tests/test_gpu_pose_batch.py's (_scan: seven random intermediates dealt to the views), the poses that file's _perturb /
_poses pattern with the moved_of of tests/test_gpu_weighted_poses.py.  delta = robust_scale(the base's rows, 0.5), so about half the
pairs have residuals beyond it.  The contract is BITS: values and inlier masses equal setProjectionMatrices + evaluate_robust per pose
on a second metric with batching off, whatever the number of pairs (both forms of the sum, with and without a tail), the sampling mode,
the loss, the moved views, the fallbacks and the batch splitting; with delta = inf the values are evaluate_pose_deltas'; and nothing
else the metric returns moves."""
import numpy as np
import pytest

from test_gpu_pose_batch import _perturb, _poses, _scan
from test_gpu_weighted_poses import _moved_of

pytestmark = pytest.mark.gpu
INF = float("inf")


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


class _Scan:
    """n views over the data of _scan; every metric made here is closed with it."""

    def __init__(self, gpu_ctx, n, S=128, B=48):
        import epipolarconsistency_amd as E
        self.E, self.ctx, self.n = E, gpu_ctx, n
        self.Ps, self.base, self.data = _scan(gpu_ctx, n, S=S, B=B)
        self.P0 = E.pack_projection_matrices(self.Ps)
        self.metrics = []

    def metric(self, mode, batching=True):
        m = self.E.MetricRadonIntermediate(self.ctx, self.Ps, self.data).setSampling(mode).setPoseBatching(batching)
        self.metrics.append(m)
        return m

    def delta(self, m):
        """robust_scale of the rows at the metric's current matrices, k = 0.5, as the float32 the calls take"""
        return float(np.float32(self.E.robust_scale(m.evaluate_robust(0, INF, want_pairs=True)[2], 0.5)))

    def close(self):
        for m in self.metrics:
            m.close()
        for d in self.base:
            d.close()


def _sequential(b, poses, loss, delta):
    out = [b.setProjectionMatrices(P).evaluate_robust(loss, delta) for P in poses]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def _same(got, want):
    return np.array_equal(_u64(got[0]), _u64(want[0])) and np.array_equal(_u64(got[1]), _u64(want[1]))


# ---- (a) - (d): sequential bits, not vacuous, delta = inf, nothing else moved -------------------------------------------------------
@pytest.mark.parametrize("n,mode,loss", [(2, "polynomial", 0), (3, "auto", 1), (9, "auto", 2), (9, "polynomial", 0), (34, "per_sample", 1),
                                         (67, "polynomial", 2), (257, "polynomial", 0), (258, "auto", 1)])
def test_deltas_have_the_sequential_bits(gpu_ctx, n, mode, loss):
    """Pairs: 1; 3 (tail only); 36 (reference arithmetic under auto, four waves per pair); 36; 561; 2 211 (tail 3); 32 896 / 33 153
    (sixteen slices, without and with a tail).  Losses: Huber, truncated, Geman-McClure in turn."""
    s = _Scan(gpu_ctx, n, B=32 if n > 100 else 48)
    try:
        K = 23 if n < 200 else 11
        poses, views, rows = _poses(s.P0, n, K, _moved_of(n))
        a, b = s.metric(mode), s.metric(mode, batching=False)
        delta = s.delta(a)
        assert 0.0 < delta < INF
        want = _sequential(b, poses, loss, delta)
        before = (a.evaluate(), a.evaluate_robust(loss, delta, want_pairs=True), a.evaluate_pose_deltas(views[:4], rows[:4]))
        got = a.evaluate_robust_pose_deltas(views, rows, loss, delta)
        # (a)
        assert _same(got, want), (n, mode, loss, np.flatnonzero(got[0] != want[0]), np.flatnonzero(got[1] != want[1]))
        # (a pose that moves view 0 changes the automatic object radius: evaluated the sequential way inside the call)
        assert K - sum(1 for vk in views if 0 in vk) <= a.last_batched_poses() <= K
        # (c) delta = inf: the plain pose deltas' bits, every mass exactly 1
        plain = a.evaluate_pose_deltas(views, rows)
        at_inf = a.evaluate_robust_pose_deltas(views, rows, loss, INF)
        assert np.array_equal(_u64(at_inf[0]), _u64(plain)), (n, mode, at_inf[0] - plain)
        assert np.all(at_inf[1] == 1.0)
        at_max = a.evaluate_robust_pose_deltas(views, rows, loss, float(np.finfo(np.float32).max))
        assert np.array_equal(_u64(at_max[0]), _u64(plain)) and np.all(at_max[1] == 1.0)
        # (b) the loss is seen
        if n >= 9:
            assert np.all(got[1] < 1.0) and np.all(got[1] > 0.0), got[1]
            assert np.all(got[0] != plain) and np.all(got[0] > 0.0), (got[0], plain)
            assert len(set(got[0].tolist())) >= 3
        # (d) nothing else moved: evaluate(), the robust value with its rows, a pose batch made before the call
        after = (a.evaluate(), a.evaluate_robust(loss, delta, want_pairs=True), a.evaluate_pose_deltas(views[:4], rows[:4]))
        assert _u64(after[0])[()] == _u64(before[0])[()]
        assert _u64(after[1][0])[()] == _u64(before[1][0])[()] and _u64(after[1][1])[()] == _u64(before[1][1])[()]
        assert np.array_equal(_u32(after[1][2]), _u32(before[1][2]))
        assert np.array_equal(_u64(after[2]), _u64(before[2]))
        base_r = b.setProjectionMatrices(s.P0).evaluate_robust(loss, delta)
        assert _u64(base_r[0])[()] == _u64(before[1][0])[()] and _u64(base_r[1])[()] == _u64(before[1][1])[()]   # still the base
        # a second call from a different base
        P1 = poses[5 % K]
        a.setProjectionMatrices(P1)
        poses2, views2, rows2 = _poses(P1, n, 6, lambda k: [(5 * k + 2) % n])
        assert _same(a.evaluate_robust_pose_deltas(views2, rows2, loss, delta), _sequential(b, poses2, loss, delta)), (n, mode)
    finally:
        s.close()


# ---- (e) fallbacks -----------------------------------------------------------------------------------------------------------------
def test_fallbacks_inside_the_call(gpu_ctx):
    """33 moved views (more than the batch takes), view 0 moved under the automatic radius, batching off: the sequential way inside the
    call, the same bits, the base matrices current afterwards; a fixed radius batches view 0 too."""
    n, loss = 50, 0
    s = _Scan(gpu_ctx, n)
    try:
        lists = [list(range(1, 34)), [4], [0], [], [9, 30], [0, 7], [49]]
        poses, views, rows = _poses(s.P0, n, len(lists), lambda k: lists[k])
        a, b = s.metric("polynomial"), s.metric("polynomial", batching=False)
        delta = s.delta(a)
        want = _sequential(b, poses, loss, delta)
        base = b.setProjectionMatrices(s.P0).evaluate_robust(loss, delta)
        got = a.evaluate_robust_pose_deltas(views, rows, loss, delta)
        assert _same(got, want), (got[0] - want[0], got[1] - want[1])
        # the two poses that move view 0 keep the radius only if it rounds to the base's float: the plain call decides the same way
        batched = a.last_batched_poses()
        a.evaluate_pose_deltas(views, rows)
        assert batched == a.last_batched_poses() and 4 <= batched <= 6
        assert a.evaluate_robust(loss, delta) == base
        a.setObjectRadius(80.0)
        b.setObjectRadius(80.0)
        want_r = _sequential(b, poses, loss, delta)
        assert _same(a.evaluate_robust_pose_deltas(views, rows, loss, delta), want_r) and a.last_batched_poses() == 6   # all but the 33 views
        a.setPoseBatching(False)
        assert _same(a.evaluate_robust_pose_deltas(views, rows, loss, delta), want_r) and a.last_batched_poses() == 0
        assert a.evaluate_robust(loss, delta) == b.setProjectionMatrices(s.P0).evaluate_robust(loss, delta)
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
        delta = s.delta(a)
        got = a.evaluate_robust_pose_deltas_packed(np.arange(K + 1, dtype=np.int32), moved, rows, loss, delta)
        assert a.last_batched_poses() == K
        for lo in range(0, K, 4100):
            part = a.evaluate_robust_pose_deltas_packed(np.arange(4101, dtype=np.int32), moved[lo:lo + 4100], rows[lo:lo + 4100], loss, delta)
            assert _same((got[0][lo:lo + 4100], got[1][lo:lo + 4100]), part), lo
        cut = (1 << 20) // n
        which = sorted(set(range(0, K, 97)) | set(range(cut - 4, cut + 4)) | {K - 1})
        P = s.P0.copy()
        for k in which:
            P[moved[k]] = rows[k]
            want = b.setProjectionMatrices(P).evaluate_robust(loss, delta)
            P[moved[k]] = s.P0[moved[k]]
            assert _u64(got[0][k])[()] == _u64(want[0])[()] and _u64(got[1][k])[()] == _u64(want[1])[()], k
        assert np.all(got[1] < 1.0) and np.all(got[1] > 0.0)
    finally:
        s.close()


# ---- (f) errors --------------------------------------------------------------------------------------------------------------------
def test_errors(gpu_ctx):
    import ctypes as C
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib
    n = 6
    s = _Scan(gpu_ctx, n)
    try:
        m = s.metric("polynomial")
        P0 = s.P0
        delta = s.delta(m)
        base = m.evaluate()
        want = m.evaluate_robust_pose_deltas([[2]], [P0[3:4]], 0, delta)

        def raises(code, call):
            with pytest.raises(E.EccError) as e:
                call()
            assert e.value.code == code, e.value
            assert _u64(m.evaluate())[()] == _u64(base)[()]    # a following evaluate() keeps its bits
        raises(1, lambda: m.evaluate_robust_pose_deltas([[2]], [P0[3:4]], 3, delta))               # loss outside 0..2
        raises(1, lambda: m.evaluate_robust_pose_deltas([[2]], [P0[3:4]], -1, delta))
        raises(1, lambda: m.evaluate_robust_pose_deltas([[2]], [P0[3:4]], 0, 0.0))                 # delta <= 0
        raises(1, lambda: m.evaluate_robust_pose_deltas([[2]], [P0[3:4]], 0, -1.0))
        raises(1, lambda: m.evaluate_robust_pose_deltas([[2]], [P0[3:4]], 0, float("nan")))
        raises(1, lambda: m.evaluate_robust_pose_deltas([[2, 2]], [np.stack([P0[2], P0[2]])], 0, delta))   # not strictly ascending
        raises(1, lambda: m.evaluate_robust_pose_deltas([[3, 1]], [P0[:2]], 0, delta))
        raises(1, lambda: m.evaluate_robust_pose_deltas([[n]], [P0[:1]], 0, delta))                # outside [0, n)
        # a null values: the C call itself
        off, views, masses = np.array([0, 1], np.int32), np.array([2], np.int32), np.full(1, -1.0)
        row = np.ascontiguousarray(P0[3:4])
        rc = _lib.lib().ecc_metric_evaluate_robust_pose_deltas(m._h, 1, C.c_void_p(off.ctypes.data), C.c_void_p(views.ctypes.data),
                                                               C.c_void_p(row.ctypes.data), 0, delta, None, C.c_void_p(masses.ctypes.data))
        assert rc == 1 and masses[0] == -1.0 and _u64(m.evaluate())[()] == _u64(base)[()]
        # ... and a null inlier_masses is allowed
        values = np.zeros(1)
        rc = _lib.lib().ecc_metric_evaluate_robust_pose_deltas(m._h, 1, C.c_void_p(off.ctypes.data), C.c_void_p(views.ctypes.data),
                                                               C.c_void_p(row.ctypes.data), 0, delta, C.c_void_p(values.ctypes.data), None)
        assert rc == 0 and _u64(values[0])[()] == _u64(want[0][0])[()]
        m.useCorrelation(True)
        plain_base, base = base, m.evaluate()                                                      # (what `raises` compares with)
        raises(5, lambda: m.evaluate_robust_pose_deltas([[2]], [P0[3:4]], 0, delta))               # ECC_ERR_UNSUPPORTED
        raises(1, lambda: m.evaluate_robust_pose_deltas([[2]], [P0[3:4]], 3, delta))               # (the loss is checked before it)
        m.useCorrelation(False)
        base = plain_base
        assert _same(m.evaluate_robust_pose_deltas([[2]], [P0[3:4]], 0, delta), want)
        values, masses = m.evaluate_robust_pose_deltas([], [], 0, delta)                           # n_poses < 1: ECC_OK
        assert len(values) == 0 and len(masses) == 0
        assert m.last_batched_poses() == 1                                         # (the call before it; n_poses < 1 returns before the reset)
        here = m.evaluate_robust(0, delta)
        values, masses = m.evaluate_robust_pose_deltas([[]], [np.zeros((0, 12))], 0, delta)        # a pose that moves nothing: the base
        assert _u64(values[0])[()] == _u64(here[0])[()] and _u64(masses[0])[()] == _u64(here[1])[()]
        few = E.MetricRadonIntermediate(gpu_ctx, s.Ps, s.data[:-1])                                # fewer intermediates than views
        s.metrics.append(few)
        with pytest.raises(E.EccError) as e:
            few.evaluate_robust_pose_deltas([[2]], [P0[3:4]], 0, delta)
        assert e.value.code == 1
        one = E.MetricRadonIntermediate(gpu_ctx, s.Ps[:1], s.data[:1])                             # fewer than two views
        s.metrics.append(one)
        with pytest.raises(E.EccError) as e:
            one.evaluate_robust_pose_deltas([[0]], [P0[:1]], 0, delta)
        assert e.value.code == 1
        none = E.MetricRadonIntermediate(gpu_ctx, None, s.data)                                    # no matrices set
        s.metrics.append(none)
        with pytest.raises(E.EccError) as e:
            none.evaluate_robust_pose_deltas([[0]], [P0[:1]], 0, delta)
        assert e.value.code == 1
    finally:
        s.close()
