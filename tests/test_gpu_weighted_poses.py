"""ecc_metric_evaluate_weighted_pose_deltas / ecc_metric_evaluate_weighted_pairs on the GPU (csrc/ecc_weighted_poses.hip,
csrc/weighted_poses_kernel.hip): the metric with per-line weights for pose optimisers -- K poses that each move a few views as one
record / pair / segmented-sum launch each, and index lists.

The data are tests/test_gpu_pose_batch.py's (_scan: seven random intermediates dealt to the views), the weights
tests/weighted_terms.weight_fields (blocks of exactly 0, exactly 1, U(0, 1)), seven fields dealt the same way, the poses that file's
_perturb / _poses pattern.  The contract of the pose call is BITS: values and coverages equal setProjectionMatrices + evaluate_weighted
per pose on a second metric with batching off, whatever the number of pairs (both forms of the sum, with and without a tail, a slice
longer than a chunk), the sampling mode, the moved views, the fallbacks and the batch splitting; and nothing else the metric returns
moves.  Index lists: the rows of evaluate_weighted, the unweighted list's bits at weights 1, and tuples whose matrices and data differ
against the float64 statement of tests/weighted_terms.py."""
import numpy as np
import pytest

import channel_terms as T
import weighted_terms as W
from test_gpu_pose_batch import _perturb, _poses, _scan

pytestmark = pytest.mark.gpu


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


class _Scan:
    """n views: the data of _scan, weight intermediates from `fields` (seven, dealt like the data; None: weight_fields)."""

    def __init__(self, gpu_ctx, n, S=128, B=48, fields=None, per_view=None):
        import epipolarconsistency_amd as E
        self.E, self.ctx, self.n, self.S, self.B = E, gpu_ctx, n, S, B
        self.Ps, self.base, self.data = _scan(gpu_ctx, n, S=S, B=B)
        self.P0 = E.pack_projection_matrices(self.Ps)
        if per_view is not None:     # one field per view
            self.fields = list(per_view)
            self.wbase = [E.RadonIntermediate.from_host(gpu_ctx, f, S, S, filter=E.FILTER_NONE) for f in self.fields]
            self.weights = list(self.wbase)
        else:
            self.fields = W.weight_fields(7, B, B) if fields is None else list(fields)
            self.wbase = [E.RadonIntermediate.from_host(gpu_ctx, f, S, S, filter=E.FILTER_NONE) for f in self.fields]
            self.weights = [self.wbase[v % 7] for v in range(n)]
        self.metrics = []

    def metric(self, mode, batching=True):
        m = self.E.MetricRadonIntermediate(self.ctx, self.Ps, self.data + self.weights).setSampling(mode).setPoseBatching(batching)
        self.metrics.append(m)
        return m

    def close(self):
        for m in self.metrics:
            m.close()
        for d in self.base + self.wbase:
            d.close()


def _sequential(b, poses):
    out = [b.setProjectionMatrices(P).evaluate_weighted() for P in poses]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def _same(got, want):
    return np.array_equal(_u64(got[0]), _u64(want[0])) and np.array_equal(_u64(got[1]), _u64(want[1]))


def _same_pair(x, y):
    """Two (value, coverage) results, bit for bit."""
    return _u64(x[0])[()] == _u64(y[0])[()] and _u64(x[1])[()] == _u64(y[1])[()]


def _moved_of(n):
    def moved_of(k):
        if k % 7 == 3:
            return []                                   # the base itself
        if k % 5 == 0 and n > 4:
            return [k % n, (3 * k + 1) % n, (n - 1 - k) % n, n // 2]   # several, pairs of two moved views among them
        if k % 11 == 6 or k == 2:
            return [n - 1]                              # the last view
        return [(2 * k + 1) % n]
    return moved_of


# ---- 1. sequential bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,mode", [(2, "polynomial"), (3, "auto"), (9, "auto"), (9, "polynomial"), (34, "per_sample"), (67, "polynomial"),
                                    (130, "auto"), (257, "polynomial"), (258, "auto"), (520, "polynomial")])
def test_deltas_have_the_sequential_bits(gpu_ctx, n, mode):
    """Pairs: 1; 3 (tail only); 36 (reference arithmetic under auto, four waves per pair); 561; 2 211 (tail 3); 8 385 (one slice,
    several chunks, tail 1); 32 896 / 33 153 (sixteen slices, without and with a tail); 134 940 (a slice longer than one chunk)."""
    s = _Scan(gpu_ctx, n, S=96 if n > 300 else 128, B=32 if n > 100 else 48)
    try:
        K = 23 if n < 200 else (11 if n < 500 else 3)
        moved_of = _moved_of(n) if n < 500 else (lambda k: [[n - 1], [1, n // 2], []][k])
        poses, views, rows = _poses(s.P0, n, K, moved_of)
        a, b = s.metric(mode), s.metric(mode, batching=False)
        want = _sequential(b, poses)
        before = (a.evaluate_weighted(want_pairs=True), a.evaluate(), a.evaluate_pose_deltas(views[:4], rows[:4]))
        got = a.evaluate_weighted_pose_deltas(views, rows)
        assert _same(got, want), (n, mode, np.flatnonzero(got[0] != want[0]), np.flatnonzero(got[1] != want[1]))
        assert len(set(want[0].tolist())) >= min(K, 3) - 1 and np.all(want[1] > 0) and np.all(want[1] < 1)
        # (a pose that moves view 0 changes the automatic object radius: evaluated the sequential way inside the call)
        assert K - sum(1 for vk in views if 0 in vk) <= a.last_batched_poses() <= K
        # nothing else moved: the weighted value and its rows, evaluate(), a pose batch made before the call
        after = (a.evaluate_weighted(want_pairs=True), a.evaluate(), a.evaluate_pose_deltas(views[:4], rows[:4]))
        assert _u64(after[0][0])[()] == _u64(before[0][0])[()] and _u64(after[0][1])[()] == _u64(before[0][1])[()]
        assert np.array_equal(_u32(after[0][2]), _u32(before[0][2]))
        assert _u64(after[1])[()] == _u64(before[1])[()] and np.array_equal(_u64(after[2]), _u64(before[2]))
        base_w = b.setProjectionMatrices(s.P0).evaluate_weighted()
        assert _same_pair(before[0], base_w)     # the current matrices are still the base
        # a second call from a different base
        P1 = poses[5 % K]
        a.setProjectionMatrices(P1)
        poses2, views2, rows2 = _poses(P1, n, 6 if n < 500 else 2, lambda k: [(5 * k + 2) % n])
        assert _same(a.evaluate_weighted_pose_deltas(views2, rows2), _sequential(b, poses2)), (n, mode)
    finally:
        s.close()


# ---- 2. weights all 1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,mode", [(9, "auto"), (34, "polynomial"), (67, "per_sample")])
def test_ones_are_the_unweighted_pose_deltas(gpu_ctx, n, mode):
    s = _Scan(gpu_ctx, n, fields=[np.ones((48, 48), np.float32)] * 7)
    try:
        poses, views, rows = _poses(s.P0, n, 12, _moved_of(n))
        a = s.metric(mode)
        plain = a.evaluate_pose_deltas(views, rows)
        values, coverages = a.evaluate_weighted_pose_deltas(views, rows)
        assert np.array_equal(_u64(values), _u64(plain)), (values - plain)
        assert np.all(coverages == 1.0) and len(set(plain.tolist())) > 6
    finally:
        s.close()


# ---- 3. a view that does not count -------------------------------------------------------------------------------------------------
def test_a_view_without_weight_can_move_freely(gpu_ctx):
    n, v = 21, 8
    fields = [np.ones((48, 48), np.float32)] * n
    fields[v] = np.zeros((48, 48), np.float32)
    s = _Scan(gpu_ctx, n, per_view=fields)
    try:
        a = s.metric("polynomial")
        base = a.evaluate_weighted()
        poses, views, rows = _poses(s.P0, n, 9, lambda k: [v] if k % 2 == 0 else [(v + k) % n])
        values, coverages = a.evaluate_weighted_pose_deltas(views, rows)
        assert a.last_batched_poses() == 9
        for k in range(9):
            same = _u64(values[k])[()] == _u64(base[0])[()]
            if k % 2 == 0:
                assert same and _u64(coverages[k])[()] == _u64(base[1])[()], (k, values[k], base)
            else:
                assert not same, k
        assert abs(base[1] - (n - 2) / n) < 1e-12    # the share of the pairs without v
    finally:
        s.close()


# ---- 4. fallbacks ------------------------------------------------------------------------------------------------------------------
def test_fallbacks_inside_the_call(gpu_ctx):
    """33 moved views (more than the batch takes), view 0 moved under the automatic radius, batching off: the sequential way inside the
    call, the same bits, the base matrices current afterwards."""
    n = 50
    s = _Scan(gpu_ctx, n)
    try:
        lists = [list(range(1, 34)), [4], [0], [], [9, 30], [0, 7], [49]]
        poses, views, rows = _poses(s.P0, n, len(lists), lambda k: lists[k])
        a, b = s.metric("polynomial"), s.metric("polynomial", batching=False)
        want = _sequential(b, poses)
        base = b.setProjectionMatrices(s.P0).evaluate_weighted()
        got = a.evaluate_weighted_pose_deltas(views, rows)
        assert _same(got, want), (got[0] - want[0], got[1] - want[1])
        # the two poses that move view 0 keep the radius only if it rounds to the base's float: the unweighted call decides the same way
        batched = a.last_batched_poses()
        a.evaluate_pose_deltas(views, rows)
        assert batched == a.last_batched_poses() and 4 <= batched <= 6
        assert _same_pair(a.evaluate_weighted(), base)
        a.setObjectRadius(80.0)
        b.setObjectRadius(80.0)
        want_r = _sequential(b, poses)
        assert _same(a.evaluate_weighted_pose_deltas(views, rows), want_r) and a.last_batched_poses() == 6    # all but the 33 views
        a.setPoseBatching(False)
        assert _same(a.evaluate_weighted_pose_deltas(views, rows), want_r) and a.last_batched_poses() == 0
        base_r = b.setProjectionMatrices(s.P0).evaluate_weighted()
        assert _same_pair(a.evaluate_weighted(), base_r)
    finally:
        s.close()


# ---- 5. batch splitting ------------------------------------------------------------------------------------------------------------
def test_more_entries_than_one_batch_takes(gpu_ctx):
    """3 600 poses of 300 views are 1 080 000 grid entries, more than ECC_POSE_BATCH_MAX_ENTRIES (2^20): two batches (3 495 + 105
    columns) over one base.  Every pose against the same poses in three calls of one batch each; the poses around the cut and every
    41st against the sequential call."""
    n, K = 300, 3600
    s = _Scan(gpu_ctx, n, S=96, B=32)
    try:
        rng = np.random.default_rng(2)
        moved = rng.integers(1, n, size=K).astype(np.int32)
        rows = np.stack([_perturb(s.P0[v], k % 97, int(v)) for k, v in enumerate(moved)])
        a, b = s.metric("polynomial"), s.metric("polynomial", batching=False)
        got = a.evaluate_weighted_pose_deltas_packed(np.arange(K + 1, dtype=np.int32), moved, rows)
        assert a.last_batched_poses() == K
        for lo in range(0, K, 1200):
            part = a.evaluate_weighted_pose_deltas_packed(np.arange(1201, dtype=np.int32), moved[lo:lo + 1200], rows[lo:lo + 1200])
            assert _same((got[0][lo:lo + 1200], got[1][lo:lo + 1200]), part), lo
        which = sorted(set(range(0, K, 41)) | set(range(3490, 3500)) | {K - 1})
        P = s.P0.copy()
        for k in which:
            P[moved[k]] = rows[k]
            want = b.setProjectionMatrices(P).evaluate_weighted()
            P[moved[k]] = s.P0[moved[k]]
            assert _u64(got[0][k])[()] == _u64(want[0])[()] and _u64(got[1][k])[()] == _u64(want[1])[()], k
    finally:
        s.close()


# ---- 6. index lists ----------------------------------------------------------------------------------------------------------------
def _pair_index(i, j, n):
    return i * n - i * (i + 1) // 2 + (j - i - 1)


@pytest.mark.parametrize("mode", ["polynomial", "per_sample", "reference"])
def test_list_rows_are_the_all_pairs_rows(gpu_ctx, mode):
    """(a) tuples (i, j, i, j), shuffled, with duplicates: the get_ij rows of evaluate_weighted under the same explicit mode."""
    n = 12
    s = _Scan(gpu_ctx, n)
    try:
        m = s.metric(mode)
        _, _, full = m.evaluate_weighted(want_pairs=True)
        rng = np.random.default_rng(4)
        ij = np.array([(i, j) for i in range(n) for j in range(i + 1, n)])
        pick = np.concatenate([rng.permutation(len(ij)), rng.integers(0, len(ij), 30)])
        idx = np.array([(i, j, i, j) for i, j in ij[pick]], np.int32)
        value, coverage, rows = m.evaluate_weighted_pairs(idx, want_pairs=True)
        assert rows.shape == (len(idx), 2) and rows.dtype == np.float32
        assert np.array_equal(_u32(rows), _u32(full[[_pair_index(i, j, n) for i, j in ij[pick]]])), mode
        # (d) value and coverage are the sums of the rows
        sc, su = rows[:, 0].astype(np.float64).sum(), rows[:, 1].astype(np.float64).sum()
        assert abs(value - sc / su) <= 1e-12 * abs(sc / su) and abs(coverage - su / len(idx)) <= 1e-12 * su / len(idx)
        assert m.evaluate_weighted_pairs(idx) == (value, coverage)
        assert np.array_equal(_u32(m.evaluate_weighted(want_pairs=True)[2]), _u32(full))
    finally:
        s.close()


def test_ones_are_the_unweighted_list(gpu_ctx):
    """(b) weights all 1, list lengths around the auto threshold (512) and with every tail: the c column and sum c / n_pairs have the
    bits of evaluate(indices, out) of the same list; u and coverage are 1."""
    n = 67
    s = _Scan(gpu_ctx, n, fields=[np.ones((48, 48), np.float32)] * 7)
    try:
        m = s.metric("auto")
        rng = np.random.default_rng(9)
        ij = np.array([(i, j) for i in range(n) for j in range(i + 1, n)])
        ij = ij[rng.permutation(len(ij))]
        for length in (1, 3, 511, 513, 2211):
            idx = np.ascontiguousarray([(i, j, i, j) for i, j in ij[:length]], np.int32)
            out = np.zeros(length, np.float32)
            mean = m.evaluate(idx, out)
            value, coverage, rows = m.evaluate_weighted_pairs(idx, want_pairs=True)
            assert np.array_equal(_u32(rows[:, 0]), _u32(out)), (length, np.max(np.abs(rows[:, 0] - out)))
            assert _u64(value)[()] == _u64(mean)[()], (length, value, mean)
            assert np.all(rows[:, 1] == 1.0) and coverage == 1.0 and mean > 0
    finally:
        s.close()


@pytest.mark.parametrize("mode", ["reference", "polynomial"])
def test_weights_follow_the_data_index(gpu_ctx, oracle_mod, mode):
    """(c) tuples (a, b, c, d): the matrices of views a, b with the data AND weights of views c, d, against weighted_terms.pair_terms
    with the pair geometry of (a, b) from debug_K01: 1e-6 of the scale under the reference arithmetic, 1e-3 on the throughput path.
    The same comparison rejects weights taken from dtr n + P (views a, b) by the printed ratio; the views are chosen so that every
    tuple's weight fields differ between P and D (the seven fields are dealt v % 7)."""
    n = 16
    s = _Scan(gpu_ctx, n)
    try:
        m = s.metric(mode)
        tuples = [(0, 5, 2, 10), (3, 4, 8, 6), (1, 14, 13, 3), (7, 9, 9, 4), (2, 11, 5, 15), (6, 12, 0, 1)]
        for a, b, c, d in tuples:
            assert a < b and (a % 7, b % 7) != (c % 7, d % 7) and a % 7 != c % 7
        idx = np.array(tuples, np.int32)
        value, coverage, rows = m.evaluate_weighted_pairs(idx, want_pairs=True)
        data = [x.readback() for x in s.base]
        want, slip, scales = [], [], []
        for a, b, c, d in tuples:
            K01 = m.debug_K01(_pair_index(a, b, n), 1)[0]
            t = W.pair_terms(K01, data[c % 7], data[d % 7], s.fields[c % 7], s.fields[d % 7], s.S, s.S)
            w = W.pair_terms(K01, data[c % 7], data[d % 7], s.fields[a % 7], s.fields[b % 7], s.S, s.S)
            assert t["n_kappa"] > 8
            want.append((t["c"], t["u"]))
            slip.append((w["c"], w["u"]))
            scales.append((t["s"], 1.0))
        want, slip, scales = np.array(want), np.array(slip), np.array(scales)
        tol = T.tolerance(mode, len(tuples))
        ratio = T.compare(rows, want, scales, tol)
        rejected = T.compare(slip, want, scales, tol)
        print("%s: c %.3g of the bar %.0e, u %.3g; weights from dtr n + P are rejected %.3g-fold (c) and %.3g-fold (u)"
              % (mode, ratio[0], tol, ratio[1], rejected[0], rejected[1]))
        assert ratio.max() <= 1.0, (mode, ratio)
        assert rejected.min() > 10.0, (mode, rejected)     # the oracle alone separates the two by well over the bar
        # (d)
        sc, su = rows[:, 0].astype(np.float64).sum(), rows[:, 1].astype(np.float64).sum()
        assert abs(value - sc / su) <= 1e-12 * abs(sc / su) and abs(coverage - su / len(idx)) <= 1e-12 * su / len(idx)
    finally:
        s.close()


# ---- 7. argument errors ------------------------------------------------------------------------------------------------------------
def test_errors(gpu_ctx):
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib
    n = 6
    s = _Scan(gpu_ctx, n)
    try:
        m = s.metric("polynomial")
        P0 = s.P0
        idx = np.array([[0, 1, 0, 1], [2, 5, 2, 5]], np.int32)
        want = m.evaluate_weighted_pairs(idx, want_pairs=True)
        want_p = m.evaluate_weighted_pose_deltas([[2]], [P0[3:4]])

        def raises(code, call):
            with pytest.raises(E.EccError) as e:
                call()
            assert e.value.code == code, e.value
        for bad in ([0, 1, 0, n], [0, 1, n, 1], [0, n, 0, 1], [-1, 1, 0, 1], [0, 1, 0, 2 * n - 1]):   # D in the weights' range: refused
            raises(1, lambda: m.evaluate_weighted_pairs(np.array([idx[0], bad], np.int32)))
        raises(1, lambda: m.evaluate_weighted_pose_deltas([[2, 2]], [np.stack([P0[2], P0[2]])]))   # not strictly ascending
        raises(1, lambda: m.evaluate_weighted_pose_deltas([[n]], [P0[:1]]))                        # outside [0, n)
        raises(1, lambda: m.evaluate_weighted_pose_deltas([[3, 1]], [P0[:2]]))
        assert m.evaluate_weighted_pairs(np.zeros((0, 4), np.int32)) == (0.0, 0.0)                 # n_pairs == 0: ECC_OK, nothing written
        assert m.last_batched_poses() == 1                                                         # (want_p's pose)
        values, coverages = m.evaluate_weighted_pose_deltas([], [])
        assert len(values) == 0 and len(coverages) == 0
        assert m.last_batched_poses() == 1                                                         # n_poses < 1 returns before the count is reset
        with pytest.raises(E.EccError) as e:
            m.evaluate_weighted_pairs(np.array([idx[0], [0, 1, 0, n]], np.int32))
        assert str(e.value).endswith("(matrices and data intermediates lie in [0, n_views))")    # the weighted lists' own text
        L, empty = _lib.lib(), np.zeros((0, 4), np.int32)
        assert L.ecc_metric_evaluate_weighted_pairs(m._h, None, -1, None, None, None) == 1 and b"value is null" in L.ecc_last_error()
        base = m.evaluate_weighted()
        values, coverages = m.evaluate_weighted_pose_deltas([[]], [np.zeros((0, 12))])             # a pose that moves nothing: the base
        assert _u64(values[0])[()] == _u64(base[0])[()] and _u64(coverages[0])[()] == _u64(base[1])[()]
        degenerate = m.evaluate_weighted_pairs(np.array([[1, 1, 1, 1], [0, 1, 0, 1]], np.int32), want_pairs=True)[2]
        assert tuple(degenerate[0]) == (0.0, 1.0) and np.array_equal(_u32(degenerate[1]), _u32(want[2][0]))   # no samples: {0, 1}
        m.useCorrelation(True)
        raises(5, lambda: m.evaluate_weighted_pairs(idx))                                          # ECC_ERR_UNSUPPORTED
        raises(5, lambda: m.evaluate_weighted_pose_deltas([[2]], [P0[3:4]]))
        assert m.evaluate_weighted_pairs(empty) == (0.0, 0.0)          # n_pairs == 0 returns before the metric's state is looked at
        m.useCorrelation(False)
        again = m.evaluate_weighted_pairs(idx, want_pairs=True)
        assert again[:2] == want[:2] and np.array_equal(_u32(again[2]), _u32(want[2]))
        assert _same(m.evaluate_weighted_pose_deltas([[2]], [P0[3:4]]), want_p)
        for dtrs in (s.data, s.data + s.weights[:-1], s.data + s.weights + s.weights[:1]):        # n, 2 n - 1, 2 n + 1 intermediates
            bad = E.MetricRadonIntermediate(gpu_ctx, s.Ps, dtrs)
            raises(1, lambda: bad.evaluate_weighted_pairs(idx))
            raises(1, lambda: bad.evaluate_weighted_pose_deltas([[2]], [P0[3:4]]))
            assert bad.evaluate_weighted_pairs(empty) == (0.0, 0.0)
            bad.close()
        one = E.MetricRadonIntermediate(gpu_ctx, s.Ps[:1], [s.data[0], s.weights[0]])              # fewer than two views
        raises(1, lambda: one.evaluate_weighted_pairs(np.array([[0, 0, 0, 0]], np.int32)))
        raises(1, lambda: one.evaluate_weighted_pose_deltas([[0]], [P0[:1]]))
        assert one.evaluate_weighted_pairs(empty) == (0.0, 0.0)
        one.close()
        none = E.MetricRadonIntermediate(gpu_ctx, None, s.data + s.weights)                       # no matrices set
        raises(1, lambda: none.evaluate_weighted_pairs(idx))
        raises(1, lambda: none.evaluate_weighted_pose_deltas([[0]], [P0[:1]]))
        assert none.evaluate_weighted_pairs(empty) == (0.0, 0.0)
        none.close()
    finally:
        s.close()
