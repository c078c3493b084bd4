"""ecc_metric_evaluate_robust_transforms on the GPU (csrc/ecc_robust_batches.hip): the metric under a per-sample robust loss for the
registration of two scans -- K rigid source-to-target transforms as ONE compose / E1 / list launch, ONE record launch, ONE robust pair
launch and ONE segmented sum of the columns c and u.

The scans, cross lists and transforms are tests/test_gpu_transforms.py's.  delta = robust_scale(the base's cross-list rows, 0.5), so
about half the pairs have residuals beyond it.  The contract is BITS: values, inlier masses and pair terms {c, u, r} equal
setProjectionMatrices(composed matrices) + evaluate_robust_pairs(the cross list) per transform on a second metric -- whatever the list
length (one pair, the reference arithmetic's bound, the sixteen-slice sum), the sampling mode, the loss and the object radius (under
the automatic one every transform has its OWN); with delta = inf the values are evaluate_transforms'; batching off gives the same
bits; the call leaves the metric as it found it."""
import numpy as np
import pytest

from test_gpu_transforms import _composed, _configure, _cross_list, _scan, _transforms

pytestmark = pytest.mark.gpu
INF = float("inf")


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


class _Scan:
    def __init__(self, gpu_ctx, n, B=48):
        import epipolarconsistency_amd as E
        self.E, self.ctx, self.n = E, gpu_ctx, n
        self.Ps, self.base, self.data = _scan(gpu_ctx, n, B=B)
        self.metrics = []

    def metric(self, mode, radius=0.0, dkappa=0.0):
        m = self.E.MetricRadonIntermediate(self.ctx, self.Ps, self.data)
        self.metrics.append(m)
        return _configure(m, mode, radius, dkappa)

    def delta(self, m, ns, nt):
        """robust_scale of the cross list's rows at the metric's current matrices, k = 0.5, as the float32 the calls take"""
        rows = m.evaluate_robust_pairs(_cross_list(ns, nt), 0, INF, want_pairs=True)[2]
        return float(np.float32(self.E.robust_scale(rows, 0.5)))

    def close(self):
        for m in self.metrics:
            m.close()
        for d in self.base:
            d.close()


def _sequential(b, Ps, ns, nt, Ts, loss, delta):
    """What a caller without the entry point does: per transform setProjectionMatrices + evaluate_robust_pairs of the cross list."""
    idx = _cross_list(ns, nt)
    values, masses, pairs = np.zeros(len(Ts)), np.zeros(len(Ts)), np.zeros((len(Ts), nt, ns, 3), np.float32)
    for k, Tk in enumerate(Ts):
        values[k], masses[k], rows = b.setProjectionMatrices(_composed(Ps, ns, Tk)).evaluate_robust_pairs(idx, loss, delta, want_pairs=True)
        pairs[k] = rows.reshape(nt, ns, 3)
    b.setProjectionMatrices(Ps)
    return values, masses, pairs


def _same(got, want):
    return all(np.array_equal(_u64(g), _u64(w)) for g, w in zip(got[:2], want[:2])) and \
        (len(got) < 3 or np.array_equal(_u32(got[2]), _u32(want[2])))


CASES = [
    # (n_source, n_target, mode, radius, loss)
    (1, 1, "auto", 0.0, 0), (1, 1, "polynomial", 80.0, 1),   # one pair
    (2, 3, "polynomial", 0.0, 1), (2, 3, "auto", 90.0, 2),
    (5, 7, "auto", 0.0, 2), (5, 7, "auto", 75.0, 0),         # 35 tuples: the reference arithmetic under auto
    (20, 26, "auto", 0.0, 0), (20, 26, "per_sample", 75.0, 1),   # 520: just past the 512-tuple switch
    (180, 183, "auto", 0.0, 1), (180, 183, "polynomial", 100.0, 2),   # 32 940 values: the sixteen-slice sum
]


# ---- (a) - (c): sequential bits, delta = inf, not vacuous --------------------------------------------------------------------------
@pytest.mark.parametrize("ns,nt,mode,radius,loss", CASES)
def test_transforms_have_the_sequential_bits(gpu_ctx, ns, nt, mode, radius, loss):
    n = ns + nt
    s = _Scan(gpu_ctx, n, B=32 if n > 100 else 48)
    try:
        # 17 transforms; at the largest size three of them: a rotation, a translation that changes the automatic radius, and it again
        Ts = _transforms(17) if n < 200 else [_transforms(5)[q] for q in (2, 3, 3)]
        K = len(Ts)
        a, b = s.metric(mode, radius), s.metric(mode, radius)
        if radius == 0.0:
            # the automatic radius follows the COMPOSED view 0: the case tests the per-transform radius only if they differ
            radii = {np.float32(s.E.host_object_radius(_composed(s.Ps, ns, Tk)[0], 128, 128)) for Tk in Ts}
            assert len(radii) >= 2, radii
        delta = s.delta(a, ns, nt)
        assert 0.0 < delta < INF
        want = _sequential(b, s.Ps, ns, nt, Ts, loss, delta)
        got = a.evaluate_robust_transforms(ns, Ts, loss, delta, want_pairs=True)
        # (a)
        assert a.last_batched_transforms() == K
        assert got[2].shape == (K, nt, ns, 3) and got[2].dtype == np.float32 and got[0].dtype == got[1].dtype == np.float64
        assert np.array_equal(_u32(got[2]), _u32(want[2])), (np.argwhere(got[2] != want[2])[:5], np.abs(got[2] - want[2]).max())
        assert np.array_equal(_u64(got[0]), _u64(want[0])), (np.flatnonzero(got[0] != want[0]), (got[0] - want[0])[got[0] != want[0]])
        assert np.array_equal(_u64(got[1]), _u64(want[1])), (np.flatnonzero(got[1] != want[1]), (got[1] - want[1])[got[1] != want[1]])
        assert got[0][-1] == got[0][-2] and got[1][-1] == got[1][-2] and np.array_equal(got[2][-1], got[2][-2])   # two equal transforms
        # the values alone (no pair terms), and again in reverse order from whatever state the call left
        assert _same(a.evaluate_robust_transforms(ns, Ts, loss, delta), want[:2])
        back = a.evaluate_robust_transforms(ns, Ts[::-1], loss, delta, want_pairs=True)
        assert _same(back, (want[0][::-1], want[1][::-1], want[2][::-1])) and a.last_batched_transforms() == K
        # (b) delta = inf: evaluate_transforms' bits (means and pair values), every u and every mass exactly 1
        means, vals = a.evaluate_transforms(ns, Ts, want_pairs=True)
        at_inf = a.evaluate_robust_transforms(ns, Ts, loss, INF, want_pairs=True)
        assert np.array_equal(_u64(at_inf[0]), _u64(means)), (at_inf[0] - means)
        assert np.array_equal(_u32(at_inf[2][..., 0]), _u32(vals))
        assert np.all(at_inf[1] == 1.0) and np.all(at_inf[2][..., 1] == 1.0)
        assert np.array_equal(_u32(at_inf[2][..., 2]), _u32(got[2][..., 2]))    # r knows neither loss nor delta
        # (c) the loss is seen (lists of a few tuples: at least no mass outside (0, 1])
        assert np.all(got[1] <= 1.0) and np.all(got[1] > 0.0) and np.all(got[0] > 0.0), got
        if ns * nt >= 35:
            assert np.all(got[1] < 1.0), got[1]
            assert np.all(got[0] != means), (got[0], means)
    finally:
        s.close()


# ---- (d) the sequential fallback ---------------------------------------------------------------------------------------------------
def test_batching_off_goes_the_sequential_way(gpu_ctx):
    """setPoseBatching(False): the sequential way inside the call, same bits, nothing batched, the base matrices current again.  (A
    list longer than a batch needs more than 2^20 tuples per transform: no hook makes a batch smaller, so that branch -- the same
    function -- is not run here.)"""
    ns, nt, loss = 9, 6, 2
    s = _Scan(gpu_ctx, ns + nt)
    try:
        Ts = _transforms(6)
        a, b = s.metric("auto"), s.metric("auto")
        delta = s.delta(a, ns, nt)
        want = _sequential(b, s.Ps, ns, nt, Ts, loss, delta)
        before = (a.evaluate(), a.evaluate_robust(loss, delta))
        assert _same(a.evaluate_robust_transforms(ns, Ts, loss, delta, want_pairs=True), want) and a.last_batched_transforms() == 6
        a.setPoseBatching(False)
        assert _same(a.evaluate_robust_transforms(ns, Ts, loss, delta, want_pairs=True), want) and a.last_batched_transforms() == 0
        assert _same(a.evaluate_robust_transforms(ns, Ts, loss, delta), want[:2]) and a.last_batched_transforms() == 0
        assert [np.array_equal(x, y) for x, y in zip(a.getProjectionMatrices(), s.Ps)] == [True] * (ns + nt)
        assert (a.evaluate(), a.evaluate_robust(loss, delta)) == before
        a.setPoseBatching(True)
        one = a.evaluate_robust_transforms(ns, Ts[1], loss, delta)   # a single (4, 4) matrix
        assert one[0].shape == (1,) and _u64(one[0][0])[()] == _u64(want[0][1])[()] and a.last_batched_transforms() == 1
    finally:
        s.close()


# ---- (e) the metric is left as found -----------------------------------------------------------------------------------------------
def test_the_metric_is_left_as_found(gpu_ctx):
    """evaluate() (record reuse on: the kept records are neither used for the batch nor overwritten by it), evaluate_robust() with its
    rows and an evaluate_pose_deltas made before the call give the same bits after it; the current matrices are unchanged; one view
    moved afterwards refits from the kept records as if the batch had not happened."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import geometry
    ns, nt, loss = 60, 52, 0
    n = ns + nt   # 6 216 pairs: above ECC_RECORD_REUSE_MIN_PAIRS
    s = _Scan(gpu_ctx, n)
    try:
        Ts = _transforms(7)
        P0 = E.pack_projection_matrices(s.Ps)
        P1 = P0.copy()
        P1[5] = (P0[5].reshape(4, 3).T @ geometry.rigid_transform(tx=0.3, rz=0.001)).T.reshape(12)
        views = [[3], [7, 9], [n - 1]]
        rows = [np.stack([(P0[v].reshape(4, 3).T @ geometry.rigid_transform(tx=0.2 * (q + 1), ry=0.002)).T.reshape(12) for v in vk])
                for q, vk in enumerate(views)]
        a, ref, seq = s.metric("polynomial").setRecordReuse(True, always=True), s.metric("polynomial").setRecordReuse(True, always=True), \
            s.metric("polynomial")
        delta = s.delta(seq, ns, nt)
        want = _sequential(seq, s.Ps, ns, nt, Ts, loss, delta)

        def observe(m):
            w = m.evaluate_robust(loss, delta, want_pairs=True)
            return np.concatenate([[m.evaluate(), w[0], w[1]], m.evaluate_pose_deltas(views, rows)]), w[2]
        before, rows_before = observe(a)
        assert _u64(before[0])[()] == _u64(ref.evaluate())[()]
        assert _same(a.evaluate_robust_transforms(ns, Ts, loss, delta, want_pairs=True), want) and a.last_batched_transforms() == len(Ts)
        assert [np.array_equal(x, y) for x, y in zip(a.getProjectionMatrices(), s.Ps)] == [True] * n
        after, rows_after = observe(a)
        assert np.array_equal(_u64(before), _u64(after)) and np.array_equal(_u32(rows_before), _u32(rows_after))
        # straight after a batch, without anything in between
        assert _same(a.evaluate_robust_transforms(ns, Ts[:3], loss, delta), (want[0][:3], want[1][:3]))
        assert _u64(a.evaluate())[()] == _u64(before[0])[()]
        # one view moves: the reuse path refits its pairs from the kept records
        assert _u64(a.setProjectionMatrices(P1).evaluate())[()] == _u64(ref.setProjectionMatrices(P1).evaluate())[()]
        assert _u64(a.setProjectionMatrices(P0).evaluate())[()] == _u64(before[0])[()]
    finally:
        s.close()


# ---- errors on a live metric -------------------------------------------------------------------------------------------------------
def test_errors_on_a_live_metric(gpu_ctx):
    import epipolarconsistency_amd as E
    ns, nt = 3, 2
    s = _Scan(gpu_ctx, ns + nt)
    try:
        Ts = _transforms(4)
        m = s.metric("auto")
        delta = s.delta(m, ns, nt)
        base = m.evaluate()
        want = m.evaluate_robust_transforms(ns, Ts, 0, delta, want_pairs=True)

        def raises(code, call, text=None):
            with pytest.raises(E.EccError) as e:
                call()
            assert e.value.code == code and (text is None or text in str(e.value)), e.value
        # no transforms: nothing happens, after the other checks
        empty = m.evaluate_robust_transforms(ns, np.zeros((0, 4, 4)), 0, delta, want_pairs=True)
        assert empty[0].shape == empty[1].shape == (0,) and empty[2].shape == (0, nt, ns, 3) and m.last_batched_transforms() == 0
        for bad_ns in (0, -1, ns + nt, ns + nt + 3):
            for Tk in (Ts, np.zeros((0, 4, 4))):
                raises(1, lambda: m.evaluate_robust_transforms(bad_ns, Tk, 0, delta), "n_source")
        for loss, d in ((3, delta), (-1, delta), (0, 0.0), (1, -2.0), (2, float("nan"))):
            raises(1, lambda: m.evaluate_robust_transforms(ns, Ts, loss, d))
            raises(1, lambda: m.evaluate_robust_transforms(0, Ts, loss, d))        # ... which come before n_source
        m.useCorrelation(True)
        raises(5, lambda: m.evaluate_robust_transforms(ns, Ts, 0, delta))          # ECC_ERR_UNSUPPORTED
        raises(5, lambda: m.evaluate_robust_transforms(0, Ts, 0, delta))           # ... which comes before n_source
        m.useCorrelation(False)
        assert _same(m.evaluate_robust_transforms(ns, Ts, 0, delta, want_pairs=True), want)
        assert _u64(m.evaluate())[()] == _u64(base)[()]
        few = E.MetricRadonIntermediate(gpu_ctx, s.Ps, s.data[:-1])                # fewer intermediates than views
        none = E.MetricRadonIntermediate(gpu_ctx, None, s.data)                    # no matrices set
        s.metrics += [few, none]
        raises(1, lambda: few.evaluate_robust_transforms(ns, Ts, 0, delta))
        raises(1, lambda: none.evaluate_robust_transforms(ns, Ts, 0, delta))
    finally:
        s.close()
