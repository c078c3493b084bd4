"""ecc_metric_evaluate_weighted_robust_transforms on the GPU (csrc/ecc_weighted_robust_batches.hip, csrc/form_sums_kernel.hip): line
weights and the robust loss together for the registration of two scans -- K rigid source-to-target transforms as ONE compose / E1 /
list launch, ONE record launch, ONE weighted-robust pair launch and ONE segmented sum of the columns c, u and k.

The scans, weights, cross lists and transforms are tests/test_gpu_weighted_transforms.py's and tests/test_gpu_transforms.py's.  delta =
weighted_robust_scale(the base's cross-list rows at delta = inf, 0.5) as a float32.  The contract is BITS: values, coverages, inlier
masses and pair terms {c, u, k, r} equal setProjectionMatrices(composed matrices) + evaluate_weighted_robust_pairs(the cross list) per
transform on a second metric -- whatever the list length (one pair, the reference arithmetic's bound, the sixteen-slice sum without and
with a tail), the sampling mode, the loss and the object radius (under the automatic one every transform has its OWN); with delta = inf
the results are evaluate_weighted_transforms', with weights of one evaluate_robust_transforms'; batching off gives the same bits; the
call leaves the metric as it found it."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_robust_transforms import CASES as ROBUST_CASES
from test_gpu_transforms import _composed, _cross_list, _transforms
from test_gpu_weighted_transforms import _Scan

pytestmark = pytest.mark.gpu
INF = float("inf")


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _delta(s, m, ns, nt):
    """weighted_robust_scale of the cross list's rows at the metric's current matrices, k = 0.5, as the float32 the calls take"""
    rows = m.evaluate_weighted_robust_pairs(_cross_list(ns, nt), 0, INF, want_pairs=True)[3]
    return float(np.float32(s.E.weighted_robust_scale(rows, 0.5)))


def _sequential(b, Ps, ns, nt, Ts, loss, delta):
    """What a caller without the entry point does: per transform setProjectionMatrices + evaluate_weighted_robust_pairs of the cross list."""
    idx = _cross_list(ns, nt)
    K = len(Ts)
    values, coverages, masses, pairs = np.zeros(K), np.zeros(K), np.zeros(K), np.zeros((K, nt, ns, 4), np.float32)
    for k, Tk in enumerate(Ts):
        values[k], coverages[k], masses[k], rows = \
            b.setProjectionMatrices(_composed(Ps, ns, Tk)).evaluate_weighted_robust_pairs(idx, loss, delta, want_pairs=True)
        pairs[k] = rows.reshape(nt, ns, 4)
    b.setProjectionMatrices(Ps)
    return values, coverages, masses, pairs


def _same(got, want):
    return all(np.array_equal(_u64(g), _u64(w)) for g, w in zip(got[:3], want[:3])) and \
        (len(got) < 4 or np.array_equal(_u32(got[3]), _u32(want[3])))


# (n_source, n_target, mode, radius, loss): the robust file's, and 33 123 tuples -- sixteen slices with a tail of 3
CASES = ROBUST_CASES + [(181, 183, "polynomial", 0.0, 0)]


@pytest.mark.parametrize("ns,nt,mode,radius,loss", CASES)
def test_transforms_have_the_sequential_bits(gpu_ctx, ns, nt, mode, radius, loss):
    n = ns + nt
    s = _Scan(gpu_ctx, n, B=32 if n > 100 else 48)
    try:
        # 17 transforms; at the largest sizes three of them: a rotation, a translation that changes the automatic radius, and it again
        Ts = _transforms(17) if n < 200 else [_transforms(5)[q] for q in (2, 3, 3)]
        K = len(Ts)
        a, b = s.metric(mode, radius), s.metric(mode, radius)
        if radius == 0.0:
            # the automatic radius follows the COMPOSED view 0: the case tests the per-transform radius only if they differ
            radii = {np.float32(s.E.host_object_radius(_composed(s.Ps, ns, Tk)[0], 128, 128)) for Tk in Ts}
            assert len(radii) >= 2, radii
        delta = _delta(s, a, ns, nt)
        assert 0.0 < delta < INF
        want = _sequential(b, s.Ps, ns, nt, Ts, loss, delta)
        got = a.evaluate_weighted_robust_transforms(ns, Ts, loss, delta, want_pairs=True)
        assert a.last_batched_transforms() == K
        assert len(got) == 4 and got[3].shape == (K, nt, ns, 4) and got[3].dtype == np.float32
        assert got[0].dtype == got[1].dtype == got[2].dtype == np.float64
        assert np.array_equal(_u32(got[3]), _u32(want[3])), (np.argwhere(got[3] != want[3])[:5], np.abs(got[3] - want[3]).max())
        for q in range(3):
            assert np.array_equal(_u64(got[q]), _u64(want[q])), (q, np.flatnonzero(got[q] != want[q]), (got[q] - want[q])[got[q] != want[q]])
        assert all(got[q][-1] == got[q][-2] for q in range(3)) and np.array_equal(got[3][-1], got[3][-2])   # two equal transforms
        # the results alone (no pair terms), and again in reverse order from whatever state the call left
        alone = a.evaluate_weighted_robust_transforms(ns, Ts, loss, delta)
        assert len(alone) == 3 and _same(alone, want[:3])
        back = a.evaluate_weighted_robust_transforms(ns, Ts[::-1], loss, delta, want_pairs=True)
        assert _same(back, tuple(w[::-1] for w in want)) and a.last_batched_transforms() == K
        # delta = inf: evaluate_weighted_transforms' bits (values, coverages, {c, u}), k has the bits of u, every mass exactly 1
        weighted = a.evaluate_weighted_transforms(ns, Ts, want_pairs=True)
        at_inf = a.evaluate_weighted_robust_transforms(ns, Ts, loss, INF, want_pairs=True)
        assert np.array_equal(_u64(at_inf[0]), _u64(weighted[0])) and np.array_equal(_u64(at_inf[1]), _u64(weighted[1]))
        assert np.array_equal(_u32(at_inf[3][..., :2]), _u32(weighted[2]))
        assert np.array_equal(_u32(at_inf[3][..., 2]), _u32(at_inf[3][..., 1])) and np.all(at_inf[2] == 1.0)
        assert np.array_equal(_u32(at_inf[3][..., 3]), _u32(got[3][..., 3]))    # r knows neither loss nor delta
        # weights and loss are seen (lists of a few tuples: at least nothing outside (0, 1])
        assert np.all(got[1] > 0.0) and np.all(got[1] <= 1.0) and np.all(got[2] > 0.0) and np.all(got[2] <= 1.0) and np.all(got[0] > 0.0), got[:3]
        if ns * nt >= 35:
            assert np.all(got[1] < 1.0) and np.all(got[2] < 1.0), got[1:3]
            assert np.all(got[0] != weighted[0]), (got[0], weighted[0])
    finally:
        s.close()


@pytest.mark.parametrize("ns,nt,mode,loss", [(3, 2, "auto", 0), (20, 26, "polynomial", 1), (67, 33, "per_sample", 2)])
def test_ones_are_the_robust_transforms(gpu_ctx, ns, nt, mode, loss):
    """Every weight 1.0f: values, inlier masses and the columns {c, k, r} have the bits of evaluate_robust_transforms' values, masses
    and {c, u, r} on a metric of the data alone; every u and every coverage is 1.0."""
    s = _Scan(gpu_ctx, ns + nt, fields=[np.ones((48, 48), np.float32)] * 7)
    try:
        Ts = _transforms(9)
        a, plain = s.metric(mode), s.metric(mode, dtrs=s.data)
        delta = _delta(s, a, ns, nt)
        robust = plain.evaluate_robust_transforms(ns, Ts, loss, delta, want_pairs=True)
        got = a.evaluate_weighted_robust_transforms(ns, Ts, loss, delta, want_pairs=True)
        assert a.last_batched_transforms() == plain.last_batched_transforms() == 9
        assert np.array_equal(_u64(got[0]), _u64(robust[0])), (got[0], robust[0])
        assert np.array_equal(_u64(got[2]), _u64(robust[1])), (got[2], robust[1])
        assert np.array_equal(_u32(got[3][..., [0, 2, 3]]), _u32(robust[2]))
        assert np.all(got[3][..., 1] == 1.0) and np.all(got[1] == 1.0)
        if ns * nt >= 35:
            assert np.all(got[2] < 1.0)
    finally:
        s.close()


def test_batching_off_goes_the_sequential_way(gpu_ctx):
    """setPoseBatching(False): the sequential way inside the call, same bits, nothing batched, the base matrices current again.  (A
    list longer than a batch needs more than 2^20 tuples per transform: no hook makes a batch smaller, so that branch -- the same
    function -- is not run here.)"""
    ns, nt, loss = 9, 6, 2
    s = _Scan(gpu_ctx, ns + nt)
    try:
        Ts = _transforms(6)
        a, b = s.metric("auto"), s.metric("auto")
        delta = _delta(s, a, ns, nt)
        want = _sequential(b, s.Ps, ns, nt, Ts, loss, delta)
        before = (a.evaluate(), a.evaluate_weighted_robust(loss, delta))
        assert _same(a.evaluate_weighted_robust_transforms(ns, Ts, loss, delta, want_pairs=True), want) and a.last_batched_transforms() == 6
        a.setPoseBatching(False)
        assert _same(a.evaluate_weighted_robust_transforms(ns, Ts, loss, delta, want_pairs=True), want) and a.last_batched_transforms() == 0
        assert _same(a.evaluate_weighted_robust_transforms(ns, Ts, loss, delta), want[:3]) and a.last_batched_transforms() == 0
        assert [np.array_equal(x, y) for x, y in zip(a.getProjectionMatrices(), s.Ps)] == [True] * (ns + nt)
        assert (a.evaluate(), a.evaluate_weighted_robust(loss, delta)) == before
        a.setPoseBatching(True)
        one = a.evaluate_weighted_robust_transforms(ns, Ts[1], loss, delta)   # a single (4, 4) matrix
        assert one[0].shape == (1,) and all(_u64(one[q][0])[()] == _u64(want[q][1])[()] for q in range(3)) and a.last_batched_transforms() == 1
    finally:
        s.close()


def test_the_metric_is_left_as_found(gpu_ctx):
    """evaluate() (record reuse on: the kept records are neither used for the batch nor overwritten by it), evaluate_weighted_robust()
    with its rows and an evaluate_pose_deltas made before the call give the same bits after it; the current matrices are unchanged; one
    view moved afterwards refits from the kept records as if the batch had not happened."""
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
        delta = _delta(s, seq, ns, nt)
        want = _sequential(seq, s.Ps, ns, nt, Ts, loss, delta)

        def observe(m):
            w = m.evaluate_weighted_robust(loss, delta, want_pairs=True)
            return np.concatenate([[m.evaluate(), w[0], w[1], w[2]], m.evaluate_pose_deltas(views, rows)]), w[3]
        before, rows_before = observe(a)
        assert _u64(before[0])[()] == _u64(ref.evaluate())[()]
        assert _same(a.evaluate_weighted_robust_transforms(ns, Ts, loss, delta, want_pairs=True), want) and a.last_batched_transforms() == len(Ts)
        assert [np.array_equal(x, y) for x, y in zip(a.getProjectionMatrices(), s.Ps)] == [True] * n
        after, rows_after = observe(a)
        assert np.array_equal(_u64(before), _u64(after)) and np.array_equal(_u32(rows_before), _u32(rows_after))
        # straight after a batch, without anything in between
        assert _same(a.evaluate_weighted_robust_transforms(ns, Ts[:3], loss, delta), tuple(w[:3] for w in want[:3]))
        assert _u64(a.evaluate())[()] == _u64(before[0])[()]
        # one view moves: the reuse path refits its pairs from the kept records
        assert _u64(a.setProjectionMatrices(P1).evaluate())[()] == _u64(ref.setProjectionMatrices(P1).evaluate())[()]
        assert _u64(a.setProjectionMatrices(P0).evaluate())[()] == _u64(before[0])[()]
    finally:
        s.close()


def test_errors_on_a_live_metric(gpu_ctx):
    """Every documented error, through the C call with its outputs preset: the code, and nothing written."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib
    ns, nt = 3, 2
    s = _Scan(gpu_ctx, ns + nt)
    try:
        Ts = _transforms(4)
        m = s.metric("auto")
        delta = _delta(s, m, ns, nt)
        base = m.evaluate()
        want = m.evaluate_weighted_robust_transforms(ns, Ts, 0, delta, want_pairs=True)
        fn = _lib.lib().ecc_metric_evaluate_weighted_robust_transforms
        flat = np.ascontiguousarray(np.asarray(Ts, np.float64).transpose(0, 2, 1)).reshape(-1, 16)

        def call(metric, n_source, K, loss, d, with_Ts=True, outputs=(True, True, True, True)):
            outs = [np.full(4, -7.0), np.full(4, -7.0), np.full(4, -7.0), np.full((4, nt, ns, 4), -7.0, np.float32)]
            rc = fn(metric._h, n_source, K, C.c_void_p(flat.ctypes.data) if with_Ts else None, loss, d,
                    *[C.c_void_p(o.ctypes.data) if on else None for o, on in zip(outs, outputs)])
            return rc, outs

        def refused(code, *args, text=None, **kw):
            rc, outs = call(*args, **kw)
            assert rc == code, (rc, code, args[1:])
            assert text is None or text in _lib.lib().ecc_last_error().decode(), _lib.lib().ecc_last_error()
            assert all(np.all(o == -7.0) for o in outs), outs          # nothing written
        refused(1, m, ns, -1, 0, delta)                                  # n_transforms < 0
        refused(1, m, ns, 4, 0, delta, with_Ts=False)                    # null Ts / values with n_transforms > 0
        refused(1, m, ns, 4, 0, delta, outputs=(False, True, True, True))
        for loss, d in ((3, delta), (-1, delta), (0, 0.0), (1, -2.0), (2, float("nan"))):
            refused(1, m, ns, 4, loss, d)
            refused(1, m, 0, 4, loss, d)                                 # ... which come before n_source
        for bad_ns in (0, -1, ns + nt, ns + nt + 3):
            for K in (4, 0):
                refused(1, m, bad_ns, K, 0, delta, text="n_source")
        rc, outs = call(m, ns, 0, 0, delta, with_Ts=False, outputs=(False, False, False, False))   # no transforms, after the checks: ECC_OK
        assert rc == 0 and m.last_batched_transforms() == 0
        empty = m.evaluate_weighted_robust_transforms(ns, np.zeros((0, 4, 4)), 0, delta, want_pairs=True)
        assert empty[0].shape == empty[1].shape == empty[2].shape == (0,) and empty[3].shape == (0, nt, ns, 4)
        rc, outs = call(m, ns, 4, 0, delta, outputs=(True, False, False, False))                     # only values is required
        assert rc == 0 and np.array_equal(_u64(outs[0]), _u64(want[0])) and np.all(outs[1] == -7.0) and np.all(outs[2] == -7.0)
        m.useCorrelation(True)
        refused(5, m, ns, 4, 0, delta)                                   # ECC_ERR_UNSUPPORTED
        refused(5, m, 0, 4, 0, delta)                                    # ... which comes before n_source
        refused(1, m, ns, 4, 3, delta)                                   # ... and behind the loss
        m.useCorrelation(False)
        assert _same(m.evaluate_weighted_robust_transforms(ns, Ts, 0, delta, want_pairs=True), want)
        assert _u64(m.evaluate())[()] == _u64(base)[()]
        for dtrs in (s.data, s.data + s.weights[:-1], s.data + s.weights + s.weights[:1]):   # n, 2 n - 1, 2 n + 1 intermediates
            refused(1, s.metric("auto", dtrs=dtrs), ns, 4, 0, delta)
        none = E.MetricRadonIntermediate(gpu_ctx, None, s.data + s.weights)                 # no matrices set
        s.metrics.append(none)
        refused(1, none, ns, 4, 0, delta)
    finally:
        s.close()
