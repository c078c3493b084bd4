"""ecc_metric_evaluate_weighted_transforms on the GPU (csrc/ecc_weighted_transforms.hip, csrc/weighted_transforms_kernel.hip): the
metric with per-line weights for the registration of two scans -- K rigid source-to-target transforms as ONE compose / E1 / list
launch, ONE record launch, ONE weighted pair launch and ONE segmented sum of both columns.

The scans, cross lists and transforms are tests/test_gpu_transforms.py's (_scan: seven random intermediates dealt to the views), the
weights tests/weighted_terms.weight_fields (blocks of exactly 0, exactly 1, U(0, 1)), seven fields dealt the same way.  The contract
is BITS: values, coverages and pair terms equal setProjectionMatrices(composed matrices) + evaluate_weighted_pairs(the cross list) per
transform on a second metric -- whatever the list length (the reference arithmetic's bound, whole float4s and tails, the
sixteen-slice sum), the sampling mode, the object radius (under the automatic one every transform has its OWN), batches that split and
whatever the metric did before; the call leaves the metric as it found it.  The terms are also held against the float64 statement of
tests/weighted_terms.py directly, and one registration shows what the call is for."""
import numpy as np
import pytest

import channel_terms as T
import weighted_terms as W
from test_gpu_transforms import _composed, _configure, _cross_list, _scan, _transforms
from test_gpu_weighted import BLOCK, _flag

pytestmark = pytest.mark.gpu


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


class _Scan:
    """n views: the data of test_gpu_transforms._scan, weight intermediates from seven fields dealt like the data (None: weight_fields)."""

    def __init__(self, gpu_ctx, n, B=48, fields=None):
        import epipolarconsistency_amd as E
        self.E, self.ctx, self.n, self.B = E, gpu_ctx, n, B
        self.Ps, self.base, self.data = _scan(gpu_ctx, n, B=B)
        self.fields = W.weight_fields(7, B, B) if fields is None else list(fields)
        self.wbase = [E.RadonIntermediate.from_host(gpu_ctx, f, 128, 128, filter=E.FILTER_NONE) for f in self.fields]
        self.weights = [self.wbase[v % 7] for v in range(n)]
        self.metrics = []

    def metric(self, mode, radius=0.0, dkappa=0.0, dtrs=None):
        m = self.E.MetricRadonIntermediate(self.ctx, self.Ps, self.data + self.weights if dtrs is None else dtrs)
        self.metrics.append(m)
        return _configure(m, mode, radius, dkappa)

    def close(self):
        for m in self.metrics:
            m.close()
        for d in self.base + self.wbase:
            d.close()


def _sequential(b, Ps, ns, nt, Ts):
    """What a caller without the entry point does: per transform setProjectionMatrices + evaluate_weighted_pairs of the cross list."""
    idx = _cross_list(ns, nt)
    values, coverages, pairs = np.zeros(len(Ts)), np.zeros(len(Ts)), np.zeros((len(Ts), nt, ns, 2), np.float32)
    for k, Tk in enumerate(Ts):
        values[k], coverages[k], rows = b.setProjectionMatrices(_composed(Ps, ns, Tk)).evaluate_weighted_pairs(idx, want_pairs=True)
        pairs[k] = rows.reshape(nt, ns, 2)
    b.setProjectionMatrices(Ps)
    return values, coverages, pairs


def _same(got, want):
    return all(np.array_equal(_u64(g), _u64(w)) for g, w in zip(got[:2], want[:2])) and \
        (len(got) < 3 or np.array_equal(_u32(got[2]), _u32(want[2])))


# ---- 1. sequential bits ----------------------------------------------------------------------------------------------------------
CASES = [
    # (n_source, n_target, mode, radius, dkappa)
    (1, 1, "auto", 0.0, 0.0), (1, 1, "polynomial", 0.0, 0.0), (1, 7, "polynomial", 90.0, 0.006), (3, 2, "reference", 0.0, 0.0),
    (20, 20, "auto", 0.0, 0.0), (20, 20, "polynomial", 0.0, 0.0), (20, 20, "per_sample", 75.0, 0.0),
    (23, 22, "auto", 0.0, 0.0),      # 506 tuples: below ECC_SAMPLING_AUTO_REFERENCE_PAIRS
    (23, 23, "auto", 0.0, 0.0),      # 529: above it
    (64, 65, "per_sample", 0.0, 0.0),   # 4 160 values: whole float4s
    (67, 33, "polynomial", 0.0, 0.0),   # 2 211: a tail of 3
    (181, 182, "auto", 0.0, 0.0),       # 32 942 values: the sixteen-slice sum
]


@pytest.mark.parametrize("ns,nt,mode,radius,dkappa", CASES)
def test_transforms_have_the_sequential_bits(gpu_ctx, ns, nt, mode, radius, dkappa):
    n = ns + nt
    s = _Scan(gpu_ctx, n, B=32 if n > 100 else 48)
    try:
        K = 9 if n < 200 else 5
        Ts = _transforms(K)
        assert len(Ts) == K
        a, b = s.metric(mode, radius, dkappa), s.metric(mode, radius, dkappa)
        if radius == 0.0:
            # the automatic radius follows the COMPOSED view 0: the case tests the per-transform radius only if they differ
            radii = {np.float32(s.E.host_object_radius(_composed(s.Ps, ns, Tk)[0], 128, 128)) for Tk in Ts}
            assert len(radii) >= 2, radii
        want = _sequential(b, s.Ps, ns, nt, Ts)
        got = a.evaluate_weighted_transforms(ns, Ts, want_pairs=True)
        assert a.last_batched_transforms() == K
        assert got[2].shape == (K, nt, ns, 2) and got[2].dtype == np.float32 and got[0].dtype == got[1].dtype == np.float64
        assert np.array_equal(_u32(got[2]), _u32(want[2])), (np.argwhere(got[2] != want[2])[:5], np.abs(got[2] - want[2]).max())
        assert np.array_equal(_u64(got[0]), _u64(want[0])), (np.flatnonzero(got[0] != want[0]), (got[0] - want[0])[got[0] != want[0]])
        assert np.array_equal(_u64(got[1]), _u64(want[1])), (np.flatnonzero(got[1] != want[1]), (got[1] - want[1])[got[1] != want[1]])
        # the weights are seen: some lines count, some do not
        assert np.all(want[1] > 0) and np.all(want[1] < 1) and np.all(want[0] > 0)
        assert got[0][-1] == got[0][-2] and got[1][-1] == got[1][-2] and np.array_equal(got[2][-1], got[2][-2])   # two equal transforms
        # the values alone (no pair terms), and again in reverse order from whatever state the call left
        assert _same(a.evaluate_weighted_transforms(ns, Ts), want[:2])
        back = a.evaluate_weighted_transforms(ns, Ts[::-1], want_pairs=True)
        assert _same(back, (want[0][::-1], want[1][::-1], want[2][::-1])) and a.last_batched_transforms() == K
        # neither coverages nor pair terms: the C call with both null
        import ctypes as C
        from epipolarconsistency_amd import _lib
        flat = np.ascontiguousarray(np.asarray(Ts, np.float64).transpose(0, 2, 1)).reshape(-1, 16)
        alone = np.zeros(K)
        assert _lib.lib().ecc_metric_evaluate_weighted_transforms(a._h, ns, K, C.c_void_p(flat.ctypes.data), C.c_void_p(alone.ctypes.data),
                                                                  None, None) == 0
        assert np.array_equal(_u64(alone), _u64(want[0]))
    finally:
        s.close()


# ---- 2. batches that split -------------------------------------------------------------------------------------------------------
def test_batches_that_split(gpu_ctx):
    """181 x 182 = 32 942 entries per transform: ECC_POSE_BATCH_MAX_ENTRIES = 2^20 holds 31 of them, so 40 transforms go as two
    batches (31 + 9); same bits, all of them through the batch."""
    ns, nt, K = 181, 182, 40
    s = _Scan(gpu_ctx, ns + nt, B=32)
    try:
        Ts = _transforms(K)
        a, b = s.metric("auto"), s.metric("auto")
        want = _sequential(b, s.Ps, ns, nt, Ts)
        got = a.evaluate_weighted_transforms(ns, Ts, want_pairs=True)
        assert a.last_batched_transforms() == K
        assert _same(got, want), (np.flatnonzero(got[0] != want[0]), np.flatnonzero(got[1] != want[1]))
    finally:
        s.close()


# ---- 3. weights all 1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,nt,mode", [(3, 2, "auto"), (20, 20, "polynomial"), (67, 33, "per_sample")])
def test_ones_are_the_unweighted_transforms(gpu_ctx, ns, nt, mode):
    """Every weight 1.0f: values and the c column have the bits of evaluate_transforms' means and pair values on a metric of the data
    alone, every u and every coverage is 1.0."""
    s = _Scan(gpu_ctx, ns + nt, fields=[np.ones((48, 48), np.float32)] * 7)
    try:
        Ts = _transforms(9)
        a, plain = s.metric(mode), s.metric(mode, dtrs=s.data)
        means, vals = plain.evaluate_transforms(ns, Ts, want_pairs=True)
        values, coverages, pairs = a.evaluate_weighted_transforms(ns, Ts, want_pairs=True)
        assert a.last_batched_transforms() == plain.last_batched_transforms() == 9
        assert np.array_equal(_u64(values), _u64(means)), (values, means)
        assert np.array_equal(_u32(pairs[..., 0]), _u32(vals))
        assert np.all(pairs[..., 1] == 1.0) and np.all(coverages == 1.0)
        assert (vals > 0).mean() > 0.8
    finally:
        s.close()


# ---- 4. the metric is left as found ----------------------------------------------------------------------------------------------
def test_the_metric_is_left_as_found(gpu_ctx):
    """evaluate() (record reuse on: the kept records are neither used for the batch nor overwritten by it), evaluate_weighted() with
    its rows and an evaluate_pose_deltas made before the call give the same bits after it; the current matrices are unchanged; one
    view moved afterwards refits from the kept records as if the batch had not happened."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import geometry
    ns, nt = 60, 52
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
        want = _sequential(seq, s.Ps, ns, nt, Ts)

        def observe(m):
            w = m.evaluate_weighted(want_pairs=True)
            return np.concatenate([[m.evaluate(), w[0], w[1]], m.evaluate_pose_deltas(views, rows)]), w[2]
        before, rows_before = observe(a)
        assert _u64(before[0])[()] == _u64(ref.evaluate())[()]
        assert _same(a.evaluate_weighted_transforms(ns, Ts, want_pairs=True), want) and a.last_batched_transforms() == len(Ts)
        assert [np.array_equal(x, y) for x, y in zip(a.getProjectionMatrices(), s.Ps)] == [True] * n
        after, rows_after = observe(a)
        assert np.array_equal(_u64(before), _u64(after)) and np.array_equal(_u32(rows_before), _u32(rows_after))
        # straight after a batch, without anything in between
        assert _same(a.evaluate_weighted_transforms(ns, Ts[:3]), (want[0][:3], want[1][:3]))
        assert _u64(a.evaluate())[()] == _u64(before[0])[()]
        # one view moves: the reuse path refits its pairs from the kept records
        assert _u64(a.setProjectionMatrices(P1).evaluate())[()] == _u64(ref.setProjectionMatrices(P1).evaluate())[()]
        moved_Ps = [p.reshape(4, 3).T for p in P1]
        got = a.evaluate_weighted_transforms(ns, Ts[:3], want_pairs=True)
        seq.setProjectionMatrices(P1)
        idx = _cross_list(ns, nt)
        for k in range(3):
            v, c, r = seq.setProjectionMatrices(_composed(moved_Ps, ns, Ts[k])).evaluate_weighted_pairs(idx, want_pairs=True)
            assert _u64(v)[()] == _u64(got[0][k])[()] and _u64(c)[()] == _u64(got[1][k])[()]
            assert np.array_equal(_u32(r.reshape(nt, ns, 2)), _u32(got[2][k]))
        assert _u64(a.setProjectionMatrices(P0).evaluate())[()] == _u64(before[0])[()]
    finally:
        s.close()


# ---- 5. fallbacks ----------------------------------------------------------------------------------------------------------------
def test_batching_off_goes_the_sequential_way(gpu_ctx):
    """setPoseBatching(False): the sequential way inside the call, same bits, nothing batched, the base matrices current again.  (A
    list longer than a batch needs more than 2^20 tuples per transform: no hook makes a batch smaller, so that branch -- the same
    function -- is not run here.)"""
    ns, nt = 9, 6
    s = _Scan(gpu_ctx, ns + nt)
    try:
        Ts = _transforms(6)
        a, b = s.metric("auto"), s.metric("auto")
        want = _sequential(b, s.Ps, ns, nt, Ts)
        before = (a.evaluate(), a.evaluate_weighted())
        assert _same(a.evaluate_weighted_transforms(ns, Ts, want_pairs=True), want) and a.last_batched_transforms() == 6
        a.setPoseBatching(False)
        assert _same(a.evaluate_weighted_transforms(ns, Ts, want_pairs=True), want) and a.last_batched_transforms() == 0
        assert _same(a.evaluate_weighted_transforms(ns, Ts), want[:2]) and a.last_batched_transforms() == 0
        assert [np.array_equal(x, y) for x, y in zip(a.getProjectionMatrices(), s.Ps)] == [True] * (ns + nt)
        assert (a.evaluate(), a.evaluate_weighted()) == before
        a.setPoseBatching(True)
        one = a.evaluate_weighted_transforms(ns, Ts[1])   # a single (4, 4) matrix
        assert one[0].shape == (1,) and _u64(one[0][0])[()] == _u64(want[0][1])[()] and a.last_batched_transforms() == 1
    finally:
        s.close()


# ---- 6. directly against the float64 statement -----------------------------------------------------------------------------------
def test_against_the_oracle_directly(gpu_ctx, oracle_mod, small_scan):
    """4 source + 4 target views of the small scan with ORACLE dtrs and weight_fields, the five transforms of
    tests/test_gpu_transforms.py::test_against_the_oracle_directly: c and u of every cross pair of every transform against
    weighted_terms.pair_terms with the C oracle's pair geometry of the COMPOSED matrices (automatic radius: every transform its own)
    -- not through the sequential calls.  The bars are the project's: 1e-6 of the scale under the reference
    arithmetic ("auto": 16 tuples), 1e-3 in POLYNOMIAL.  The same comparison rejects the weights of source view i taken from source
    view (i + 1) % n_source -- what a weight that followed the extended matrix index, or a wrong n_views, would sample."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import geometry
    s = small_scan
    ns = nt = 4
    n_u, n_v, B = s["n_u"], s["n_v"], s["n_alpha"]
    fields = W.weight_fields(8, s["n_t"], s["n_alpha"])
    Ts = [np.eye(4), geometry.rigid_transform(tx=4.0, ty=-2.0), geometry.rigid_transform(rz=0.02, rx=-0.01),
          geometry.rigid_transform(tx=-6.0, tz=5.0, ry=0.015), geometry.rigid_transform(tx=1.0, ty=1.0, tz=1.0, rx=0.01, ry=0.01, rz=0.01)]
    idx = _cross_list(ns, nt)
    want, scales, slip = (np.zeros((len(Ts), nt, ns, 2)) for _ in range(3))
    for k, Tk in enumerate(Ts):
        K01s = oracle_mod.evaluate_pairs(_composed(s["Ps"], ns, Tk), s["dtrs"], n_u, n_v, idx, want_K01=True)["K01s"]
        for q, (i, j, _, _) in enumerate(idx):
            t = W.pair_terms(K01s[q], s["dtrs"][i], s["dtrs"][j], fields[i], fields[j], n_u, n_v)
            w = W.pair_terms(K01s[q], s["dtrs"][i], s["dtrs"][j], fields[(i + 1) % ns], fields[j], n_u, n_v)
            want[k, q // ns, q % ns] = (t["c"], t["u"])
            scales[k, q // ns, q % ns] = (t["s"], 1.0)
            slip[k, q // ns, q % ns] = (w["c"], w["u"])
    dtrs = [E.RadonIntermediate.from_host(gpu_ctx, d, n_u, n_v) for d in s["dtrs"]]
    ws = [E.RadonIntermediate.from_host(gpu_ctx, f, n_u, n_v, filter=E.FILTER_NONE) for f in fields]
    m = E.MetricRadonIntermediate(gpu_ctx, s["Ps"], dtrs + ws)
    try:
        failures = []
        for mode in ("auto", "polynomial"):
            m.setSampling(mode)
            tol = T.tolerance(mode, ns * nt)
            assert tol == (T.TOL_REFERENCE if mode == "auto" else T.TOL_THROUGHPUT)
            values, coverages, pairs = m.evaluate_weighted_transforms(ns, Ts, want_pairs=True)
            assert m.last_batched_transforms() == len(Ts) and np.all(np.isfinite(pairs))
            ratio = T.compare(pairs.reshape(-1, 2), want.reshape(-1, 2), scales.reshape(-1, 2), tol)
            rejected = T.compare(slip.reshape(-1, 2), want.reshape(-1, 2), scales.reshape(-1, 2), tol)
            ev = np.max(np.abs(values - want[..., 0].sum(axis=(1, 2)) / want[..., 1].sum(axis=(1, 2))) / values) / T.TOL_MEAN
            line = "%s: c %.3g of the bar %.0e, u %.3g (values, reported: %.3g of 1e-05); the slip: c %.3g, u %.3g of the bar" % (
                mode, ratio[0], tol, ratio[1], ev, rejected[0], rejected[1])
            print(line)
            if not (ratio.max() <= 1.0 and rejected.min() > 1.0):
                failures.append(line)
        assert not failures, "\n".join(failures)
    finally:
        m.close()
        for d in dtrs + ws:
            d.close()


# ---- 7. what the call is for -----------------------------------------------------------------------------------------------------
def test_an_instrument_in_one_source_view_changes_no_bit_of_a_sweep(gpu_ctx, oracle_mod):
    """The registration of tests/test_gpu_transforms.py::test_a_registration_finds_the_true_transform -- make_small_scan, source views
    0, 2, 4, 6 under inv(T_true), 21 transforms tx = 6 + d, d = -10 .. 10 mm, radius fixed at 60 mm -- with the dtrs computed on the
    GPU and the opaque block of tests/test_gpu_weighted.py pasted into source view 2.  Its dilation flagged and turned into
    line_weights(guard_bins=1) for that view (ones elsewhere), values, coverages and pair terms of the corrupted and of the clean scan
    are the same bits for all 21 transforms, while evaluate_transforms sees the block.  The float64 statement (weighted_terms.scan_terms
    over the composed matrices, cross pairs only) has its minimum at the interior point d = 0, 5319.72, the runner-up d = -1 at
    5334.43, i.e. 2.77e-3 above: 277 times the 1e-5 value bar (computed with oracle dtrs; the test asserts at least ten times the bar
    on its own data before it compares the argmin)."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import geometry
    from conftest import make_small_scan
    Ps, imgs = make_small_scan()
    n_u = n_v = 128
    B, n, ns, nt, bad_view = 96, 8, 4, 4, 2
    T_true = geometry.rigid_transform(tx=6, ty=-3, rz=0.02)
    src, tgt = [0, 2, 4, 6], [1, 3, 5, 7]
    Ps_reg = [Ps[i] @ np.linalg.inv(T_true) for i in src] + [Ps[j] for j in tgt]
    clean = np.array([imgs[v] for v in src + tgt], np.float32)
    bad = clean.copy()
    bad[bad_view][BLOCK] += 4.0 * float(np.max(clean[bad_view]))
    ds = np.arange(-10, 11)
    Ts = [geometry.rigid_transform(tx=6 + float(d), ty=-3, rz=0.02) for d in ds]
    clean_d = E.RadonIntermediate.compute_batch(gpu_ctx, clean, B, B)
    bad_d = E.RadonIntermediate.compute_batch(gpu_ctx, bad, B, B)
    ones = [E.RadonIntermediate.from_host(gpu_ctx, np.ones((B, B), np.float32), n_u, n_v, filter=E.FILTER_NONE) for _ in range(n)]
    w2 = E.line_weights(gpu_ctx, _flag(clean[0].shape), B, B, guard_bins=1)
    ws = ones[:bad_view] + [w2] + ones[bad_view + 1:]
    try:
        field = w2.readback()
        assert field.min() == 0.0 and field.max() == 1.0
        # the data differ only where the weight is exactly 0, with a ring of one bin (the bilinear taps) to spare
        host = [d.readback() for d in bad_d]
        changed = clean_d[bad_view].readback() != host[bad_view]
        grown = np.pad(changed, 1, mode="edge")
        grown = np.max([grown[dj:dj + B, di:di + B] for dj in range(3) for di in range(3)], axis=0)
        assert changed.any() and np.all(field[grown] == 0.0)
        out = {}
        for key, data in (("clean", clean_d), ("bad", bad_d)):
            m = E.MetricRadonIntermediate(gpu_ctx, Ps_reg, data + ws).setSampling("polynomial")
            m.setObjectRadius(60.0)
            out[key] = m.evaluate_weighted_transforms(ns, Ts, want_pairs=True)
            assert m.last_batched_transforms() == len(Ts)
            m.close()
            m = E.MetricRadonIntermediate(gpu_ctx, Ps_reg, data).setSampling("polynomial")
            m.setObjectRadius(60.0)
            out[key + " unweighted"] = m.evaluate_transforms(ns, Ts)
            m.close()
        assert _same(out["bad"], out["clean"]), (out["bad"][0], out["clean"][0])
        assert np.all(out["bad unweighted"] != out["clean unweighted"])    # the unweighted sweep sees the block
        values, coverages, pairs = out["bad"]
        assert np.all(coverages < 1.0) and np.all(coverages > 0.5) and np.all(values > 0)
        assert np.all(pairs[:, :, [0, 1, 3], 1] == 1.0) and pairs[:, :, bad_view, 1].min() < 1.0   # only the pairs of the flagged view
        # the float64 statement over the composed matrices, cross pairs only, on the corrupted data
        cross = [q for q in range(n * (n - 1) // 2) if oracle_mod.get_ij(q, n)[0] < ns <= oracle_mod.get_ij(q, n)[1]]
        fields = [np.ones((B, B), np.float32)] * bad_view + [field] + [np.ones((B, B), np.float32)] * (n - bad_view - 1)
        want = np.zeros(len(Ts))
        for k, Tk in enumerate(Ts):
            comp = _composed(Ps_reg, ns, Tk)
            K01s = oracle_mod.evaluate_all(comp, host, n_u, n_v, object_radius_mm=60.0, want_K01=True)["K01s"]
            t = W.scan_terms(comp, host, fields, n_u, n_v, K01s, pairs=cross)
            want[k] = t["c"].sum() / t["u"].sum()
        order = np.argsort(want)
        margin = (want[order[1]] - want[order[0]]) / want[order[0]]
        print("oracle", want, "batch", values, "rel", np.abs(values - want) / want, "runner-up above the minimum by", margin)
        assert 0 < int(order[0]) < len(ds) - 1 and margin >= 10 * T.TOL_MEAN, (order[:2], margin)
        assert int(np.argmin(values)) == int(order[0]) == int(np.argmin(out["clean"][0]))
    finally:
        for d in clean_d + bad_d + ones + [w2]:
            d.close()


# ---- 8. errors on a live metric --------------------------------------------------------------------------------------------------
def test_errors_on_a_live_metric(gpu_ctx):
    import epipolarconsistency_amd as E
    ns, nt = 3, 2
    s = _Scan(gpu_ctx, ns + nt)
    try:
        Ts = _transforms(4)
        m = s.metric("auto")
        want = m.evaluate_weighted_transforms(ns, Ts, want_pairs=True)
        # no transforms: nothing happens, after the other checks
        empty = m.evaluate_weighted_transforms(ns, np.zeros((0, 4, 4)), want_pairs=True)
        assert empty[0].shape == empty[1].shape == (0,) and empty[2].shape == (0, nt, ns, 2) and m.last_batched_transforms() == 0
        for bad_ns in (0, -1, ns + nt, ns + nt + 3):
            for Tk in (Ts, np.zeros((0, 4, 4))):
                with pytest.raises(E.EccError) as e:
                    m.evaluate_weighted_transforms(bad_ns, Tk)
                assert e.value.code == 1 and "n_source" in str(e.value)
        m.useCorrelation(True)
        with pytest.raises(E.EccError) as e:
            m.evaluate_weighted_transforms(ns, Ts)
        assert e.value.code == 5, e.value   # ECC_ERR_UNSUPPORTED
        with pytest.raises(E.EccError) as e:   # ... which comes before n_source
            m.evaluate_weighted_transforms(0, Ts)
        assert e.value.code == 5, e.value
        m.useCorrelation(False)
        assert _same(m.evaluate_weighted_transforms(ns, Ts, want_pairs=True), want)
        for dtrs in (s.data, s.data + s.weights[:-1], s.data + s.weights + s.weights[:1]):   # n, 2 n - 1, 2 n + 1 intermediates
            bad = s.metric("auto", dtrs=dtrs)
            with pytest.raises(E.EccError) as e:
                bad.evaluate_weighted_transforms(ns, Ts)
            assert e.value.code == 1 and "2 * n_views" in str(e.value), (len(dtrs), e.value)
        none = E.MetricRadonIntermediate(gpu_ctx, None, s.data + s.weights)   # no matrices set
        s.metrics.append(none)
        with pytest.raises(E.EccError) as e:
            none.evaluate_weighted_transforms(ns, Ts)
        assert e.value.code == 1
    finally:
        s.close()
