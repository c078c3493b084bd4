"""ecc_metric_evaluate_weighted on the GPU (csrc/ecc_weighted.hip, csrc/weighted_kernel.hip): the metric with per-line weights in
Radon space.  The cases are channel_terms.CASES with the data of channel 0 and the weight fields of tests/weighted_terms.py -- the
geometries, grids and settings that select each kernel and loop (labels a .. j); each case asserts from the records
of a single-channel metric that it reached its loop class, as tests/test_gpu_channel_terms.py does.

  ones        all weights 1.0f: value, the c column, the u column and coverage have the bits of evaluate() / 1.0;
  excluded    W_v = 0, the rest 1: the pairs of v are {0, 0}, every other pair has evaluate(cost)'s bits, value is their mean;
  oracle      c and u of every pair against weighted_terms (tests/test_weighted_terms_oracle.py shows that this comparison rejects
              the slips it is there for), value and coverage to 1e-5;
  invariance  the reason the call exists: an opaque block pasted into one view, flagged and turned into line weights, changes no
              bit of the weighted result -- and does change evaluate();
  line_weights, repeatability, errors."""
import numpy as np
import pytest

import channel_terms as T
import weighted_terms as W
from test_gpu_channel_terms import _reached, _records

pytestmark = pytest.mark.gpu


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _close(dtrs):
    for d in dtrs:
        d.close()


def _pair_order(cost):
    n = cost.shape[0]
    iu = np.triu_indices(n, 1)
    return cost[iu[1], iu[0]].copy()


class _Case:
    """The data of a case on the device, and metrics over them with the weight fields asked for."""

    def __init__(self, gpu_ctx, label):
        import epipolarconsistency_amd as E
        self.E, self.ctx, self.label = E, gpu_ctx, label
        self.name, self.n, self.n_alpha, self.n_t, self.radius, self.dkappa, self.derivative, self.setups = W.settings(label)
        self.Ps, self.n_u, self.n_v, self.host, self.weights, self.K01s = W.case_inputs(label)
        self.N = self.n * (self.n - 1) // 2
        gpu_ctx.setQuadCopies(self.setups[0][1])
        kw = {} if self.derivative else dict(filter=E.FILTER_NONE)
        self.data = [E.RadonIntermediate.from_host(gpu_ctx, h, self.n_u, self.n_v, **kw) for h in self.host]
        self.made = []

    def weight_dtrs(self, fields):
        ws = [self.E.RadonIntermediate.from_host(self.ctx, f, self.n_u, self.n_v, filter=self.E.FILTER_NONE) for f in fields]
        self.made += ws
        return ws

    def metric(self, sampling, ws):
        m = self.E.MetricRadonIntermediate(self.ctx, self.Ps, self.data + ws).setSampling(sampling)
        m.setObjectRadius(self.radius)
        m.setEpipolarPlaneStep(self.dkappa)
        return m

    def reached(self, sampling, t):
        rec = _records(self.ctx, self.Ps, self.data, self.radius, self.dkappa)
        _reached(self.label, sampling, rec, t, self.N)
        return rec

    def close(self):
        self.ctx.setQuadCopies("auto")
        _close(self.data + self.made)


@pytest.fixture
def case(gpu_ctx, oracle_mod, request):
    c = _Case(gpu_ctx, request.param)
    try:
        yield c
    finally:
        c.close()


LABELS = sorted(W.CASES)


@pytest.mark.parametrize("case", LABELS, indirect=True)
def test_ones_are_evaluate_bit_for_bit(case):
    """All weights 1.0f (1.0f * d is d): value has the bits of evaluate() on the same metric, pairs[:, 0] those of evaluate(cost),
    pairs[:, 1] == 1.0 and coverage == 1.0 -- in every case and sampling mode of the table."""
    ones = case.weight_dtrs([np.ones((case.n_t, case.n_alpha), np.float32)] * case.n)
    for sampling, _ in case.setups:
        m = case.metric(sampling, ones)
        value, coverage, pairs = m.evaluate_weighted(want_pairs=True)
        plain = m.evaluate()
        cost = np.full((case.n, case.n), -2.0, np.float32)
        with_cost = m.evaluate(cost)
        m.close()
        vals = _pair_order(cost)
        assert pairs.shape == (case.N, 2) and pairs.dtype == np.float32
        assert np.array_equal(_u32(pairs[:, 0]), _u32(vals)), (sampling, np.max(np.abs(pairs[:, 0] - vals)))
        assert _u64(value)[()] == _u64(plain)[()] == _u64(with_cost)[()], (sampling, value, plain)
        assert np.all(pairs[:, 1] == 1.0) and coverage == 1.0, (sampling, coverage)
        assert (vals > 0).sum() >= 0.8 * case.N


@pytest.mark.parametrize("case", LABELS, indirect=True)
def test_an_excluded_view(case):
    """W_v = 0 and the other weights 1: the pairs with v are {0, 0}, every other pair has the bits of evaluate(cost), value equals
    the float64 mean of those entries to 1e-12 relative, coverage is their share of the pairs."""
    v = case.n // 3
    fields = [np.ones((case.n_t, case.n_alpha), np.float32)] * case.n
    fields[v] = np.zeros((case.n_t, case.n_alpha), np.float32)
    ws = case.weight_dtrs(fields)
    iu = np.triu_indices(case.n, 1)
    hit = (iu[0] == v) | (iu[1] == v)
    for sampling, _ in case.setups:
        m = case.metric(sampling, ws)
        value, coverage, pairs = m.evaluate_weighted(want_pairs=True)
        cost = np.full((case.n, case.n), -2.0, np.float32)
        m.evaluate(cost)
        m.close()
        vals = _pair_order(cost)
        assert hit.sum() == case.n - 1 and np.all(pairs[hit] == 0.0), (sampling, pairs[hit])
        assert np.array_equal(_u32(pairs[~hit, 0]), _u32(vals[~hit])) and np.all(pairs[~hit, 1] == 1.0), sampling
        mean = vals[~hit].astype(np.float64).mean()
        assert abs(value - mean) <= 1e-12 * mean, (sampling, value, mean)
        assert abs(coverage - (~hit).sum() / case.N) <= 1e-15, (sampling, coverage)


@pytest.mark.parametrize("case", LABELS, indirect=True)
def test_pair_terms_against_the_direct_oracle(case):
    """c and u of every pair (case e: weighted_terms' sample of the pairs) against the float64 statement: 1e-6 of the scale under the
    reference arithmetic, 1e-3 on the throughput paths, the scale s = w sum d^2 for c and 1 for u; value and coverage to 1e-5
    relative.  The worst ratios of a GPU run are recorded in DESIGN.md 4.15."""
    t = W.case_terms(case.label)
    rows = t["pairs"]
    want, scales = W.columns(t)
    ws = case.weight_dtrs(case.weights)
    failures = []
    for sampling, _ in case.setups:
        rec = case.reached(sampling, t)
        assert np.max(np.abs(rec["kmax"] - case.K01s[:, 15])) <= 1e-3   # the records describe the oracle's ranges, in its pair order
        tol = T.tolerance(sampling, case.N)
        m = case.metric(sampling, ws)
        value, coverage, pairs = m.evaluate_weighted(want_pairs=True)
        m.close()
        assert np.all(np.isfinite(pairs)) and np.isfinite(value)
        ratio = T.compare(pairs[rows], want, scales, tol)
        line = "case %s %s: c %.3g of the bar %.0e, u %.3g" % (case.label, sampling, ratio[0], tol, ratio[1])
        if tol == T.TOL_THROUGHPUT:   # reported: the same against the float64-position statement
            c64, _ = W.columns(W.case_terms(case.label, "float64"))
            r64 = T.compare(pairs[rows], c64, scales, tol)
            line += "; against float64 positions c %.3g, u %.3g" % (r64[0], r64[1])
        if "value" in t:
            ev, ec = abs(value - t["value"]) / (T.TOL_MEAN * t["value"]), abs(coverage - t["coverage"]) / (T.TOL_MEAN * t["coverage"])
            line += "; value %.3g of the bar 1e-05, coverage %.3g" % (ev, ec)
            ratio = np.append(ratio, [ev, ec])
        print(line)
        if not ratio.max() <= 1.0:
            failures.append(line)
    assert not failures, "\n".join(failures)


# ---- invariance: the reason the feature exists -----------------------------------------------------------------------------------
BLOCK = (slice(50, 62), slice(58, 68))   # rows (v), columns (u) of the opaque block in view 3: inside the object's shadow
MARGIN = 3


def _flag(shape):
    """The block dilated by MARGIN pixels.  Why 3: a Radon bin of the data reads the image by bilinear samples (support 1 px either
    side) along its line and, under the derivative filter, along the parallel line 1 px off; so the block changes the bins of lines
    that pass within 1 + sqrt(2) = 2.4 px of one of its pixels.  Such a line crosses the 7 x 7 flagged square around that pixel on a
    chord of at least 3.6 px, i.e. at least 5 samples of step 0.66: L >= 3.3 > zero_at_px = 1, and the weight is exactly 0."""
    f = np.zeros(shape, np.float32)
    f[BLOCK[0].start - MARGIN:BLOCK[0].stop + MARGIN, BLOCK[1].start - MARGIN:BLOCK[1].stop + MARGIN] = 1.0
    return f


@pytest.mark.parametrize("sampling", ["polynomial", "per_sample", "auto"])
def test_a_flagged_block_in_one_view_changes_nothing(gpu_ctx, small_scan, sampling):
    """8 views of the spheres at 128^2 -> 96^2 bins; a second copy with an opaque block in view 3 only.  With the dilated block
    flagged and line_weights(guard_bins=1) for view 3 (ones elsewhere) the weighted result of the corrupted scan == that of the clean
    scan -- value, coverage and every pair term -- while evaluate() of the corrupted scan is larger and coverage < 1."""
    import epipolarconsistency_amd as E
    Ps, imgs, B = small_scan["Ps"], small_scan["imgs"], 96
    n, bad_view = len(Ps), 3
    bad = np.array(imgs, np.float32)
    bad[bad_view][BLOCK] += 4.0 * float(np.max(imgs[bad_view]))
    clean_d = E.RadonIntermediate.compute_batch(gpu_ctx, np.asarray(imgs, np.float32), B, B)
    bad_d = E.RadonIntermediate.compute_batch(gpu_ctx, bad, B, B)
    ones = [E.RadonIntermediate.from_host(gpu_ctx, np.ones((B, B), np.float32), 128, 128, filter=E.FILTER_NONE) for _ in range(n)]
    w3 = E.line_weights(gpu_ctx, _flag(imgs[0].shape), B, B, guard_bins=1)
    ws = ones[:bad_view] + [w3] + ones[bad_view + 1:]
    field = w3.readback()
    assert w3.getFilter() == E.FILTER_NONE and field.min() == 0.0 and field.max() == 1.0
    # the data differ only where the weight is exactly 0, with a ring of one bin (the bilinear taps) to spare
    changed = clean_d[bad_view].readback() != bad_d[bad_view].readback()
    grown = np.pad(changed, 1, mode="edge")
    grown = np.max([grown[dj:dj + B, di:di + B] for dj in range(3) for di in range(3)], axis=0)
    assert changed.any() and np.all(field[grown] == 0.0)
    out = {}
    for key, data in (("clean", clean_d), ("bad", bad_d)):
        m = E.MetricRadonIntermediate(gpu_ctx, Ps, data + ws).setSampling(sampling)
        out[key] = m.evaluate_weighted(want_pairs=True) + (m.evaluate(),)
        m.close()
    (v0, c0, p0, e0), (v1, c1, p1, e1) = out["clean"], out["bad"]
    assert _u64(v0)[()] == _u64(v1)[()] and _u64(c0)[()] == _u64(c1)[()] and np.array_equal(_u32(p0), _u32(p1)), (v0, v1)
    assert e1 > e0, (e0, e1)     # the unweighted metric sees the block
    assert c0 < 1.0 and v0 > 0.0 and np.all(p0[:, 1] <= 1.0)
    iu = np.triu_indices(n, 1)
    hit = (iu[0] == bad_view) | (iu[1] == bad_view)
    assert np.all(p0[~hit, 1] == 1.0) and p0[hit, 1].min() < 1.0
    print("%s: weighted %.9g (coverage %.4f) on both scans; evaluate() clean %.6g, corrupted %.6g" % (sampling, v0, c0, e0, e1))
    _close(clean_d + bad_d + ones + [w3])


def test_line_weights_are_the_oracles_transform(gpu_ctx, oracle_mod):
    """In the exact Radon arithmetic: line_weights == the oracle's FILTER_NONE transform of the flagged image put through the same
    clip and minimum, bit for bit -- one image, a stack, and non-default zero_at_px / guard_bins on a non-square grid."""
    import epipolarconsistency_amd as E
    assert gpu_ctx.getRadonArithmetic() == "exact"
    flagged = _flag((128, 128))
    other = np.zeros((128, 128), np.float32)
    other[:, 90:92] = 1.0   # a defective column pair
    for n_alpha, n_t, zero_at, guard in ((96, 96, 1.0, 1), (80, 56, 2.5, 2), (48, 40, 1.0, 0)):
        want = [E.line_weights_from_lengths(oracle_mod.radon(f, n_alpha, n_t, filter=E.FILTER_NONE), zero_at, guard) for f in (flagged, other)]
        one = E.line_weights(gpu_ctx, flagged, n_alpha, n_t, zero_at, guard)
        both = E.line_weights(gpu_ctx, [flagged, other], n_alpha, n_t, zero_at_px=zero_at, guard_bins=guard)
        assert isinstance(both, list) and len(both) == 2 and one.getFilter() == E.FILTER_NONE
        assert (one.getRadonBinNumber(0), one.getRadonBinNumber(1), one.getOriginalImageSize(0)) == (n_alpha, n_t, 128)
        assert np.array_equal(_u32(one.readback()), _u32(want[0]))
        for d, w in zip(both, want):
            assert np.array_equal(_u32(d.readback()), _u32(w)) and 0.0 < (w == 0).mean() < 1.0
        _close([one] + both)


# ---- repeatability, nothing else moved, errors -----------------------------------------------------------------------------------
def test_repeatable_and_nothing_else_moved(gpu_ctx, oracle_mod):
    """Two calls give identical bits; evaluate() (with one view moved and back), a pose batch and an evaluate_view_coefficients call
    around the call are unchanged."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import geometry as Gm
    c = _Case(gpu_ctx, "i")
    try:
        n = c.n
        m = c.metric("polynomial", c.weight_dtrs(c.weights))
        P0 = E.pack_projection_matrices(c.Ps)
        P1 = P0.copy()
        P1[n // 2] = E.pack_projection_matrices([Gm.compose_transform(P0[n // 2].reshape(4, 3).T, Gm.rigid_transform(tx=3.0, ry=0.01))])[0]
        a = np.random.default_rng(11).uniform(0.5, 1.5, (2, n))

        def observe():
            base = m.setProjectionMatrices(P0).evaluate()
            moved = m.setProjectionMatrices(P1).evaluate()
            back = m.setProjectionMatrices(P0).evaluate()
            deltas = m.evaluate_pose_deltas([n // 2, 1], np.stack([P1[n // 2], P0[2]]))
            value, grad = m.evaluate_view_coefficients(a)
            cost = np.zeros((n, n), np.float32)
            with_cost = m.evaluate(cost)
            return np.concatenate([[base, moved, back, value, with_cost], np.ravel(deltas), grad.reshape(-1)]), cost
        before, cost_b = observe()
        first = m.evaluate_weighted(want_pairs=True)
        second = m.evaluate_weighted(want_pairs=True)
        after, cost_a = observe()
        assert np.array_equal(_u64(before), _u64(after)) and np.array_equal(_u32(cost_b), _u32(cost_a))
        assert _u64(first[0])[()] == _u64(second[0])[()] and _u64(first[1])[()] == _u64(second[1])[()]
        assert np.array_equal(_u32(first[2]), _u32(second[2]))
        assert m.evaluate_weighted() == first[:2]   # without the pair terms: the same two numbers
        # in the middle of a sequence: matrices moved, then the call, then back
        m.setProjectionMatrices(P1).evaluate()
        moved = m.evaluate_weighted()
        assert _u64(m.evaluate())[()] == _u64(before[1])[()]          # the moved matrices are still current
        assert _u64(m.setProjectionMatrices(P0).evaluate())[()] == _u64(before[0])[()]
        again = m.evaluate_weighted(want_pairs=True)
        assert _u64(again[0])[()] == _u64(first[0])[()] and np.array_equal(_u32(again[2]), _u32(first[2])) and moved[0] != first[0]
        m.close()
    finally:
        c.close()


def test_all_weights_zero(gpu_ctx, oracle_mod):
    """sum u == 0: value = 0.0, coverage = 0.0, no error."""
    c = _Case(gpu_ctx, "d")
    try:
        m = c.metric("auto", c.weight_dtrs([np.zeros((c.n_t, c.n_alpha), np.float32)] * c.n))
        value, coverage, pairs = m.evaluate_weighted(want_pairs=True)
        m.close()
        assert value == 0.0 and coverage == 0.0 and np.all(pairs == 0.0)
    finally:
        c.close()


def test_errors(gpu_ctx, oracle_mod):
    import epipolarconsistency_amd as E
    c = _Case(gpu_ctx, "d")
    try:
        ws = c.weight_dtrs(c.weights)
        m = c.metric("auto", ws)
        want = m.evaluate_weighted(want_pairs=True)
        m.useCorrelation(True)
        with pytest.raises(E.EccError) as e:
            m.evaluate_weighted()
        assert e.value.code == 5, e.value   # ECC_ERR_UNSUPPORTED
        m.useCorrelation(False)
        again = m.evaluate_weighted(want_pairs=True)
        assert _u64(again[0])[()] == _u64(want[0])[()] and np.array_equal(_u32(again[2]), _u32(want[2]))
        m.close()
        for dtrs in (c.data, c.data + ws[:-1], c.data + ws + ws[:1]):   # n, 2 n - 1, 2 n + 1 intermediates
            bad = E.MetricRadonIntermediate(gpu_ctx, c.Ps, dtrs)
            with pytest.raises(E.EccError) as e:
                bad.evaluate_weighted()
            assert e.value.code == 1, (len(dtrs), e.value)
            bad.close()
        one = E.MetricRadonIntermediate(gpu_ctx, c.Ps[:1], [c.data[0], ws[0]])   # fewer than two views
        with pytest.raises(E.EccError) as e:
            one.evaluate_weighted()
        assert e.value.code == 1
        one.close()
        none = E.MetricRadonIntermediate(gpu_ctx, None, c.data + ws)   # no matrices set
        with pytest.raises(E.EccError) as e:
            none.evaluate_weighted()
        assert e.value.code == 1
        none.close()
    finally:
        c.close()
