"""ecc_metric_evaluate_robust[_pairs] on the GPU (csrc/ecc_robust.hip, csrc/robust_kernel.hip): the metric under a per-sample robust
loss.  The cases are weighted_terms.CASES with the data of channel 0 -- the geometries, grids and settings that select each kernel
and loop (labels a .. j); each case asserts from the records of a single-channel metric that it reached its
loop class, as tests/test_gpu_weighted.py does.

  infinite scale  delta = +inf and FLT_MAX, every loss: value, the c column, the u column and inlier_mass have the bits of evaluate()
                  / 1.0; the list form has the bits of evaluate(indices) and of the all-pairs rows;
  oracle          {c, u, r} of every pair against robust_terms at both scales of the case and for all three losses
                  (tests/test_robust_terms_oracle.py shows that this comparison rejects the slips it is there for), value and
                  inlier_mass to 1e-5;
  block           the reason the call exists: an opaque block pasted into one view that nobody flagged;
  repeatability, nothing else moved, edge cases, errors."""
import ctypes as C

import numpy as np
import pytest

import channel_terms as T
import robust_terms as R
import weighted_terms as W
from test_gpu_channel_terms import _reached, _records
from test_gpu_weighted import BLOCK

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
LOSS_CODES = {"huber": 0, "truncated": 1, "geman_mcclure": 2}


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


def _all_pairs_list(n):
    iu = np.triu_indices(n, 1)   # get_ij order: i < j, i slow
    return np.ascontiguousarray(np.stack([iu[0], iu[1], iu[0], iu[1]], axis=1), np.int32)


class _Case:
    """The data of a case on the device, and metrics over them."""

    def __init__(self, gpu_ctx, label):
        import epipolarconsistency_amd as E
        self.E, self.ctx, self.label = E, gpu_ctx, label
        self.name, self.n, self.n_alpha, self.n_t, self.radius, self.dkappa, self.derivative, self.setups = W.settings(label)
        self.Ps, self.n_u, self.n_v, self.host, self.weights, self.K01s = W.case_inputs(label)
        self.N = self.n * (self.n - 1) // 2
        gpu_ctx.setQuadCopies(self.setups[0][1])
        kw = {} if self.derivative else dict(filter=E.FILTER_NONE)
        self.data = [E.RadonIntermediate.from_host(gpu_ctx, h, self.n_u, self.n_v, **kw) for h in self.host]

    def metric(self, sampling, extra=()):
        m = self.E.MetricRadonIntermediate(self.ctx, self.Ps, self.data + list(extra)).setSampling(sampling)
        m.setObjectRadius(self.radius)
        m.setEpipolarPlaneStep(self.dkappa)
        return m

    def reached(self, sampling):
        rec = _records(self.ctx, self.Ps, self.data, self.radius, self.dkappa)
        _reached(self.label, sampling, rec, W.case_terms(self.label), self.N)
        return rec

    def close(self):
        self.ctx.setQuadCopies("auto")
        _close(self.data)


@pytest.fixture
def case(gpu_ctx, oracle_mod, request):
    c = _Case(gpu_ctx, request.param)
    try:
        yield c
    finally:
        c.close()


LABELS = sorted(R.CASES)


@pytest.mark.parametrize("case", LABELS, indirect=True)
def test_an_infinite_scale_is_evaluate_bit_for_bit(case):
    """delta = +inf and delta = FLT_MAX (no |d| exceeds either: every w is 1.0f, and 1.0f * d is d), for every loss, in every case and
    sampling setup of the table: pairs[:, 0] has the bits of evaluate(cost), value those of evaluate(), pairs[:, 1] == 1.0 and
    inlier_mass == 1.0; the list form with the tuples (i, j, i, j) of all pairs has the bits of evaluate(indices) of that list and of
    the all-pairs rows (the same length, so the same resolved mode)."""
    idx = _all_pairs_list(case.n)
    for sampling, _ in case.setups:
        case.reached(sampling)
        m = case.metric(sampling)
        plain = m.evaluate()
        cost = np.full((case.n, case.n), -2.0, np.float32)
        with_cost = m.evaluate(cost)
        vals = _pair_order(cost)
        listed = np.full(case.N, -2.0, np.float32)
        list_mean = m.evaluate(idx, listed)
        assert (vals > 0).sum() >= 0.8 * case.N and _u64(plain)[()] == _u64(with_cost)[()]
        rows_r = None
        for loss in R.LOSSES:
            for delta in (float("inf"), FLT_MAX):
                value, mass, pairs = m.evaluate_robust(LOSS_CODES[loss], delta, want_pairs=True)
                where = (sampling, loss, delta)
                assert pairs.shape == (case.N, 3) and pairs.dtype == np.float32
                assert np.array_equal(_u32(pairs[:, 0]), _u32(vals)), (where, np.max(np.abs(pairs[:, 0] - vals)))
                assert _u64(value)[()] == _u64(plain)[()], (where, value, plain)
                assert np.all(pairs[:, 1] == 1.0) and mass == 1.0, (where, mass)
                assert np.all(pairs[:, 2] >= 0.0) and np.all((pairs[:, 2] > 0) == (vals > 0)), where
                if rows_r is None:
                    rows_r = pairs[:, 2].copy()
                assert np.array_equal(_u32(pairs[:, 2]), _u32(rows_r)), where          # r: no loss and no delta in it
                lvalue, lmass, lpairs = m.evaluate_robust_pairs(idx, LOSS_CODES[loss], delta, want_pairs=True)
                assert np.array_equal(_u32(lpairs[:, 0]), _u32(listed)) and _u64(lvalue)[()] == _u64(list_mean)[()], where
                assert np.array_equal(_u32(lpairs), _u32(pairs)) and lmass == 1.0, where
        m.close()


@pytest.mark.parametrize("case", LABELS, indirect=True)
def test_pair_terms_against_the_direct_oracle(case):
    """{c, u, r} of every pair (case e: the oracle's sample of the pairs) against the float64 statement, at both scales of the case
    (half and a tenth of the samples outside delta) and for all three losses: 1e-6 of the scale under the reference arithmetic, 1e-3
    on the throughput paths -- the scale s = w06 sum d^2 for c, 1 for u, and for r that raw sum in r's own units (r itself); value and
    inlier_mass to 1e-5 relative.  The worst ratios of a GPU run are recorded in DESIGN.md 4.19."""
    failures = []
    for sampling, _ in case.setups:
        rec = case.reached(sampling)
        assert np.max(np.abs(rec["kmax"] - case.K01s[:, 15])) <= 1e-3   # the records describe the oracle's ranges, in its pair order
        tol = T.tolerance(sampling, case.N)
        m = case.metric(sampling)
        for scale in R.SCALES:
            delta = R.case_delta(case.label, scale)
            for loss in R.LOSSES:
                t = R.case_terms(case.label, loss, scale)
                rows = t["pairs"]
                want, scales = R.columns(t)
                value, mass, pairs = m.evaluate_robust(LOSS_CODES[loss], delta, want_pairs=True)
                assert np.all(np.isfinite(pairs)) and np.isfinite(value)
                assert np.all(pairs[:, 1] > 0.0) and np.all(pairs[:, 1] <= 1.0)
                ratio = T.compare(pairs[rows], want, scales, tol)
                line = "case %s %-10s %-13s %-6s (delta %.6g): c %.3g of the bar %.0e, u %.3g, r %.3g" % (
                    case.label, sampling, loss, scale, delta, ratio[0], tol, ratio[1], ratio[2])
                if tol == T.TOL_THROUGHPUT:   # reported: the same against the float64-position statement
                    c64, _ = R.columns(R.case_terms(case.label, loss, scale, "float64"))
                    r64 = T.compare(pairs[rows], c64, scales, tol)
                    line += "; against float64 positions c %.3g, u %.3g, r %.3g" % (r64[0], r64[1], r64[2])
                if "value" in t:
                    ev, em = abs(value - t["value"]) / (T.TOL_MEAN * t["value"]), abs(mass - t["inlier_mass"]) / (T.TOL_MEAN * t["inlier_mass"])
                    line += "; value %.3g of the bar 1e-05, inlier mass %.3g" % (ev, em)
                    ratio = np.append(ratio, [ev, em])
                print(line)
                if not ratio.max() <= 1.0:
                    failures.append(line)
        m.close()
    assert not failures, "\n".join(failures)


# ---- the reason the call exists: a block nobody flagged ---------------------------------------------------------------------------
BAD_VIEW = 3


@pytest.fixture(scope="module")
def block_scan(gpu_ctx, small_scan, oracle_mod):
    """The clean and the corrupted scan of tests/test_gpu_weighted.py (8 views of the spheres at 128^2 -> 96^2 bins, the opaque block
    in view 3) on the device, and the oracle's residuals of the corrupted one from its own intermediates.  Made once for the module."""
    import epipolarconsistency_amd as E
    imgs, B = small_scan["imgs"], 96
    bad = np.array(imgs, np.float32)
    bad[BAD_VIEW][BLOCK] += 4.0 * float(np.max(imgs[BAD_VIEW]))
    clean_d = E.RadonIntermediate.compute_batch(gpu_ctx, np.asarray(imgs, np.float32), B, B)
    bad_d = E.RadonIntermediate.compute_batch(gpu_ctx, bad, B, B)
    host = [d.readback() for d in bad_d]
    K01s = oracle_mod.evaluate_all(small_scan["Ps"], host, 128, 128, want_K01=True)["K01s"]
    res = R.scan_residuals(small_scan["Ps"], host, 128, 128, K01s)
    yield dict(clean=clean_d, bad=bad_d, K01s=K01s, res=res)
    _close(clean_d + bad_d)


@pytest.mark.parametrize("sampling", ["polynomial", "per_sample", "auto"])
def test_a_block_nobody_flagged(gpu_ctx, small_scan, block_scan, sampling):
    """delta = robust_scale of the corrupted scan's own delta = inf call: within 1e-3 relative of robust_terms' figure for the same
    data.  For each loss the pairs without view 3 have the same bits on the clean and on the corrupted scan; corrupted / clean is
    ordered truncated < Huber < evaluate() and Geman-McClure < Huber; and under the truncated loss no pair exceeds
    K0[6] dkappa delta^2 2 n_kappa (1 + 1e-5), with K0[6], dkappa and n_kappa from the oracle's K01."""
    import epipolarconsistency_amd as E
    b = block_scan
    Ps, n = small_scan["Ps"], len(small_scan["Ps"])
    iu = np.triu_indices(n, 1)
    hit = (iu[0] == BAD_VIEW) | (iu[1] == BAD_VIEW)
    assert hit.sum() == n - 1
    m_bad = E.MetricRadonIntermediate(gpu_ctx, Ps, b["bad"]).setSampling(sampling)
    m_clean = E.MetricRadonIntermediate(gpu_ctx, Ps, b["clean"]).setSampling(sampling)
    e_bad, _, first = m_bad.evaluate_robust(E.LOSS_HUBER, float("inf"), want_pairs=True)
    e_clean = m_clean.evaluate()
    assert _u64(e_bad)[()] == _u64(m_bad.evaluate())[()]
    delta = E.robust_scale(first)
    want_delta = R.robust_scale(R.scan_terms(b["res"], "huber", np.inf)["r"])
    print("%s: delta %.6g (oracle %.6g); pooled rms %.4g; evaluate() clean %.6g, corrupted %.6g (x %.4g)" % (
        sampling, delta, want_delta, np.sqrt(first[:, 2].astype(np.float64).mean()), e_clean, e_bad, e_bad / e_clean))
    assert delta > 0 and abs(delta - want_delta) <= 1e-3 * want_delta, (delta, want_delta)
    ratios = {"evaluate": e_bad / e_clean}
    for loss in R.LOSSES:
        v_bad, u_bad, p_bad = m_bad.evaluate_robust(LOSS_CODES[loss], delta, want_pairs=True)
        v_clean, u_clean, p_clean = m_clean.evaluate_robust(LOSS_CODES[loss], delta, want_pairs=True)
        assert np.array_equal(_u32(p_bad[~hit]), _u32(p_clean[~hit])), loss
        assert not np.array_equal(_u32(p_bad[hit]), _u32(p_clean[hit])), loss
        ratios[loss] = v_bad / v_clean
        print("%s %-13s: clean %.6g (inlier mass %.4f), corrupted %.6g (%.4f): x %.4g" % (sampling, loss, v_clean, u_clean, v_bad, u_bad, ratios[loss]))
        if loss == "truncated":
            K01 = np.asarray(b["K01s"], np.float32)
            n_kappa = np.array([len(T.kappa_grid(k)) for k in K01])
            bound = K01[:, 6].astype(np.float64) * K01[:, 14].astype(np.float64) * float(np.float32(delta)) ** 2 * 2 * n_kappa * (1 + 1e-5)
            for p in (p_bad, p_clean):
                assert np.all(p[:, 0].astype(np.float64) <= bound), (p[:, 0] / bound).max()
    m_bad.close()
    m_clean.close()
    assert ratios["truncated"] < ratios["huber"] < ratios["evaluate"], ratios
    assert ratios["geman_mcclure"] < ratios["huber"], ratios


# ---- repeatability, nothing else moved, edge cases, errors --------------------------------------------------------------------------
def test_repeatable_and_nothing_else_moved(gpu_ctx, oracle_mod):
    """Two calls give identical bits; evaluate() (with one view moved and back), a pose-delta evaluation on the same metric and
    evaluate_weighted on a second metric of the same context keep their bits around robust calls of both forms."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import geometry as Gm
    c = _Case(gpu_ctx, "i")
    ws = [E.RadonIntermediate.from_host(gpu_ctx, f, c.n_u, c.n_v, filter=E.FILTER_NONE) for f in c.weights]
    try:
        n = c.n
        m = c.metric("polynomial")
        m2 = c.metric("polynomial", ws)
        delta = R.case_delta("i", "median")
        idx = _all_pairs_list(n)[::3]
        P0 = E.pack_projection_matrices(c.Ps)
        P1 = P0.copy()
        P1[n // 2] = E.pack_projection_matrices([Gm.compose_transform(P0[n // 2].reshape(4, 3).T, Gm.rigid_transform(tx=3.0, ry=0.01))])[0]

        def observe():
            base = m.setProjectionMatrices(P0).evaluate()
            moved = m.setProjectionMatrices(P1).evaluate()
            back = m.setProjectionMatrices(P0).evaluate()
            deltas = m.evaluate_pose_deltas([n // 2, 1], np.stack([P1[n // 2], P0[2]]))
            weighted = m2.evaluate_weighted(want_pairs=True)
            cost = np.zeros((n, n), np.float32)
            with_cost = m.evaluate(cost)
            return np.concatenate([[base, moved, back, with_cost], np.ravel(deltas), weighted[:2]]), cost, weighted[2]
        before, cost_b, wp_b = observe()
        first = m.evaluate_robust(E.LOSS_HUBER, delta, want_pairs=True)
        second = m.evaluate_robust(E.LOSS_HUBER, delta, want_pairs=True)
        lfirst = m.evaluate_robust_pairs(idx, E.LOSS_GEMAN_MCCLURE, delta, want_pairs=True)
        on_second = m2.evaluate_robust(E.LOSS_HUBER, delta, want_pairs=True)   # a 2 n metric: its first n intermediates are the data
        lsecond = m.evaluate_robust_pairs(idx, E.LOSS_GEMAN_MCCLURE, delta, want_pairs=True)
        after, cost_a, wp_a = observe()
        assert np.array_equal(_u64(before), _u64(after)) and np.array_equal(_u32(cost_b), _u32(cost_a)) and np.array_equal(_u32(wp_b), _u32(wp_a))
        for x, y in ((first, second), (lfirst, lsecond), (first, on_second)):
            assert _u64(x[0])[()] == _u64(y[0])[()] and _u64(x[1])[()] == _u64(y[1])[()] and np.array_equal(_u32(x[2]), _u32(y[2]))
        assert m.evaluate_robust(E.LOSS_HUBER, delta) == first[:2]   # without the pair terms: the same two numbers
        assert first[1] < 1.0 and first[0] < before[0]
        # in the middle of a sequence: matrices moved, then the call, then back
        m.setProjectionMatrices(P1).evaluate()
        moved = m.evaluate_robust(E.LOSS_HUBER, delta)
        assert _u64(m.evaluate())[()] == _u64(before[1])[()]          # the moved matrices are still current
        assert _u64(m.setProjectionMatrices(P0).evaluate())[()] == _u64(before[0])[()]
        again = m.evaluate_robust(E.LOSS_HUBER, delta, want_pairs=True)
        assert _u64(again[0])[()] == _u64(first[0])[()] and np.array_equal(_u32(again[2]), _u32(first[2])) and moved[0] != first[0]
        m.close()
        m2.close()
    finally:
        _close(ws)
        c.close()


def test_edge_cases_of_the_list_form(gpu_ctx, oracle_mod):
    """n_pairs == 0: ECC_OK and nothing written; a tuple with P0 == P1 has no samples, {0, 1, 0}, and counts in the means; data indices
    need not follow the matrix indices; tuples (i, j, i, j) in another order carry the all-pairs rows of the same resolved mode."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib
    c = _Case(gpu_ctx, "d")
    try:
        m = c.metric("reference")   # fixed, so that every list length resolves alike
        delta = R.case_delta("d", "median")
        _, _, rows = m.evaluate_robust(E.LOSS_TRUNCATED, delta, want_pairs=True)
        value, mass, terms = C.c_double(-1.0), C.c_double(-1.0), np.full(3, -1.0, np.float32)
        idx1 = np.array([[0, 1, 0, 1]], np.int32)
        for lst in (None, C.c_void_p(idx1.ctypes.data)):
            assert _lib.lib().ecc_metric_evaluate_robust_pairs(m._h, lst, 0, E.LOSS_TRUNCATED, float(delta), C.byref(value), C.byref(mass),
                                                               C.c_void_p(terms.ctypes.data)) == 0
        assert value.value == -1.0 and mass.value == -1.0 and np.all(terms == -1.0)
        assert m.evaluate_robust_pairs(np.zeros((0, 4), np.int32), E.LOSS_TRUNCATED, delta, want_pairs=True)[2].shape == (0, 3)
        full = _all_pairs_list(c.n)
        pick = np.array([5, 0, 17, 9])
        idx = np.concatenate([full[pick], [[2, 2, 2, 3]]]).astype(np.int32)
        v, u, p = m.evaluate_robust_pairs(idx, E.LOSS_TRUNCATED, delta, want_pairs=True)
        assert np.array_equal(_u32(p[:4]), _u32(rows[pick])) and np.array_equal(p[4], [0.0, 1.0, 0.0]), p
        assert abs(v - p[:, 0].astype(np.float64).sum() / 5) <= 1e-12 * v and abs(u - p[:, 1].astype(np.float64).sum() / 5) <= 1e-15
        swapped = np.array([[0, 1, 1, 0], [0, 1, 0, 1]], np.int32)   # the data of the other view on each side: another pair value
        _, _, ps = m.evaluate_robust_pairs(swapped, E.LOSS_TRUNCATED, delta, want_pairs=True)
        assert np.array_equal(_u32(ps[1]), _u32(rows[0])) and ps[0, 0] != ps[1, 0] and ps[0, 2] > 0
        m.close()
    finally:
        c.close()


def test_errors(gpu_ctx, oracle_mod):
    """Every argument error of the header on a live metric, through the C calls themselves: the code, and nothing written."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib
    L = _lib.lib()
    c = _Case(gpu_ctx, "d")
    try:
        m = c.metric("auto")
        delta = float(R.case_delta("d", "p90"))
        want = m.evaluate_robust(E.LOSS_HUBER, delta, want_pairs=True)
        value, mass, terms = C.c_double(-1.0), C.c_double(-1.0), np.full((c.N, 3), -1.0, np.float32)
        out = (C.byref(value), C.byref(mass), C.c_void_p(terms.ctypes.data))
        idx = _all_pairs_list(c.n)
        pidx = C.c_void_p(idx.ctypes.data)

        def both(h, loss, d, outs=out, lst=pidx, count=len(idx)):
            return (L.ecc_metric_evaluate_robust(h, loss, d, *outs), L.ecc_metric_evaluate_robust_pairs(h, lst, count, loss, d, *outs))
        assert both(m._h, 0, delta, outs=(None, out[1], out[2])) == (1, 1)                      # value == NULL
        for loss in (-1, 3, 100):
            assert both(m._h, loss, delta) == (1, 1), loss
        for d in (0.0, -1.0, float("nan"), float("-inf")):
            assert both(m._h, 0, d) == (1, 1), d
        assert L.ecc_metric_evaluate_robust_pairs(m._h, None, 2, 0, delta, *out) == 1          # idx4 == NULL with n_pairs > 0
        assert L.ecc_metric_evaluate_robust_pairs(m._h, pidx, -1, 0, delta, *out) == 1         # n_pairs < 0
        for bad in ([0, c.n, 0, 1], [-1, 1, 0, 1], [0, 1, c.n, 1], [0, 1, 0, -1]):              # a bad tuple, behind good ones
            lst = np.concatenate([idx[:3], [bad]]).astype(np.int32)
            assert L.ecc_metric_evaluate_robust_pairs(m._h, C.c_void_p(lst.ctypes.data), 4, 0, delta, *out) == 1, bad
            assert L.ecc_last_error().endswith(b"index array contains invalid indices")        # the robust list's own, short text
        assert L.ecc_metric_evaluate_robust_pairs(m._h, None, 0, 7, delta, *out) == 1           # an empty list: the checks come first
        assert L.ecc_metric_evaluate_robust_pairs(m._h, None, 0, 0, -1.0, *out) == 1
        m.useCorrelation(True)
        assert both(m._h, 0, delta) == (5, 5)                                                   # ECC_ERR_UNSUPPORTED
        assert both(m._h, 0, delta, lst=None, count=0)[1] == 5                                  # ... of an empty list as well
        with pytest.raises(E.EccError) as e:
            m.evaluate_robust(E.LOSS_HUBER, delta)
        assert e.value.code == 5, e.value
        m.useCorrelation(False)
        one = E.MetricRadonIntermediate(gpu_ctx, c.Ps[:1], c.data[:1])                          # fewer than two views
        none = E.MetricRadonIntermediate(gpu_ctx, None, c.data)                                 # no matrices set
        for other in (one, none):
            assert both(other._h, 0, delta, lst=pidx, count=1) == (1, 1)
            assert both(other._h, 0, delta, lst=None, count=0)[1] == 1                          # an empty list: the checks come first
            with pytest.raises(E.EccError) as e:
                other.evaluate_robust(E.LOSS_HUBER, delta)
            assert e.value.code == 1
            other.close()
        few = E.MetricRadonIntermediate(gpu_ctx, c.Ps, c.data[:-1])                             # fewer intermediates than views
        assert L.ecc_metric_evaluate_robust(few._h, 0, delta, *out) == 1 and b"fewer Radon intermediates" in L.ecc_last_error()
        few.close()
        assert value.value == -1.0 and mass.value == -1.0 and np.all(terms == -1.0)            # nothing written by any of them
        more = E.MetricRadonIntermediate(gpu_ctx, c.Ps, c.data + c.data[:1])                    # D* are bounded by the intermediates held
        rows = [more.evaluate_robust_pairs(np.array([[0, 1, D0, 1]], np.int32), E.LOSS_HUBER, delta, want_pairs=True)[2] for D0 in (0, c.n)]
        assert np.array_equal(_u32(rows[0]), _u32(rows[1])) and rows[0][0, 2] > 0
        with pytest.raises(E.EccError):
            more.evaluate_robust_pairs(np.array([[0, 1, c.n + 1, 1]], np.int32), E.LOSS_HUBER, delta)
        more.close()
        again = m.evaluate_robust(E.LOSS_HUBER, delta, want_pairs=True)
        assert _u64(again[0])[()] == _u64(want[0])[()] and np.array_equal(_u32(again[2]), _u32(want[2]))
        m.close()
    finally:
        c.close()
