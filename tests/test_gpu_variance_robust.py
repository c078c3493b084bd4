"""ecc_metric_evaluate_variance_robust on the GPU (csrc/ecc_variance_robust.hip, csrc/variance_robust_kernel.hip): inverse-variance
sample weights and a robust loss of the studentised residual.  The cases are variance_terms.CASES with their data, variance fields and
floors -- the geometries, grids and settings that select each kernel and loop (labels a .. j); each case asserts from
the records of a single-channel metric that it reached its loop class, as tests/test_gpu_variance.py does.

  infinite_delta     delta = inf: {c, u}, value and mean weight have the bits of evaluate_variance, k has u's, inlier mass == 1.0;
  half_is_robust     V == 0.5f, floor 0.25 and 1.0: {c, k, r}, value and inlier mass have the bits of evaluate_robust's {c, u, r} at the
                     same loss and delta on the n-view metric, u == 1.0 and mean weight == 1.0; with delta = inf the bits of evaluate();
  scale_invariance   all V and the floor x 4, delta x 1/2: every column x 1/4 exactly, value and inlier mass keep their bits;
  statement          {c, u, k, r} of every pair against variance_robust_terms at the six combinations
                     (tests/test_variance_robust_terms_oracle.py shows that this comparison rejects the slips it is there for), the
                     three results to 1e-5;
  demonstration      the reason the call exists: known noise in half of one view AND a block nobody flagged in another;
  repeatability, errors."""
import ctypes as C

import numpy as np
import pytest

import channel_terms as T
import robust_terms as R
import variance_robust_terms as VR
import variance_terms as V
from test_gpu_variance import _Case, _close, _plain, _u32, _u64

pytestmark = pytest.mark.gpu

INF = float("inf")
LOSS_CODES = {"huber": 0, "truncated": 1, "geman_mcclure": 2}   # ECC_LOSS_* == E.LOSS_*
LABELS = sorted(VR.CASES)


@pytest.fixture
def case(gpu_ctx, oracle_mod, request):
    c = _Case(gpu_ctx, request.param)
    try:
        yield c
    finally:
        c.close()


def test_loss_codes():
    import epipolarconsistency_amd as E
    assert (E.LOSS_HUBER, E.LOSS_TRUNCATED, E.LOSS_GEMAN_MCCLURE) == (0, 1, 2) and tuple(R.LOSSES) == tuple(LOSS_CODES)


@pytest.mark.parametrize("case", LABELS, indirect=True)
def test_infinite_delta_is_evaluate_variance(case):
    """delta = +inf: thr = inf, t = fminf(1, inf) = 1, w = 1 (Geman-McClure: inv_delta = 0, q = 0, w = 1 / 1), f = om * 1.0f = om --
    pairs[:, :2], value and mean weight have the bits of evaluate_variance at the same floor, pairs[:, 2] those of pairs[:, 1], and
    the inlier mass is 1.0, for the three losses, at both floors, in every case and sampling mode of the table."""
    vs = case.variance_dtrs(case.variances)
    for sampling, _ in case.setups:
        m = case.metric(sampling, vs)
        for floor in VR.FLOORS:
            value, mean_weight, rows = m.evaluate_variance(floor, want_pairs=True)
            for loss in VR.LOSSES:
                got = m.evaluate_variance_robust(LOSS_CODES[loss], INF, floor, want_pairs=True)
                assert got[3].shape == (case.N, 4) and got[3].dtype == np.float32
                assert np.array_equal(_u32(got[3][:, :2]), _u32(rows)), (sampling, floor, loss, np.max(np.abs(got[3][:, :2] - rows)))
                assert np.array_equal(_u32(got[3][:, 2]), _u32(got[3][:, 1])), (sampling, floor, loss)
                assert _u64(got[0])[()] == _u64(value)[()] and _u64(got[1])[()] == _u64(mean_weight)[()], (sampling, floor, loss)
                assert got[2] == 1.0, (sampling, floor, loss, got[2])
                assert (got[3][:, 3] > 0).sum() >= 0.8 * case.N
        m.close()


@pytest.mark.parametrize("case", LABELS, indirect=True)
def test_half_is_evaluate_robust(case):
    """V == 0.5f: s == 1.0f, sc == 1.0f under floor 0.25 and floor 1.0 alike, om == 1.0f, thr == delta * 1.0f, q * om == q, f == w:
    pairs[:, (0, 2, 3)], value and inlier mass have the bits of evaluate_robust's rows {c, u, r}, value and inlier mass at the same loss
    and delta on the metric over the n data intermediates; pairs[:, 1] == 1.0 and the mean weight == 1.0.  The deltas are
    robust_terms' two scales of the case and +inf, at which value and pairs[:, 0] also have the bits of evaluate()."""
    half = case.constant(0.5)
    deltas = [float(R.case_delta(case.label, scale)) for scale in R.SCALES] + [INF]
    for sampling, _ in case.setups:
        m = case.metric(sampling, half)
        plain_metric = case.E.MetricRadonIntermediate(case.ctx, case.Ps, case.data).setSampling(sampling)
        plain_metric.setObjectRadius(case.radius)
        plain_metric.setEpipolarPlaneStep(case.dkappa)
        plain, _, vals = _plain(m, case.n)
        for loss in VR.LOSSES:
            for delta in deltas:
                want = plain_metric.evaluate_robust(LOSS_CODES[loss], delta, want_pairs=True)
                for floor in (0.25, 1.0):
                    got = m.evaluate_variance_robust(LOSS_CODES[loss], delta, floor, want_pairs=True)
                    where = (sampling, loss, delta, floor)
                    assert np.array_equal(_u32(got[3][:, [0, 2, 3]]), _u32(want[2])), (where, np.max(np.abs(got[3][:, [0, 2, 3]] - want[2])))
                    assert np.all(got[3][:, 1] == 1.0) and got[1] == 1.0, where
                    assert _u64(got[0])[()] == _u64(want[0])[()] and _u64(got[2])[()] == _u64(want[1])[()], (where, got[:3], want[:2])
                    if delta == INF:
                        assert np.array_equal(_u32(got[3][:, 0]), _u32(vals)) and _u64(got[0])[()] == _u64(plain)[()] and got[2] == 1.0, where
                    else:
                        assert got[2] < 1.0, where
        plain_metric.close()
        m.close()
        assert (vals > 0).sum() >= 0.8 * case.N


@pytest.mark.parametrize("case", LABELS, indirect=True)
def test_scale_invariance(case):
    """The case's fields and floors, then all of them x 4 with delta x 1/2 (all exact in float32): sc is 4 x as large, om a quarter,
    thr = (delta / 2) * (2 sqrtf(sc)) and (q * om) * q are what they were -- every column x 0.25 bit for bit, the same value and inlier
    mass bits, a quarter of the mean weight.  V is a variance only up to a constant factor, and delta absorbs it."""
    vs = case.variance_dtrs(case.variances)
    vs4 = case.variance_dtrs([np.float32(4.0) * f for f in case.variances])
    for sampling, _ in case.setups:
        m, m4 = case.metric(sampling, vs), case.metric(sampling, vs4)
        for loss, floor, scale in VR.COMBOS:
            delta = VR.case_delta(case.label, scale)
            half_delta = np.float32(0.5) * delta
            assert np.float32(2.0) * half_delta == delta
            got = m.evaluate_variance_robust(LOSS_CODES[loss], float(delta), floor, want_pairs=True)
            got4 = m4.evaluate_variance_robust(LOSS_CODES[loss], float(half_delta), 4.0 * floor, want_pairs=True)
            where = (sampling, loss, floor, scale)
            assert np.array_equal(_u32(got4[3]), _u32(np.float32(0.25) * got[3])), (where, np.max(np.abs(got4[3] - 0.25 * got[3]), axis=0))
            assert _u64(got4[0])[()] == _u64(got[0])[()] and _u64(got4[2])[()] == _u64(got[2])[()], (where, got[:3], got4[:3])
            assert _u64(got4[1])[()] == _u64(0.25 * got[1])[()], where
            assert got[2] < 1.0 and np.all(got[3][:, 2] <= got[3][:, 1])   # the loss is seen
        m.close()
        m4.close()


@pytest.mark.parametrize("case", LABELS, indirect=True)
def test_pair_terms_against_the_direct_statement(case):
    """{c, u, k, r} of every pair (case e: the statement's sample of the pairs) against the float64 statement at the six (loss, floor,
    scale) combinations: 1e-6 of the scale under the reference arithmetic, 1e-3 on the throughput paths, the scales s omega_max for c,
    omega_max for u and k, the mean raw square x omega_max for r; value, mean weight and inlier mass to 1e-5 relative.  The worst
    ratios of a GPU run are recorded in DESIGN.md 4.30."""
    vs = case.variance_dtrs(case.variances)
    failures = []
    for sampling, _ in case.setups:
        t0 = VR.case_terms(case.label, *VR.COMBOS[0])
        rec = case.reached(sampling, t0)
        assert np.max(np.abs(rec["kmax"] - case.K01s[:, 15])) <= 1e-3   # the records describe the statement's ranges, in its pair order
        tol = T.tolerance(sampling, case.N)
        m = case.metric(sampling, vs)
        for loss, floor, scale in VR.COMBOS:
            t = VR.case_terms(case.label, loss, floor, scale)
            rows = t["pairs"]
            want, scales = VR.columns(t)
            value, mean_weight, inlier_mass, pairs = m.evaluate_variance_robust(LOSS_CODES[loss], float(VR.case_delta(case.label, scale)), floor,
                                                                                want_pairs=True)
            assert np.all(np.isfinite(pairs)) and np.isfinite(value)
            ratio = T.compare(pairs[rows], want, scales, tol)
            line = "case %s %s %s floor %g %s: c %.3g of the bar %.0e, u %.3g, k %.3g, r %.3g" % (
                case.label, sampling, loss, floor, scale, ratio[0], tol, ratio[1], ratio[2], ratio[3])
            if tol == T.TOL_THROUGHPUT:   # reported: the same against the float64-position statement
                c64, _ = VR.columns(VR.case_terms(case.label, loss, floor, scale, "float64"))
                r64 = T.compare(pairs[rows], c64, scales, tol)
                line += "; against float64 positions c %.3g, u %.3g, k %.3g, r %.3g" % (r64[0], r64[1], r64[2], r64[3])
            if "value" in t:
                means = [abs(g - t[key]) / (T.TOL_MEAN * t[key]) for g, key in ((value, "value"), (mean_weight, "mean_weight"), (inlier_mass, "inlier_mass"))]
                line += "; value %.3g of the bar 1e-05, mean weight %.3g, inlier mass %.3g" % tuple(means)
                ratio = np.append(ratio, means)
            print(line)
            if not ratio.max() <= 1.0:
                failures.append(line)
        m.close()
    assert not failures, "\n".join(failures)


# ---- demonstration: the reason the feature exists --------------------------------------------------------------------------------
def test_known_noise_and_a_block_nobody_flagged(gpu_ctx, oracle_mod):
    """8 views of the spheres at 128^2 -> 96^2 bins; Gaussian noise of 5 % of the view's maximum on the left half of view 3 with its
    variance known (V = variance_intermediates, floor = variance_floor of V_3); on top of it the opaque block pasted unflagged into
    view 5.  delta = variance_robust_scale(rows at delta = inf, 2.0) of the corrupted scan itself (the raw loss: robust_scale(., 2.0)
    of it).  On the device, from the device's own Radon intermediates, corrupted / clean of each form equals the float64 statement's
    ratio, computed from the same intermediates at the same float32 deltas, to 1e-5 relative; and
        noise + block: the variance form alone >= 100, the raw truncated loss >= 2, the studentised truncated loss <= 1.5;
        noise only:    the studentised truncated loss <= 1.05."""
    import epipolarconsistency_amd as E
    from conftest import make_small_scan
    Ps, imgs = make_small_scan()
    noisy, both, var = VR.demo_images(imgs)
    B, n = V.DEMO_BINS, len(Ps)
    dev = {key: E.RadonIntermediate.compute_batch(gpu_ctx, np.asarray(x, np.float32), B, B) for key, x in (("clean", imgs), ("noisy", noisy), ("both", both))}
    var_d = E.variance_intermediates(gpu_ctx, var, B, B)
    TR = E.LOSS_TRUNCATED
    try:
        fields = [v.readback().copy() for v in var_d]
        floor = E.variance_floor(fields[V.DEMO_VIEW], V.DEMO_FLOOR_FRACTION)
        assert floor == V.demo_floor(fields) and floor > 0
        host = {key: [d.readback().copy() for d in ds] for key, ds in dev.items()}
        K = {key: oracle_mod.evaluate_all(Ps, host[key], 128, 128, want_K01=True)["K01s"] for key in host}
        metrics = {key: (E.MetricRadonIntermediate(gpu_ctx, Ps, ds + var_d).setSampling("auto"),     # 28 pairs: the reference arithmetic
                         E.MetricRadonIntermediate(gpu_ctx, Ps, ds).setSampling("auto")) for key, ds in dev.items()}
        out = {}
        for key in ("noisy", "both"):
            bad, bad_raw = metrics[key]
            clean, clean_raw = metrics["clean"]
            delta = float(np.float32(E.variance_robust_scale(bad.evaluate_variance_robust(TR, INF, floor, want_pairs=True)[3], VR.DEMO_K)))
            raw_delta = float(np.float32(E.robust_scale(bad_raw.evaluate_robust(TR, INF, want_pairs=True)[2], VR.DEMO_K)))
            assert delta > 0 and raw_delta > 0
            got = {"evaluate": bad.evaluate() / clean.evaluate(),
                   "variance": bad.evaluate_variance(floor)[0] / clean.evaluate_variance(floor)[0],
                   "raw_truncated": bad_raw.evaluate_robust(TR, raw_delta)[0] / clean_raw.evaluate_robust(TR, raw_delta)[0],
                   "studentised_truncated": bad.evaluate_variance_robust(TR, delta, floor)[0] / clean.evaluate_variance_robust(TR, delta, floor)[0]}
            f = VR.demo_forms(Ps, host["clean"], host[key], fields, floor, 128, 128, K["clean"], K[key], delta=delta, raw_delta=raw_delta)
            want = {form: VR.demo_ratio(f, form) for form in got}
            assert abs(delta - f["own_delta"]) <= 1e-3 * delta and abs(raw_delta - f["own_raw_delta"]) <= 1e-3 * raw_delta, (delta, raw_delta, f)
            print("%-5s floor %.4g, delta %.6g sigmas, raw delta %.6g: %s" % (
                key, floor, delta, raw_delta, ", ".join("%s x %.5f (statement %.5f)" % (form, got[form], want[form]) for form in got)))
            for form in got:
                assert abs(got[form] - want[form]) <= 1e-5 * want[form], (key, form, got[form], want[form])
            out[key] = got
        for pair in metrics.values():
            for m in pair:
                m.close()
        assert out["both"]["variance"] >= 100.0, out
        assert out["both"]["raw_truncated"] >= 2.0, out
        assert out["both"]["studentised_truncated"] <= 1.5, out
        assert out["noisy"]["studentised_truncated"] <= 1.05, out
    finally:
        _close([d for ds in dev.values() for d in ds] + var_d)


# ---- repeatability, errors -------------------------------------------------------------------------------------------------------
def test_repeatable_and_nothing_else_moved(gpu_ctx, oracle_mod):
    """Two calls give identical bits; evaluate(), evaluate(cost) and a pose batch around the call are unchanged; without the pair terms
    the same three numbers; loss, delta and floor are seen."""
    c = _Case(gpu_ctx, "i")
    try:
        n = c.n
        m = c.metric("polynomial", c.variance_dtrs(c.variances))
        P0 = c.E.pack_projection_matrices(c.Ps)
        delta = float(VR.case_delta("i", "p90"))

        def observe():
            cost = np.zeros((n, n), np.float32)
            return np.concatenate([[m.evaluate(), m.evaluate(cost)], np.ravel(m.evaluate_pose_deltas([n // 2, 1], np.stack([P0[1], P0[2]])))]), cost
        before, cost_b = observe()
        first = m.evaluate_variance_robust(1, delta, VR.FLOORS[1], want_pairs=True)
        second = m.evaluate_variance_robust(1, delta, VR.FLOORS[1], want_pairs=True)
        after, cost_a = observe()
        assert np.array_equal(_u64(before), _u64(after)) and np.array_equal(_u32(cost_b), _u32(cost_a))
        assert all(_u64(first[k])[()] == _u64(second[k])[()] for k in range(3)) and np.array_equal(_u32(first[3]), _u32(second[3]))
        assert m.evaluate_variance_robust(1, delta, VR.FLOORS[1]) == first[:3]
        for other in (m.evaluate_variance_robust(0, delta, VR.FLOORS[1]), m.evaluate_variance_robust(1, 0.5 * delta, VR.FLOORS[1]),
                      m.evaluate_variance_robust(1, delta, VR.FLOORS[0])):
            assert other[0] != first[0] and other[2] != first[2]
        m.close()
    finally:
        c.close()


def _code(E, call):
    with pytest.raises(E.EccError) as e:
        call()
    return e.value.code, str(e.value)


def test_errors_in_the_stated_order(gpu_ctx, oracle_mod):
    """Every error of the all-pairs and of the list call, each in front of the ones behind it: a null value, the loss, delta (NaN, 0,
    negative) before the metric's shape; the shape before the floor; the floor before use_corr; all of them before a bad tuple; a
    negative list length and a null list before all of them.  After the checks an empty list writes nothing."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib
    L = _lib.lib()
    c = _Case(gpu_ctx, "d")
    try:
        vs = c.variance_dtrs(c.variances)
        m = c.metric("auto", vs)
        good = (1, 2.0, 1.5)
        want = m.evaluate_variance_robust(*good, want_pairs=True)
        idx = np.array([(0, 1, 0, 1), (2, 5, 2, 5)], np.int32)
        bad_idx = np.array([(0, 1, 0, c.n)], np.int32)
        value, u, k = C.c_double(-1.0), C.c_double(-1.0), C.c_double(-1.0)
        outs = (C.byref(value), C.byref(u), C.byref(k), None)
        last = lambda: L.ecc_last_error().decode()

        # on a good metric: each argument alone
        assert L.ecc_metric_evaluate_variance_robust(m._h, 1, 2.0, 1.5, None, C.byref(u), C.byref(k), None) == 1 and "value" in last()
        for loss in (-1, 3, 7):
            code, text = _code(E, lambda: m.evaluate_variance_robust(loss, 2.0, 1.5))
            assert code == 1 and "loss" in text
        for delta in (0.0, -1.0, float("nan"), -INF):
            code, text = _code(E, lambda: m.evaluate_variance_robust(1, delta, 1.5))
            assert code == 1 and "delta" in text
        for floor in (0.0, -1.0, float("nan"), INF, -INF):
            code, text = _code(E, lambda: m.evaluate_variance_robust(1, 2.0, floor))
            assert code == 1 and "floor" in text
        assert m.evaluate_variance_robust(1, INF, 1.5)[2] == 1.0   # +inf is a delta

        # value, loss and delta before the metric's shape; the shape before the floor
        shapeless = E.MetricRadonIntermediate(gpu_ctx, c.Ps, c.data + vs[:-1])
        assert L.ecc_metric_evaluate_variance_robust(shapeless._h, 7, 0.0, 0.0, None, None, None, None) == 1 and "value" in last()
        assert "loss" in _code(E, lambda: shapeless.evaluate_variance_robust(7, 0.0, 0.0))[1]
        assert "delta" in _code(E, lambda: shapeless.evaluate_variance_robust(1, 0.0, 0.0))[1]
        code, text = _code(E, lambda: shapeless.evaluate_variance_robust(1, 2.0, 0.0))
        assert code == 1 and "2 * n_views" in text
        assert "2 * n_views" in _code(E, lambda: shapeless.evaluate_variance_robust_pairs(bad_idx, 1, 2.0, 0.0))[1]
        shapeless.close()
        for dtrs in (c.data, c.data + vs + vs[:1]):
            other = E.MetricRadonIntermediate(gpu_ctx, c.Ps, dtrs)
            assert _code(E, lambda: other.evaluate_variance_robust(*good))[0] == 1
            other.close()
        one = E.MetricRadonIntermediate(gpu_ctx, c.Ps[:1], [c.data[0], vs[0]])   # fewer than two views, before n_dtrs and the floor
        assert "two views" in _code(E, lambda: one.evaluate_variance_robust(1, 2.0, 0.0))[1]
        one.close()
        none = E.MetricRadonIntermediate(gpu_ctx, None, c.data + vs)   # no matrices set
        assert "matrices" in _code(E, lambda: none.evaluate_variance_robust(1, 2.0, 0.0))[1]
        assert "delta" in _code(E, lambda: none.evaluate_variance_robust(1, -2.0, 0.0))[1]
        none.close()

        # the floor before use_corr, loss and delta before both; use_corr before a bad tuple
        m.useCorrelation(True)
        assert _code(E, lambda: m.evaluate_variance_robust(*good))[0] == 5   # ECC_ERR_UNSUPPORTED
        code, text = _code(E, lambda: m.evaluate_variance_robust(1, 2.0, 0.0))
        assert code == 1 and "floor" in text
        assert "delta" in _code(E, lambda: m.evaluate_variance_robust(1, 0.0, 1.5))[1] and "loss" in _code(E, lambda: m.evaluate_variance_robust(3, 2.0, 1.5))[1]
        assert _code(E, lambda: m.evaluate_variance_robust_pairs(bad_idx, *good))[0] == 5
        assert _code(E, lambda: m.evaluate_variance_robust_pairs(np.zeros((0, 4), np.int32), *good))[0] == 5   # an empty list is checked too
        m.useCorrelation(False)

        # the list form: its own checks first, a bad tuple last, an empty list after the checks
        p = C.c_void_p(idx.ctypes.data)
        assert L.ecc_metric_evaluate_variance_robust_pairs(m._h, p, -1, 7, 0.0, 0.0, None, None, None, None) == 1 and "negative" in last()
        assert L.ecc_metric_evaluate_variance_robust_pairs(m._h, None, 2, 7, 0.0, 0.0, None, None, None, None) == 1 and "index list is null" in last()
        assert L.ecc_metric_evaluate_variance_robust_pairs(m._h, p, 2, 7, 0.0, 0.0, None, None, None, None) == 1 and "value" in last()
        assert "loss" in _code(E, lambda: m.evaluate_variance_robust_pairs(bad_idx, 7, 0.0, 0.0))[1]
        assert "delta" in _code(E, lambda: m.evaluate_variance_robust_pairs(bad_idx, 1, 0.0, 0.0))[1]
        assert "floor" in _code(E, lambda: m.evaluate_variance_robust_pairs(bad_idx, 1, 2.0, 0.0))[1]
        for bad in ([(0, 1, 0, c.n)], [(0, c.n, 0, 1)], [(-1, 1, 0, 1)]):   # D indexes the data intermediates, P the matrices
            code, text = _code(E, lambda: m.evaluate_variance_robust_pairs(np.array(bad, np.int32), *good))
            assert code == 1 and "invalid indices" in text
        assert L.ecc_metric_evaluate_variance_robust_pairs(m._h, None, 0, 1, 2.0, 1.5, *outs) == 0
        assert L.ecc_metric_evaluate_variance_robust_pairs(m._h, None, 0, 1, 2.0, 0.0, *outs) == 1 and "floor" in last()
        assert value.value == -1.0 and u.value == -1.0 and k.value == -1.0   # nothing written, by the errors or by the empty list

        # a tuple with P0 == P1 has {0, 1, 1, 0}
        _, _, _, rows = m.evaluate_variance_robust_pairs(np.array([(3, 3, 3, 4), (0, 1, 0, 1)], np.int32), *good, want_pairs=True)
        assert rows[0].tolist() == [0.0, 1.0, 1.0, 0.0] and rows[1, 0] > 0

        again = m.evaluate_variance_robust(*good, want_pairs=True)   # nothing a later call can see has changed
        assert all(_u64(again[q])[()] == _u64(want[q])[()] for q in range(3)) and np.array_equal(_u32(again[3]), _u32(want[3]))
        m.close()
    finally:
        c.close()
