"""The pair values of useCorrelation(True) -- pairs_kernel<DERIV, true> and pairs_reference_*<true, ...>, 1 - cc per pair -- against
the direct float64 statement of tests/correlation_terms.py, on the geometries, grids and data kinds that select each loop
(correlation_terms.CASES; tests/test_correlation_terms_oracle.py holds the statement itself to the C oracle and shows that this
comparison rejects a weight, sign, view, trip or tail slip on every case).

|got - (1 - cc)| is compared absolutely (the Cauchy-Schwarz scale of cc is 1) at the project's bars: 1e-6 for the
reference arithmetic ("reference", "auto" at 512 pairs or fewer), 1e-3 for POLYNOMIAL and PER_SAMPLE against the float32-position
statement, 1e-5 relative on the mean.  The older tests see a correlation value only where cc is within 1e-2 of 1 (the consistent
small scan) or at 96 bins; here the signed samples of kappa_loop_poly<DERIV, true, ...> (each sample's own fold sign: the
squared-difference loops use the relative sign instead), the weight kappa_max / kappa of the three loops, the hand-over of one
set of moments from the polynomial part to the exact tail, DERIV = false under CORR and the three-moment wave tree and wave
partials of the reference kernels run under a checked value, away from cc = 1.

Each case asserts from the records of a polynomial-mode metric (debug_polynomials, debug_K01) and the statement's fold counts
that its pairs reach what it is there for, and prints its class counts, the loops reached and the worst distance per sampling and
fold class (throughput samplings: against the float64-position statement as well)."""
import numpy as np
import pytest

import channel_terms as T
import correlation_terms as CT

pytestmark = pytest.mark.gpu

FOLDS = ("same", "opposite", "mixed")


def _pitch_class(dtr, n_alpha):
    """Which PITCH4 the pair kernel's loops are instantiated with (csrc/ecc_pairs_device.h: poly_loop_dispatch; ecc_evaluate.hip:
    wide_offsets): -1 wide offsets (a row-paired copy of 2^24 bytes or more), 6400 (the 768-bin grid's row pitch), 0 generic."""
    pitch4 = dtr.device_view()[1] * 8
    if (n_alpha + 1) * pitch4 >= 1 << 24:
        return -1
    return 6400 if pitch4 == 6400 else 0


def _loop_degree(pitch_class, degree):
    """The DEG a recorded degree is dispatched to (poly_loop_dispatch)."""
    steps = (4, 6, 8, 10) if pitch_class == 6400 else (6, 10)
    return next(d for d in steps if degree <= d)


def _records(gpu_ctx, Ps, dtrs, radius, dkappa, pitch_class):
    """The pair records of a metric in POLYNOMIAL mode (tests/test_gpu_channel_terms.py::_records, with the degrees)."""
    import epipolarconsistency_amd as E
    n = len(Ps)
    n_pairs = n * (n - 1) // 2
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling("polynomial")
    m.setObjectRadius(radius)
    m.setEpipolarPlaneStep(dkappa)
    recs = m.debug_polynomials(0, n_pairs)
    K01 = m.debug_K01(0, n_pairs)
    m.close()
    ok = np.array([r["poly_ok"] for r in recs])
    free = np.array([r["clamp_free"] for r in recs])
    degree = np.array([r["degree"] for r in recs])
    folds_differ = np.array([bool(r["fold"][0]) != bool(r["fold"][1]) for r in recs])
    kmax = K01[:, 15]
    live = kmax > 0
    partial = ok & (kmax > float(CT.KAPPA_FIT_MAX))
    tail = (~ok & live) | partial
    # the clamp-free loops exist at pitch 6400 only
    loops = sorted({(pitch_class, bool(f) and pitch_class == 6400, _loop_degree(pitch_class, int(d))) for f, d in zip(free[ok], degree[ok])})
    return dict(ok=ok, free=free, degree=degree, folds_differ=folds_differ, kmax=kmax, dkappa=K01[:, 14], live=live, loops=loops,
                clamp_free=int((ok & free).sum()), clamped=int((ok & ~free).sum()), refused=int((~ok & live).sum()),
                partial=int(partial.sum()), above=int((kmax > np.pi / 4).sum()), poly_opposite=int((ok & folds_differ).sum()),
                exact_tail_above=int((tail & (kmax > np.pi / 4)).sum()), exact_tail_below=int((tail & (kmax <= np.pi / 4)).sum()))


COUNTS = ("clamp_free", "clamped", "refused", "partial", "above", "poly_opposite", "exact_tail_above", "exact_tail_below")

# The polynomial loops kappa_loop_poly<DERIV, true, PITCH4, DEG, 1, NOCLAMP> the POLYNOMIAL sampling of each case reaches, as
# (PITCH4, NOCLAMP, DEG): as seen on an MI355X (the fit's verdicts cannot be known without one).  Of the twelve loops per data kind
# (6400: clamp-free and clamped, degrees 4 / 6 / 8 / 10; wide offsets and generic pitch: 6 / 10) the derivative cases reach ten and
# the plain cases (c, c2, f) six; DESIGN.md 2 lists the rest.
LOOPS_SEEN = {
    "a": [(6400, True, 8), (6400, True, 10)],
    "a2": [(6400, True, 4), (6400, True, 6)],
    "b": [(6400, False, 8), (6400, False, 10), (6400, True, 10)],
    "c": [(6400, False, 8), (6400, False, 10), (6400, True, 10)],
    "c2": [(6400, True, 8), (6400, True, 10)],
    "d": [],                                   # every fit refused: the exact loop at generic pitch, with the reduction above pi/4
    "d2": [(0, False, 6), (0, False, 10)],
    "e": [(-1, False, 10)],
    "e2": [(-1, False, 6), (-1, False, 10)],
    "f": [(0, False, 6), (0, False, 10)],
}


def _reached(key, sampling, quads, rec, t, n_pairs, pitch_class, quad_bytes):
    """What the case is there for, from the records, the statement's fold counts and the metric's own memory report."""
    folds = {f: int((t["fold"] == f).sum()) for f in FOLDS}
    assert quad_bytes > 0 if quads == "on" else quad_bytes == 0, (quads, quad_bytes)
    if key in ("a", "c2"):   # pitch-6400 polynomial loops on pairs whose folds differ; the exact loop on opposite and mixed folds
        assert pitch_class == 6400 and rec["poly_opposite"] >= 10 and folds["opposite"] >= 30 and folds["mixed"] >= 5
        assert rec["exact_tail_above"] + rec["exact_tail_below"] >= 1
    elif key == "a2":        # the low degrees, on pairs whose folds differ too
        assert pitch_class == 6400 and rec["poly_opposite"] >= 10 and rec["refused"] == 0 and folds["opposite"] >= 30
    elif key in ("b", "c"):  # all four polynomial classes; the hand-over into an exact tail above pi/4 (row-quad copies when on)
        assert pitch_class == 6400 and rec["clamp_free"] > 0 and rec["clamped"] > 0 and rec["refused"] > 0 and rec["partial"] > 0
        assert rec["exact_tail_above"] >= 1
    elif key == "d":         # generic pitch, the exact loop alone (every fit is refused): ranges above pi/4 (the reduction), mixed folds
        assert pitch_class == 0 and rec["refused"] >= 100 and rec["above"] >= 10 and folds["mixed"] >= 5 and folds["opposite"] >= 1
    elif key == "d2":        # generic pitch, the polynomial loops, on pairs whose folds differ too
        assert pitch_class == 0 and rec["clamped"] + rec["clamp_free"] >= 100 and rec["poly_opposite"] >= 1
    elif key in ("e", "e2"): # the wide-offset loops
        assert pitch_class == -1 and rec["clamped"] + rec["clamp_free"] > 0
    elif key == "f":         # the caller's step reached the records; generic pitch on pairs whose folds differ
        assert np.all(rec["dkappa"][rec["live"]] == np.float32(0.004)) and pitch_class == 0 and rec["poly_opposite"] >= 5
    elif key == "g":         # "auto" at 512 pairs or fewer: the 1024-thread reference kernel
        assert sampling == "auto" and n_pairs <= 512 and folds["opposite"] >= 5 and folds["mixed"] >= 1
    elif key == "h":         # reference arithmetic, 513 .. 2 048 pairs: four waves per pair
        assert sampling == "reference" and 512 < n_pairs <= 2048 and folds["opposite"] >= 100 and folds["mixed"] >= 10
    else:                    # more than 2 048 pairs: one wave per pair
        assert key == "i" and sampling == "reference" and n_pairs > 2048 and folds["opposite"] >= 50 and folds["mixed"] >= 5
    if sampling == "polynomial":
        assert rec["loops"] == LOOPS_SEEN[key], (rec["loops"], LOOPS_SEEN[key])


def _describe(t, rec, row):
    q = int(t["pairs"][row])
    return ("pair %s (%s folds, degree %d, clamp-free %d, kappa_max %.4f)"
            % (tuple(int(v) for v in t["ij"][row]), t["fold"][row], int(rec["degree"][q]), int(rec["free"][q]), float(rec["kmax"][q])))


def _check(label, got, t, rec, tol):
    """|got - (1 - cc)| over the listed pairs against the bar tol; printed with the worst pair and the worst per fold class."""
    d = CT.distance(got, t["value"])
    row = int(np.argmax(d))
    by_fold = {f: "%.3g" % d[t["fold"] == f].max() for f in FOLDS if (t["fold"] == f).any()}
    line = "%s: worst |got - (1 - cc)| %.3g (bar %.0e) at %s; by fold class %s" % (label, d.max(), tol, _describe(t, rec, row), by_fold)
    print(line)
    bad = np.flatnonzero(~(d <= tol))
    if len(bad):
        line += "; failing: " + ", ".join("%s %.3g" % (_describe(t, rec, r), d[r]) for r in bad[:16])
    return bool(len(bad) == 0), line


@pytest.mark.parametrize("key", sorted(CT.CASES))
def test_pair_values_against_the_direct_statement(gpu_ctx, oracle_mod, key):
    """One case of correlation_terms.CASES.  Measured on an MI355X (DESIGN.md 2 has every figure): POLYNOMIAL and PER_SAMPLE at
    most 7.6e-5 from the float32-position statement (case a2; bar 1e-3) and 3.6e-5 from the float64-position one, the reference
    arithmetic at most 1.24e-7 (case i; bar 1e-6), the means within 2.5e-6 relative (case e; bar 1e-5)."""
    import epipolarconsistency_amd as E
    name, n, n_alpha, n_t, radius, dkappa, kinds, setups, data = CT.CASES[key]
    Ps, n_u, n_v, host = CT.case_data(key)
    N = n * (n - 1) // 2
    failures = []
    try:
        for derivative in kinds:
            t = CT.case_terms(key, derivative)
            rows = t["pairs"]
            live = np.isfinite(t["value"])
            # the vacuity guard: away from cc = 1, where the comparison sees nothing
            assert 0.2 < np.median(t["value"][live]) < 1.8 and live.sum() >= 0.75 * len(live)
            oracle_mod.set_use_corr(1)
            try:
                c_oracle = oracle_mod.evaluate_all(Ps, host, n_u, n_v, object_radius_mm=radius, dkappa=dkappa,
                                                   is_derivative=derivative)["pairs"].astype(np.float64)
            finally:
                oracle_mod.set_use_corr(0)
            kw = {} if derivative else dict(filter=E.FILTER_NONE)
            dtrs = [E.RadonIntermediate.from_host(gpu_ctx, h, n_u, n_v, **kw) for h in host]
            pitch_class = _pitch_class(dtrs[0], n_alpha)
            rec = _records(gpu_ctx, Ps, dtrs, radius, dkappa, pitch_class)
            print("case %s: %s, %d views, %d x %d bins, radius %g, dkappa %g, derivative %s, %s: pitch class %d; classes %s; folds %s; "
                  "polynomial loops (PITCH4, NOCLAMP, DEG) %s" % (key, name, n, n_alpha, n_t, radius, dkappa, derivative, data, pitch_class,
                                                                   {k: rec[k] for k in COUNTS}, {f: int((t["fold"] == f).sum()) for f in FOLDS}, rec["loops"]))
            # the records are in the oracle's pair order and describe the oracle's ranges
            assert np.max(np.abs(rec["kmax"] - t["K01s"][:, 15])) <= 1e-3, np.max(np.abs(rec["kmax"] - t["K01s"][:, 15]))
            for sampling, quads in setups:
                tol = CT.tolerance(sampling, N)
                gpu_ctx.setQuadCopies(quads)
                m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling(sampling)
                m.setObjectRadius(radius)
                m.setEpipolarPlaneStep(dkappa)
                m.useCorrelation(True)
                quad_bytes = m.device_bytes()["quad_copies"]
                total, got = m.evaluate_range(0, N, want_pairs=True)
                m.close()
                _reached(key, sampling, quads, rec, t, N, pitch_class, quad_bytes)
                label = "case %s %s, quad copies %s, derivative %s" % (key, sampling, quads, derivative)
                ok, line = _check(label, got[rows], t, rec, tol)
                if not ok:
                    failures.append(line)
                # a pair without samples gives what the oracle gives (NaN: 0 / 0)
                dead = np.flatnonzero(~live)
                if len(dead) and not np.array_equal(got[rows][dead], c_oracle[rows][dead].astype(np.float32), equal_nan=True):
                    failures.append("%s: pairs without samples %s: got %s, the oracle %s" % (label, t["ij"][dead].tolist(), got[rows][dead], c_oracle[rows][dead]))
                # the mean, over all pairs: the statement's where it lists every pair, the C oracle's otherwise (case i)
                want_mean = t["mean"] if "mean" in t else c_oracle.sum() / N
                mean_err = abs(total / N - want_mean) / abs(want_mean)
                line = "%s: mean %.9g, statement %.9g: %.3g relative (bar %.0e)" % (label, total / N, want_mean, mean_err, T.TOL_MEAN)
                print(line)
                if not mean_err <= T.TOL_MEAN:
                    failures.append(line)
                if tol == T.TOL_THROUGHPUT:   # reported: the same against the float64-position statement and the C oracle
                    t64 = CT.case_terms(key, derivative, "float64")
                    print("%s: against float64 positions %.3g, against the C oracle %.3g" % (
                        label, CT.distance(got[rows], t64["value"]).max(), CT.distance(got, c_oracle).max()))
            for d in dtrs:
                d.close()
    finally:
        gpu_ctx.setQuadCopies("auto")
    assert not failures, "\n".join(failures)


def test_launch_forms_give_the_same_bits(gpu_ctx, oracle_mod):
    """Under CORR, on case b's scan in POLYNOMIAL mode: the cost image of evaluate(cost), evaluate_range, an index list of more
    than 4 096 tuples (the one-wave-per-pair kernel), lists of 1, 5 and 300 tuples (several waves per pair) and a metric with
    setSmallEval(True) give identical bits per pair -- the three moments are carried by every launch form.  The crossed tuple
    (i, j, di, dj), di != i: the geometry of pair (i, j) on the data of views di, dj, against the statement evaluated on those
    data, at the throughput bar."""
    import epipolarconsistency_amd as E
    key = "b"
    name, n, n_alpha, n_t, radius, dkappa = CT.CASES[key][:6]
    Ps, n_u, n_v, host = CT.case_data(key)
    t = CT.case_terms(key, True)
    N = n * (n - 1) // 2
    dtrs = [E.RadonIntermediate.from_host(gpu_ctx, h, n_u, n_v) for h in host]

    def metric(small):
        m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling("polynomial").setSmallEval(small)
        m.setObjectRadius(radius)
        m.setEpipolarPlaneStep(dkappa)
        return m.useCorrelation(True)
    m, m_small = metric(False), metric(True)
    total, base = m.evaluate_range(0, N, want_pairs=True)
    assert CT.distance(base, t["value"]).max() <= T.TOL_THROUGHPUT      # and they are the right numbers
    cost = np.zeros((n, n), np.float32)
    mean = m.evaluate(cost)
    ij = np.array([E.get_ij(q, n) for q in range(N)])
    assert np.array_equal(cost[ij[:, 1], ij[:, 0]], base) and abs(mean - total / N) <= 1e-12 * abs(mean)
    idx_all = np.concatenate([ij, ij], axis=1).astype(np.int32)
    order = np.tile(np.arange(N), 4096 // N + 2)
    assert len(order) > 4096
    out = np.empty(len(order), np.float32)
    m.evaluate(np.ascontiguousarray(idx_all[order]), out)
    assert np.array_equal(out, base[order])
    for L in (1, 5, 300):
        sel = order[7:7 + L]
        for which in (m, m_small):
            out = np.empty(L, np.float32)
            which.evaluate(np.ascontiguousarray(idx_all[sel]), out)
            assert np.array_equal(out, base[sel]), (L, which is m_small)
    total_small, vals_small = m_small.evaluate_range(0, N, want_pairs=True)
    assert total_small == total and np.array_equal(vals_small, base)
    # crossed tuples: the pairs with the largest ranges (hand-over into the exact tail) and the first few, on other views' data
    picks = sorted(set(np.argsort(-t["kmax"])[:4].tolist() + [0, 1, 2, 3]))
    crossed, want = [], []
    for q in picks:
        i, j = (int(v) for v in ij[q])
        di, dj = (i + 3) % n, (j + 5) % n
        crossed.append((i, j, di, dj))
        want.append(CT.pair_moments(t["K01s"][q], host[di], host[dj], n_u, n_v)["value"])
    out = np.empty(len(crossed), np.float32)
    m.evaluate(np.array(crossed, np.int32), out)
    d = CT.distance(out, np.array(want))
    apart = np.abs(np.array(want) - t["value"][picks]).min()
    print("crossed tuples %s: worst |got - (1 - cc)| %.3g; the statement on the views' own data is %.3g away at least" % (crossed, d.max(), apart))
    assert apart > 10 * T.TOL_THROUGHPUT     # the crossed data, not the views' own, decide the value: 0.029 at the closest tuple
    assert d.max() <= T.TOL_THROUGHPUT, (crossed, out, want)
    m.close()
    m_small.close()
    for dt in dtrs:
        dt.close()
