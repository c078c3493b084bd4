"""The cross terms of ecc_metric_evaluate_view_coefficients and ecc_metric_evaluate_gram -- the gradient columns h0[c], h1[c] and
the Gram entries g_cd -- against the direct float64 statement of tests/channel_terms.py, on the geometries, grids and channel
counts that select each kernel and loop (channel_terms.CASES; tests/test_channel_terms_oracle.py holds the statement itself to
the C oracle and shows that this comparison rejects a sign, channel, view or trip slip at least 100-fold).

Every column both calls return is compared: per pair the value, h0[c], h1[c] and every g_cd, each relative to its Cauchy-Schwarz
scale (s0 / s1 = sqrt(value w sum v_c^2), sg = sqrt(g_cc g_dd)); every gradient entry grad[c, i] relative to the sum of its terms'
scales; the means value and G.  Bars (the project's own): 1e-6 for the reference arithmetic ("reference", "auto" at
512 pairs or fewer), 1e-3 for POLYNOMIAL and PER_SAMPLE against the float32-position statement, 1e-5 on the means.  The older tests
(test_gpu_view_coefficients.py, test_gpu_gram.py) pin the value column and the Gram diagonal bit for bit but see the cross terms
only on the planar short scan, where the two fold signs of a pair are equal on every sample; `mirrored` has 46 of 120 pairs with
opposite folds on every sample and 9 mixed, so the relative-sign weight of coeff_loop_poly, the subtraction of coeff_loop_exact on
oppositely signed samples and sample_line_plain's sign in the reference kernels are executed under a checked gradient here.

Each case asserts from the records of a single-channel metric (debug_polynomials, debug_K01) and the oracle's fold counts that its
pairs reach what it is there for, and prints its class counts and the worst ratio per column (throughput cases: against the
float64-position statement as well)."""
import numpy as np
import pytest

import channel_terms as T

pytestmark = pytest.mark.gpu

KAPPA_FIT_MAX = float(np.float32(0.98))   # csrc/ecc_layout.h: ecc_kappa_fit


def _records(gpu_ctx, Ps, dtrs, radius, dkappa):
    """The pair records of a single-channel metric in POLYNOMIAL mode (tests/test_gpu_gram.py::_pair_classes, per pair)."""
    import epipolarconsistency_amd as E
    n = len(Ps)
    n_pairs = n * (n - 1) // 2
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs[:n]).setSampling("polynomial")
    m.setObjectRadius(radius)
    m.setEpipolarPlaneStep(dkappa)
    recs = m.debug_polynomials(0, n_pairs)
    K01 = m.debug_K01(0, n_pairs)
    m.close()
    ok = np.array([r["poly_ok"] for r in recs])
    free = np.array([r["clamp_free"] for r in recs])
    folds_differ = np.array([bool(r["fold"][0]) != bool(r["fold"][1]) for r in recs])
    kmax = K01[:, 15]
    live = kmax > 0
    return dict(ok=ok, free=free, folds_differ=folds_differ, kmax=kmax, dkappa=K01[:, 14], live=live,
                clamp_free=int((ok & free).sum()), clamped=int((ok & ~free).sum()), refused=int((~ok & live).sum()),
                partial=int((ok & (kmax > KAPPA_FIT_MAX)).sum()), above=int((kmax > np.pi / 4).sum()),
                below=int((live & (kmax <= np.pi / 4)).sum()), poly_opposite=int((ok & folds_differ).sum()),
                exact_tail_above=int((((~ok & live) | (ok & (kmax > KAPPA_FIT_MAX))) & (kmax > np.pi / 4)).sum()))


def _reached(key, sampling, rec, t, n_pairs):
    """What the case is there for, from the records and the oracle's fold counts (see channel_terms.CASES)."""
    opposite_samples = t["opposite"] > 0                       # pairs with oppositely signed samples (oracle, listed pairs)
    kmax = rec["kmax"][t["pairs"]]
    if key == "a":      # polynomial loops with rel_sign = +1
        assert rec["poly_opposite"] >= 10, rec["poly_opposite"]
    elif key == "b":    # the exact loop on opposite folds, with and without the pi/4 reduction
        assert (opposite_samples & (kmax > np.pi / 4)).sum() >= 1 and (opposite_samples & (kmax <= np.pi / 4)).sum() >= 1
    elif key == "c":    # the row-quad loop in the exact tails (kappa_max > pi/4, refused or partial fits), on opposite folds too
        assert rec["exact_tail_above"] >= 1 and (opposite_samples & (kmax > np.pi / 4)).sum() >= 1, rec["exact_tail_above"]
    elif key == "d":    # pairs_coeff_reference_kernel<4, 4>: "auto" at 512 pairs or fewer, four waves per pair
        assert n_pairs <= 512 and (t["fold"] == "opposite").sum() >= 5 and (t["fold"] == "mixed").sum() >= 1
    elif key == "e":    # more than 2 048 pairs: one wave per pair
        assert n_pairs > 2048 and (t["fold"] == "opposite").sum() >= 50 and (t["fold"] == "mixed").sum() >= 5
    elif key == "f":    # the main-path kernels at K = 4 in all four polynomial classes
        assert rec["clamp_free"] > 0 and rec["clamped"] > 0 and rec["refused"] > 0 and rec["partial"] > 0
    elif key == "g":
        if sampling == "polynomial":   # refused fits, ranges above pi/4, mixed folds
            assert rec["refused"] > 0 and rec["above"] > 0 and (t["fold"] == "mixed").sum() >= 5
        else:
            assert opposite_samples.sum() >= 1 and (opposite_samples & (kmax > np.pi / 4)).sum() >= 1
    elif key == "h":    # the wide-offset grid's polynomial loops
        assert rec["clamp_free"] + rec["clamped"] > 0
    elif key == "i":    # DERIV = false on pairs whose folds differ: the sign must NOT be applied
        assert rec["poly_opposite"] >= 5 and (t["fold"] == "opposite").sum() >= 5
    else:               # j: the caller's kappa step reached the records
        assert np.all(rec["dkappa"][rec["live"]] == np.float32(0.004)) and rec["clamp_free"] + rec["clamped"] > 0


def _pair(t, row):
    return tuple(int(v) for v in t["ij"][row])


def _worst(label, got, want, scales, tol, t, names):
    """compare() per column, printed with the pair of the worst column and, per fold class, the worst ratio; a failure names them."""
    ratio = T.compare(got, want, scales, tol)
    with np.errstate(divide="ignore", invalid="ignore"):
        per = np.where(scales > 0, np.abs(np.asarray(got, np.float64) - want) / (tol * scales), 0.0)
    col = int(np.argmax(ratio))
    row = int(np.argmax(per[:, col]))
    by_fold = {f: float(per[t["fold"] == f].max()) for f in ("same", "opposite", "mixed") if (t["fold"] == f).any()}
    line = ("%s: worst %.3g of the bar %.0e (%.3g of the scale) in column %s, pair %s (%s folds); by fold class %s"
            % (label, ratio.max(), tol, ratio.max() * tol, names[col], _pair(t, row), t["fold"][row],
               {f: "%.3g" % v for f, v in by_fold.items()}))
    print(line)
    bad = np.argwhere(per > 1.0)
    if len(bad):
        line += "; failing (pair, column, fold): " + ", ".join("%s %s %s" % (_pair(t, r), names[c], t["fold"][r]) for r, c in bad[:24])
    return float(ratio.max()), line


@pytest.mark.parametrize("key", sorted(T.CASES))
def test_every_column_against_the_direct_oracle(gpu_ctx, oracle_mod, key):
    """One case of channel_terms.CASES (a .. j; j1 / j2: one and two channels).  The worst ratios of a GPU run are recorded in DESIGN.md 4.13 (none measured yet: written without a GPU; the
    class assertions of cases a, f, g, h and i depend on the fit's verdicts and are unconfirmed until the first run)."""
    import epipolarconsistency_amd as E
    name, n, n_alpha, n_t, K, radius, dkappa, derivative, setups = T.CASES[key]
    Ps, n_u, n_v, host, a = T.case_data(key)
    t = T.case_terms(key)
    N = n * (n - 1) // 2
    rows = t["pairs"]
    want_c, scale_c = T.coefficient_columns(t)
    want_g, scale_g = T.gram_columns(t)
    names_c = ["value"] + ["h0[%d]" % c for c in range(K)] + ["h1[%d]" % c for c in range(K)]
    names_g = ["g_%d%d" % (c, d) for c in range(K) for d in range(c, K)]
    kw = {} if derivative else dict(filter=E.FILTER_NONE)
    failures = []
    gpu_ctx.setQuadCopies(setups[0][1])
    try:
        dtrs = [E.RadonIntermediate.from_host(gpu_ctx, h, n_u, n_v, **kw) for h in host]
        rec = _records(gpu_ctx, Ps, dtrs, radius, dkappa)
        print("case %s: %s, %d views, %d x %d bins, K = %d, radius %g, dkappa %g, derivative %s: classes %s; folds %s" % (
            key, name, n, n_alpha, n_t, K, radius, dkappa, derivative,
            {k: rec[k] for k in ("clamp_free", "clamped", "refused", "partial", "above", "below", "poly_opposite", "exact_tail_above")},
            {f: int((t["fold"] == f).sum()) for f in ("same", "opposite", "mixed")}))
        # the records are in the oracle's pair order and describe the oracle's ranges
        assert np.max(np.abs(rec["kmax"] - t["K01s"][:, 15])) <= 1e-3, np.max(np.abs(rec["kmax"] - t["K01s"][:, 15]))
        for sampling, _ in setups:
            _reached(key, sampling, rec, t, N)
            tol = T.tolerance(sampling, N)
            m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling(sampling)
            m.setObjectRadius(radius)
            m.setEpipolarPlaneStep(dkappa)
            value, grad, pairs = m.evaluate_view_coefficients(a.astype(np.float32), want_pairs=True)
            G, gpairs = m.evaluate_gram(K, want_pairs=True) if K >= 2 else (None, None)
            m.close()
            assert np.array_equal(a.astype(np.float32).astype(np.float64), a)   # the coefficients are exactly what the oracle used
            label = "case %s %s" % (key, sampling)
            checks = [_worst(label + ", pair columns", pairs[rows], want_c, scale_c, tol, t, names_c)]
            done = t["complete"]
            checks.append(_worst(label + ", gradient entries", grad[:, done].T, t["grad"][:, done].T, t["grad_scale"][:, done].T, tol,
                                 dict(ij=[(i, i) for i in np.flatnonzero(done)], fold=np.array(["-"] * int(done.sum()))),
                                 ["grad[%d]" % c for c in range(K)]))
            if K >= 2:
                checks.append(_worst(label + ", Gram pair entries", gpairs[rows], want_g, scale_g, tol, t, names_g))
            if "mean" in t:   # every pair listed: the means
                mean_err = abs(value - t["mean"]) / (T.TOL_MEAN * t["mean"])
                line = "%s, value: %.3g of the bar 1e-05" % (label, mean_err)
                if K >= 2:
                    Gd = np.sqrt(np.outer(np.diag(t["G"]), np.diag(t["G"])))
                    G_err = float((np.abs(G - t["G"]) / (T.TOL_MEAN * Gd)).max())
                    line += "; G: %.3g of the bar" % G_err
                    mean_err = max(mean_err, G_err)
                print(line)
                checks.append((mean_err, line))
            if tol == T.TOL_THROUGHPUT:   # reported: the same against the float64-position statement
                t64 = T.case_terms(key, "float64")
                c64, _ = T.coefficient_columns(t64)
                print("%s, against float64 positions: pair columns %.3g of the bar, gradient entries %.3g" % (
                    label, T.compare(pairs[rows], c64, scale_c, tol).max(),
                    T.compare(grad.reshape(-1), t64["grad"].reshape(-1), t["grad_scale"].reshape(-1), tol)))
            assert np.all(np.isfinite(grad)) and np.isfinite(value)
            failures += [line for worst, line in checks if not worst <= 1.0]
    finally:
        gpu_ctx.setQuadCopies("auto")
    for d in dtrs:
        d.close()
    assert not failures, "\n".join(failures)
