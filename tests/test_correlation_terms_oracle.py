"""The direct float64 statement of the correlation form (tests/correlation_terms.py) against the C oracle, and the cases of
tests/test_gpu_correlation.py against their own requirements (no GPU).

The GPU test compares every pair value of useCorrelation(True) with correlation_terms.scan_moments; this file holds that helper to
oracle.evaluate_all under set_use_corr(1), measures how far its float32- and float64-position forms are apart, and shows that the
comparison the GPU test makes rejects the slips it is there for -- on every case, with the case's own data."""
import numpy as np
import pytest

import channel_terms as T
import correlation_terms as CT
import geometry_catalog

KEYS = sorted(CT.CASES)


def _corr_oracle(oracle_mod, *args, **kw):
    oracle_mod.set_use_corr(1)
    try:
        return oracle_mod.evaluate_all(*args, **kw)
    finally:
        oracle_mod.set_use_corr(0)


def _case_bar(key):
    """The loosest per-pair bar of the case's samplings: what a slip has to exceed."""
    n = CT.CASES[key][1]
    return max(CT.tolerance(s, n * (n - 1) // 2) for s, _ in CT.CASES[key][7])


def _fold_counts(t):
    return {k: int((t["fold"] == k).sum()) for k in ("same", "opposite", "mixed", "dead")}


TIE = [("mirrored", 8, 96, 64, 0.0), ("mirrored", 16, 768, 768, 0.0), ("near_opposite", 16, 768, 768, 185.0),
       ("scattered", 12, 1000, 767, 0.0)]


@pytest.mark.parametrize("name,n,n_alpha,n_t,radius", TIE)
def test_values_are_the_c_oracles(oracle_mod, name, n, n_alpha, n_t, radius):
    """The float32-position statement's 1 - cc is oracle.evaluate_all's pair value under set_use_corr(1) to 2e-7 absolute -- the
    float rounding of a stored value near 1, taken twice (the moments rounded to float, the stored 1 - cc), the bar of
    tests/test_channel_terms_oracle.py::test_values_are_the_c_oracles -- on white noise (default_rng(5)), derivative and plain
    data, the automatic step and dkappa = 0.004.  Measured, worst of the four settings: 1.08e-7 (mirrored 8, 96 x 64), 1.41e-7
    (mirrored 16, 768 x 768), 9.6e-8 (near_opposite 16, 768 x 768, 185 mm), 9.5e-8 (scattered 12, 1000 x 767)."""
    Ps, n_u, n_v = geometry_catalog.make(name, n)
    rng = np.random.default_rng(5)
    host = [rng.standard_normal((n_t, n_alpha), dtype=np.float32) for _ in range(n)]
    for derivative in (True, False):
        for dkappa in (0.0, 0.004):
            r = _corr_oracle(oracle_mod, Ps, host, n_u, n_v, object_radius_mm=radius, dkappa=dkappa, is_derivative=derivative,
                             want_K01=True)
            t = CT.scan_moments(Ps, host, n_u, n_v, derivative=derivative, K01s=r["K01s"])
            d = CT.distance(t["value"], r["pairs"].astype(np.float64))
            live = np.isfinite(t["value"])
            print("%s %d, %d x %d, radius %g, dkappa %g, derivative %s: worst |statement - oracle| %.3g, %d live pairs of %d"
                  % (name, n, n_alpha, n_t, radius, dkappa, derivative, d.max(), live.sum(), len(live)))
            assert d.max() <= 2e-7 and live.sum() >= 0.8 * len(live), (dkappa, derivative, d.max())


@pytest.mark.parametrize("key", KEYS)
def test_float32_against_float64_positions_and_the_oracle_per_case(oracle_mod, key):
    """The throughput paths' positions are neither the float32 nor the binary64 statement; the GPU test compares them with the
    float32 one at 1e-3.  The two statements themselves differ per pair by at most 1e-4, a tenth of that bar, on every case: the
    bar has at least 10 x room over the reference's own position noise.  Measured: a / c2 3.8e-5, a2 4.8e-5, b / c 5.4e-5, d 4.8e-5,
    d2 7.1e-5, e 4.2e-5, e2 2.8e-5, f 6.6e-6, g 3.5e-6, h 6.7e-6, i 2.4e-6.  The mean of the two statements differs by at most 2.2e-6 relative (a), but
    for case e's six pairs: 6.6e-6, two thirds of TOL_MEAN.
    With the case's own data (spikes, patches) the float32-position statement is again the C oracle's value to 2e-7; measured at
    most 1.5e-7 (b, c)."""
    name, n, n_alpha, n_t, radius, dkappa, kinds = CT.CASES[key][:7]
    Ps, n_u, n_v, host = CT.case_data(key)
    for derivative in kinds:
        t32, t64 = CT.case_terms(key, derivative, "float32"), CT.case_terms(key, derivative, "float64")
        floor = CT.distance(t64["value"], t32["value"]).max()
        r = _corr_oracle(oracle_mod, Ps, host, n_u, n_v, object_radius_mm=radius, dkappa=dkappa, is_derivative=derivative)
        tie = CT.distance(t32["value"], r["pairs"][t32["pairs"]].astype(np.float64)).max()
        line = "case %s, derivative %s: float32 against float64 positions %.3g; against the C oracle %.3g" % (key, derivative, floor, tie)
        if "mean" in t32:
            line += "; the means differ by %.3g relative" % (abs(t32["mean"] - t64["mean"]) / abs(t32["mean"]))
        print(line)
        assert floor <= 0.1 * T.TOL_THROUGHPUT and tie <= 2e-7, line


@pytest.mark.parametrize("key", KEYS)
def test_cases_have_their_fold_mix_and_are_not_vacuous(oracle_mod, key):
    """Every case has the fold mix it is there for (counts of pairs whose two fold signs are equal on every sample, opposite on
    every sample, both), the ranges it is there for, and is away from cc = 1, where the comparison sees nothing: the median of
    1 - cc lies in (0.2, 1.8) and at least three quarters of the pairs are live.  Kept as a record: if the catalog or the data
    change, this fails before the GPU cases lose their reason.
    Counts (same / opposite / mixed; pairs above 0.98 / above pi/4): a, c2 65 / 46 / 9, 5 / 8; a2 72 / 48 / 0, none; b, c 120 / 0 / 0,
    24 / 24; d 93 / 4 / 23, 4 / 23; d2 112 / 4 / 4, none; e 6 / 0 / 0, 0 / 1; e2 6 / 0 / 0, none; f 38 / 26 / 2, 1 / 1; g 15 / 11 / 2, 1 / 2; h 453 / 286 / 41, 32 / 43; i (484 of
    2 145 pairs) 272 / 173 / 39, 26 / 36."""
    for derivative in CT.CASES[key][6]:
        t = CT.case_terms(key, derivative)
        c = _fold_counts(t)
        live = np.isfinite(t["value"])
        tail, above = int((t["kmax"] > CT.KAPPA_FIT_MAX).sum()), int((t["kmax"] > np.pi / 4).sum())
        median = float(np.median(t["value"][live]))
        print("case %s, derivative %s: folds %s; kappa_max > 0.98 on %d pairs, > pi/4 on %d; median 1 - cc %.3f (%.3f .. %.3f), %d live of %d"
              % (key, derivative, c, tail, above, median, t["value"][live].min(), t["value"][live].max(), live.sum(), len(live)))
        assert 0.2 < median < 1.8 and live.sum() >= 0.75 * len(live) and c["dead"] == len(live) - live.sum()
        if key in ("a", "c2"):       # signed samples on opposite and mixed folds at pitch 6400
            assert c["opposite"] >= 30 and c["mixed"] >= 5 and tail >= 3
        elif key == "a2":            # the same scan with short ranges (low degrees)
            assert c["opposite"] >= 30 and t["kmax"].max() < 0.25
        elif key in ("b", "c"):      # every fit class of the flat scan and many exact tails; no pair whose folds differ
            assert c["same"] == len(live) and tail >= 10 and above >= 10
        elif key == "d":             # generic pitch: mixed folds, ranges above pi/4, exact tails
            assert c["mixed"] >= 10 and above >= 10 and tail >= 3
        elif key == "d2":            # generic pitch with short ranges
            assert c["mixed"] + c["opposite"] >= 5 and t["kmax"].max() < 0.25
        elif key in ("e", "e2"):     # wide offsets (six pairs)
            assert c["same"] == 6
        elif key == "f":             # the caller's step; generic pitch on pairs whose folds differ
            assert c["opposite"] >= 10 and tail >= 1 and np.all(t["K01s"][live, 14] == np.float32(0.004))
        elif key == "g":
            assert len(live) == 28 and c["opposite"] >= 5 and c["mixed"] >= 1
        elif key == "h":
            assert 512 < len(live) <= 2048 and c["opposite"] >= 100 and c["mixed"] >= 10
        else:
            assert key == "i" and t["n_pairs"] > 2048 and c["opposite"] >= 50 and c["mixed"] >= 5 and len(live) >= 0.15 * t["n_pairs"]


@pytest.mark.parametrize("key", KEYS)
def test_the_comparison_rejects_the_slips(oracle_mod, key):
    """The GPU test's comparison (|got - (1 - cc)| against the case's loosest bar) fed with the statement's own output under each
    slip, on the case's own scan and data, at the worst pair: the weight dropped, the fold sign of view j not applied (derivative
    data) or the signs applied (plain data), view j's data taken from another view -- each rejected at least 100-fold; the last
    64-sample trip dropped (pairs of more than 64 samples) and the whole exact tail dropped (pairs with kappa_max > 0.98) -- at
    least 20-fold.  Nothing runs on a GPU.  Measured against the 1e-3 bar (weight / sign / other view / trip / tail):
        a 491 / 817 / 799 / 56 / 130      a2 763 / 1 068 / 1 371 / 32 / none    b 611 / 661 / 561 / 31 / 40
        c 611 / -- / 561 / 31 / 40        c2 491 / 997 / 799 / 56 / 131         d 367 / 476 / 474 / 86 / 41
        d2 639 / 682 / 1 029 / 90 / none  e 199 / 232 / 338 / 95 / none         e2 252 / 136 / 516 / 81 / none
        f 763 / 862 (plain: 1 173) / 1 213 / 625 / 177 (one pair)              (none: no pair with kappa_max > 0.98)
    and against the 1e-6 bar of g, h and i at least 18 000-fold.
    The agreement of the weight's constant factor between the polynomial part and the exact tail of one pair (all of the factor
    that cc can show) is a far smaller signal than a dropped tail: a tail weighted 1 / kappa instead of kappa_max / kappa moves the
    worst pair of b and c by 5.3 bars (asserted at 5), of a and c2 by 9.7, of d by 5.3, of f by 21 -- if that pair's fit is a
    partial one on the GPU, which the CPU cannot know.  (A library built with that mistake moved case b by the same 5.4e-3 on an
    MI355X and failed b, c and f; the one partial pair of a and c2 moved by 0.8 bars and passed.)
    Gap: on case c (`near_opposite`, plain data) the two fold signs of a pair are equal on every sample, so signs applied to BOTH
    views cancel in xx, yy and xy alike: that slip moves nothing there (asserted: exactly 0) and is what case c2 is for; case c
    sees a sign on one view only, which is the slip "sign of view j not applied" with the roles of the data kinds exchanged."""
    name, n, n_alpha, n_t, radius, dkappa, kinds = CT.CASES[key][:7]
    Ps, n_u, n_v, host = CT.case_data(key)
    bar = _case_bar(key)
    for derivative in kinds:
        t = CT.case_terms(key, derivative)
        assert CT.distance(t["value"], t["value"]).max() == 0.0

        def rejected(label, factor, select=None, **kw):
            u = CT.scan_moments(Ps, host, n_u, n_v, pairs=CT.case_pairs(key), derivative=derivative, K01s=t["K01s"], **kw)
            d = CT.distance(u["value"], t["value"])
            d = d if select is None else d[select]
            worst = float(d.max()) / bar if len(d) else 0.0
            print("case %s, derivative %s: %-45s rejected %.4g-fold (bar %.0e, %d pairs)" % (key, derivative, label, worst, bar, len(d)))
            if factor is not None:
                assert worst >= factor, (key, label, worst)
            return worst

        rejected("weight dropped", 100.0, slip="no_weight")
        if derivative:
            rejected("fold sign of view j not applied", 100.0, slip="no_sign_j")
        elif key == "c":
            assert rejected("fold signs applied to plain data (equal folds)", None, slip="sign_on_plain") == 0.0
        else:
            rejected("fold signs applied to plain data", 100.0, slip="sign_on_plain")
        rejected("view j's data taken from another view", 100.0, other_view=True)
        long_enough = t["n_kappa"] > 64
        assert long_enough.sum() >= 5
        rejected("last 64-sample trip dropped", 20.0, select=long_enough, slip="skip_trip")
        tail = t["kmax"] > CT.KAPPA_FIT_MAX
        if key in ("a2", "d2", "e", "e2"):
            assert not tail.any()
        else:
            rejected("exact tail (kappa >= 0.98) dropped", 20.0, select=tail, slip="no_tail")
            # not one of the required slips -- the one thing of the weight's FACTOR that is observable: the tail takes 1 / kappa where
            # the polynomial part takes kappa_max / kappa (0.64 of it at kappa_max = pi/2).  Cases b and c are there for the
            # hand-over: asserted at what is reached there, printed elsewhere
            rejected("exact tail weighted by another constant factor", 5.0 if key in ("b", "c") else None, select=tail, slip="tail_factor")
