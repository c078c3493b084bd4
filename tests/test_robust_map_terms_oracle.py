"""tests/robust_map_terms.py on the CPU: the per-bin comparison tests/test_gpu_robust_map.py uses, at its LOOSEST bar (1e-3 of the
bin scale, the throughput paths'), rejects every slip of robust_map_terms.SLIPS on at least two cases; the float32- and
float64-position statements agree far inside that bar; the statement conserves what it must; and the reason the call exists holds
in the statement itself, before any GPU run."""
import numpy as np
import pytest

import channel_terms as T
import robust_map_terms as M
import robust_terms as R
import weighted_terms as W

SMALL = ("d", "e", "i", "j")          # the cases with small grids: every slip is a property of the deposit rule, not of the grid
SETTINGS = (("truncated", "p90"), ("huber", "median"))


def test_the_comparison_rejects_every_slip(oracle_mod):
    """Per slip: the worst bin of HITS and of REJ against the unslipped statement, in bars of 1e-3 of the bin scale.  Every slip is
    rejected (more than one bar) on at least two cases; the figures are printed."""
    report = {}
    for slip in M.SLIPS:
        rejected = {}
        for label in SMALL:
            loss, scale = SETTINGS[0]
            hits, rej = M.case_map(label, loss, scale)
            s_hits, s_rej = M.case_map(label, loss, scale, slip=slip)
            bars = max(M.compare(s_hits, hits, M.bin_scale(hits), T.TOL_THROUGHPUT), M.compare(s_rej, rej, M.bin_scale(hits), T.TOL_THROUGHPUT))
            rejected[label] = bars
        report[slip] = rejected
        print("%-26s %s" % (slip, "  ".join("%s: %.3g bars" % kv for kv in sorted(rejected.items()))))
    for slip, rejected in report.items():
        assert sum(b > 1.0 for b in rejected.values()) >= 2, (slip, rejected)


@pytest.mark.parametrize("label", SMALL)
def test_float32_and_float64_positions_agree_inside_the_bar(oracle_mod, label):
    """The throughput paths' positions are neither statement's: the two statements must agree far inside the 1e-3 bar per bin."""
    for loss, scale in SETTINGS:
        h32, r32 = M.case_map(label, loss, scale)
        h64, r64 = M.case_map(label, loss, scale, "float64")
        s = M.bin_scale(h32)
        a, b = M.compare(h64, h32, s, T.TOL_THROUGHPUT), M.compare(r64, r32, s, T.TOL_THROUGHPUT)
        print("case %s %s %s: float64 against float32 positions, HITS %.3g, REJ %.3g of the bar 1e-3" % (label, loss, scale, a, b))
        assert a <= 0.2 and b <= 0.2, (label, a, b)


@pytest.mark.parametrize("label", SMALL)
def test_the_statement_conserves_samples_and_rejections(oracle_mod, label):
    """Per view: sum HITS == the samples taken in the view; sum REJ == sum over its pairs of (1 - u) 2 n_kappa; 0 <= REJ <= HITS."""
    n = W.settings(label)[1]
    res = R.case_residuals(label)
    for loss, scale in SETTINGS:
        hits, rej = M.case_map(label, loss, scale)
        t = R.case_terms(label, loss, scale)
        want_rej = np.zeros(n)
        for r in range(len(t["pairs"])):
            i, j = t["ij"][r]
            want_rej[[i, j]] += (1.0 - t["u"][r]) * 2 * t["n_kappa"][r]
        assert np.allclose(hits.sum(axis=(1, 2)), M.sample_counts(res, n), rtol=1e-12)
        assert np.allclose(rej.sum(axis=(1, 2)), want_rej, rtol=1e-9, atol=1e-9)
        assert np.all(rej >= 0.0) and np.all(rej <= hits * (1 + 1e-12))


def test_map_weights_rule():
    rng = np.random.default_rng(3)
    h = rng.uniform(0, 8, (5, 7)).astype(np.float32)
    r = (h * rng.uniform(0, 1, h.shape)).astype(np.float32)
    h[0, 0] = r[0, 0] = 0.0
    mu = M.map_weights(h, r, 1.0, 1.0)
    assert mu.dtype == np.float32 and np.all(mu[h < 1.0] == 1.0) and np.all((mu >= 0) & (mu <= 1))
    assert np.all(M.map_weights(h, np.zeros_like(h), 0.0, 2.5)[h > 0] == 1.0)
    assert M.map_weights(h, r, 0.0, 1.0)[0, 0] == 0.0       # 0 / 0 under min_hits == 0: fmax(0, nan) = 0
    assert np.all(M.map_weights(h, r, 4.0, 2.5)[h >= 4] == np.fmax(0.0, 1.0 - 2.5 * (r[h >= 4].astype(np.float64) / h[h >= 4])).astype(np.float32))


# ---- the reason the call exists, in the statement ------------------------------------------------------------------------------------
BAD_VIEW, BINS, GAIN, MIN_HITS = 6, 96, 1.0, 1.0
BLOCK = (slice(50, 62), slice(58, 68))   # the opaque block of tests/test_gpu_weighted.py


def block_statement(oracle_mod, small_scan, positions="float32"):
    """The fixture of tests/test_gpu_robust_map.py's test 7 in the statement: the spheres with the opaque block in view 6, the
    truncated loss at delta = robust_scale(rows at delta = inf, 0.5).  Returns a dict."""
    imgs, Ps = small_scan["imgs"], small_scan["Ps"]
    n = len(Ps)
    bad = np.array(imgs, np.float32)
    bad[BAD_VIEW][BLOCK] += 4.0 * float(np.max(imgs[BAD_VIEW]))
    clean_d = small_scan["dtrs"]
    bad_d = list(clean_d)
    bad_d[BAD_VIEW] = oracle_mod.radon(bad[BAD_VIEW], BINS, BINS)
    K01s = oracle_mod.evaluate_all(Ps, bad_d, 128, 128, want_K01=True)["K01s"]
    res = R.scan_residuals(Ps, bad_d, 128, 128, K01s, positions=positions)
    delta = R.robust_scale(R.scan_terms(res, "truncated", np.inf)["r"], 0.5)
    hits, rej = M.scan_map(res, K01s, n, BINS, BINS, 128, 128, "truncated", delta, positions)
    return dict(Ps=Ps, clean=clean_d, bad=bad_d, K01s=K01s, res=res, delta=delta, hits=hits, rej=rej, n=n)


def block_footprint(oracle_mod, shape):
    """The bins of view 6 whose lines cross the block: where the Radon transform of the block's indicator is positive."""
    flag = np.zeros(shape, np.float32)
    flag[BLOCK] = 1.0
    return oracle_mod.radon(flag, BINS, BINS, filter=2) > 0.0   # FILTER_NONE: line lengths


def test_the_reason_holds_in_the_statement(oracle_mod, small_scan):
    """(a) the view with the largest sum REJ / sum HITS is view 6; (b) in view 6 the bins whose lines cross the block hold a larger
    share of sum REJ than of sum HITS; (c) with mu = map_weights on all 8 views, the weighted metric's corrupted / clean is below
    the plain metric's."""
    s = block_statement(oracle_mod, small_scan)
    hits, rej, n = s["hits"], s["rej"], s["n"]
    share = rej.sum(axis=(1, 2)) / hits.sum(axis=(1, 2))
    print("delta %.6g; sum REJ / sum HITS per view: %s" % (s["delta"], " ".join("%.4f" % v for v in share)))
    assert int(np.argmax(share)) == BAD_VIEW, share
    cross = block_footprint(oracle_mod, s["Ps"] is not None and small_scan["imgs"][0].shape)
    rej_share, hit_share = rej[BAD_VIEW][cross].sum() / rej[BAD_VIEW].sum(), hits[BAD_VIEW][cross].sum() / hits[BAD_VIEW].sum()
    print("view 6, bins crossing the block: %.4f of sum REJ, %.4f of sum HITS" % (rej_share, hit_share))
    assert rej_share > hit_share, (rej_share, hit_share)
    mu = [M.map_weights(hits[v], rej[v], MIN_HITS, GAIN) for v in range(n)]
    Kc = oracle_mod.evaluate_all(s["Ps"], s["clean"], 128, 128, want_K01=True)["K01s"]
    w_bad = W.scan_terms(s["Ps"], s["bad"], mu, 128, 128, s["K01s"])["value"]
    w_clean = W.scan_terms(s["Ps"], s["clean"], mu, 128, 128, Kc)["value"]
    ones = [np.ones_like(m) for m in mu]
    p_bad = W.scan_terms(s["Ps"], s["bad"], ones, 128, 128, s["K01s"])["value"]
    p_clean = W.scan_terms(s["Ps"], s["clean"], ones, 128, 128, Kc)["value"]
    print("corrupted / clean: plain %.4g, weighted by the map (min_hits %g, gain %g) %.4g" % (p_bad / p_clean, MIN_HITS, GAIN, w_bad / w_clean))
    assert w_bad / w_clean < p_bad / p_clean
