"""tests/weighted_robust_map_terms.py on the CPU: the per-bin comparison tests/test_gpu_weighted_robust_map.py uses, at its LOOSEST
bar (1e-3 of the bin scale, the throughput paths'), rejects every slip of weighted_robust_map_terms.SLIPS on at least two cases;
the float32- and float64-position statements agree far inside that bar; the statement conserves what it must; the weights rule;
and the reason the call exists -- a second pass improves on the first -- holds in the statement itself, before any GPU run
(DESIGN.md 4.25)."""
import numpy as np
import pytest

import channel_terms as T
import robust_map_terms as M
import weighted_robust_map_terms as WM
import weighted_robust_terms as WR
import weighted_terms as W
from test_robust_map_terms_oracle import GAIN, MIN_HITS, block_statement

SMALL = ("d", "e", "i", "j")
SETTINGS = (("truncated", "p90"), ("huber", "median"))


def test_the_comparison_rejects_every_slip(oracle_mod):
    """Per slip: the worst bin of HITS and of REJ against the unslipped statement, in bars of 1e-3 of the bin scale (the unweighted
    HITS over the bin's neighbourhood).  Every slip is rejected (more than one bar) on at least two cases; the figures are printed."""
    report = {}
    for slip in WM.SLIPS:
        rejected = {}
        for label in SMALL:
            loss, scale = SETTINGS[0]
            hits, rej = WM.case_map(label, loss, scale)
            s_hits, s_rej = WM.case_map(label, loss, scale, slip=slip)
            s = WM.case_scale(label, loss, scale)
            rejected[label] = max(M.compare(s_hits, hits, s, T.TOL_THROUGHPUT), M.compare(s_rej, rej, s, T.TOL_THROUGHPUT))
        report[slip] = rejected
        print("%-26s %s" % (slip, "  ".join("%s: %.3g bars" % kv for kv in sorted(rejected.items()))))
    for slip, rejected in report.items():
        assert sum(b > 1.0 for b in rejected.values()) >= 2, (slip, rejected)


@pytest.mark.parametrize("label", SMALL)
def test_float32_and_float64_positions_agree_inside_the_bar(oracle_mod, label):
    """The throughput paths' positions are neither statement's: the two statements must agree within 0.2 of the 1e-3 bar per bin."""
    for loss, scale in SETTINGS:
        h32, r32 = WM.case_map(label, loss, scale)
        h64, r64 = WM.case_map(label, loss, scale, "float64")
        s = WM.case_scale(label, loss, scale)
        a, b = M.compare(h64, h32, s, T.TOL_THROUGHPUT), M.compare(r64, r32, s, T.TOL_THROUGHPUT)
        print("case %s %s %s: float64 against float32 positions, HITS %.3g, REJ %.3g of the bar 1e-3" % (label, loss, scale, a, b))
        assert a <= 0.2 and b <= 0.2, (label, a, b)


@pytest.mark.parametrize("label", SMALL)
def test_the_statement_conserves_weight_mass_and_refusals(oracle_mod, label):
    """Per view: sum HITS == sum over its pairs of u 2 n_kappa; sum REJ == sum of (u - k) 2 n_kappa; 0 <= REJ <= HITS <= the
    unweighted HITS (weights in [0, 1])."""
    n = W.settings(label)[1]
    for loss, scale in SETTINGS:
        hits, rej = WM.case_map(label, loss, scale)
        mass, refused = WM.conserved(WR.case_terms(label, loss, scale), n)
        assert np.allclose(hits.sum(axis=(1, 2)), mass, rtol=1e-12)
        assert np.allclose(rej.sum(axis=(1, 2)), refused, rtol=1e-9, atol=1e-9)
        assert np.all(rej >= 0.0) and np.all(rej <= hits * (1 + 1e-12))
        assert np.all(hits <= M.case_map(label, loss, scale)[0] * (1 + 1e-12) + 1e-12)
        assert hits.sum() < M.case_map(label, loss, scale)[0].sum()        # the case's weights do remove mass


def test_map_weights_rule():
    rng = np.random.default_rng(5)
    h = rng.uniform(0, 8, (5, 7)).astype(np.float32)
    r = (h * rng.uniform(0, 1, h.shape)).astype(np.float32)
    w_old = rng.uniform(0, 1, h.shape).astype(np.float32)
    w_old[1, 1] = 0.0
    h[0, 0] = r[0, 0] = 0.0
    mu = WM.map_weights(w_old, h, r, 1.0, 1.0)
    assert mu.dtype == np.float32 and np.all(mu <= w_old) and np.all(mu >= 0) and mu[1, 1] == 0.0
    assert np.array_equal(mu[h < 1.0], w_old[h < 1.0])                      # too few hits: the old weight stays
    assert np.array_equal(WM.map_weights(w_old, h, np.zeros_like(h), 1.0, 2.5), w_old)      # nothing refused: W_old
    assert np.array_equal(WM.map_weights(np.ones_like(h), h, r, 4.0, 2.5), M.map_weights(h, r, 4.0, 2.5))   # W_old == 1: the n-metric's rule
    with np.errstate(invalid="ignore"):
        want = w_old * np.fmax(0.0, 1.0 - 2.5 * (r.astype(np.float64) / h)).astype(np.float32)    # W_old * factor, the product in float32
    assert want.dtype == np.float32 and np.array_equal(WM.map_weights(w_old, h, r, 4.0, 2.5)[h >= 4], want[h >= 4])


# ---- the reason the call exists, in the statement ------------------------------------------------------------------------------------
def test_a_second_pass_improves_on_the_first(oracle_mod, small_scan):
    """The fixture of tests/test_robust_map_terms_oracle.py::block_statement (the opaque block in view 6, truncated loss, delta of
    pass 1 held, min_hits 1, gain 1).  Pass 1: the n-metric's map and its weights mu1.  Pass 2: the map under mu1 at the same
    delta, mu2 = mu1 * factor.  corrupted / clean of the weighted metric under mu2 is below that under mu1.  Only the ordering is
    asserted; the figures are printed (a run: 74.94 after pass 1, 52.06 after pass 2)."""
    s = block_statement(oracle_mod, small_scan)
    n, Ps, bad, clean, K01s, delta = s["n"], s["Ps"], s["bad"], s["clean"], s["K01s"], s["delta"]
    Kc = oracle_mod.evaluate_all(Ps, clean, 128, 128, want_K01=True)["K01s"]

    def ratio(mu):
        return W.scan_terms(Ps, bad, mu, 128, 128, K01s)["value"] / W.scan_terms(Ps, clean, mu, 128, 128, Kc)["value"]
    mu1 = [M.map_weights(s["hits"][v], s["rej"][v], MIN_HITS, GAIN) for v in range(n)]
    first = ratio(mu1)
    smp = WR.scan_samples(Ps, bad, mu1, 128, 128, K01s)
    bins = mu1[0].shape[::-1]
    hits2, rej2 = WM.scan_map(smp, K01s, n, bins[0], bins[1], 128, 128, "truncated", delta)
    mu2 = [WM.map_weights(mu1[v], hits2[v], rej2[v], MIN_HITS, GAIN) for v in range(n)]
    second = ratio(mu2)
    share = rej2.sum(axis=(1, 2)) / hits2.sum(axis=(1, 2))
    print("delta %.6g; corrupted / clean of the weighted metric: %.4g under pass 1's weights, %.4g under pass 2's; pass 2's "
          "sum REJ / sum HITS per view: %s" % (delta, first, second, " ".join("%.4f" % v for v in share)))
    assert all(np.all(b <= a) for a, b in zip(mu1, mu2)) and any(np.any(b < a) for a, b in zip(mu1, mu2))
    assert second < first, (first, second)
