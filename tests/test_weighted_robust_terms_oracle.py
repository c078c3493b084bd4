"""The direct float64 statement of the weighted robust pair sums (tests/weighted_robust_terms.py) against weighted_terms' and
robust_terms' statements, and the cases of tests/test_gpu_weighted_robust.py against their own requirements (no GPU): an infinite
scale gives the weighted terms, weights of one give the robust terms, the cases exercise both mechanisms in the same pair, and the
comparison the GPU test makes rejects the slips it is there for."""
import numpy as np
import pytest

import channel_terms as T
import robust_terms as R
import weighted_terms as W
import weighted_robust_terms as WR


def test_module_states_the_slips_the_issue_names():
    for slip in ("w_of_weighted_residual", "k_without_mu", "r_without_mu", "inlier_mass_over_n_pairs", "value_over_kept", "wj_from_view_i"):
        assert slip in WR.SLIPS
    assert WR.CASES is W.CASES and WR.LOSSES == R.LOSSES and WR.SCALES == R.SCALES


@pytest.mark.parametrize("label", ["d", "e", "i", "j"])
def test_an_infinite_scale_is_the_weighted_statement(oracle_mod, label):
    """delta = inf, every loss, both position statements: c, u and s are weighted_terms.case_terms' to 1e-12, k == u exactly (w == 1),
    value and coverage are its value and coverage, inlier_mass == 1."""
    for positions in ("float32", "float64"):
        ref = W.case_terms(label, positions)
        smp = WR.case_samples(label, positions)
        assert np.array_equal(smp["pairs"], ref["pairs"])
        for loss in WR.LOSSES:
            t = WR.scan_terms(smp, loss, np.inf)
            for key in ("c", "u", "s"):
                assert np.all(np.abs(t[key] - ref[key]) <= 1e-12 * np.abs(ref[key])), (label, positions, loss, key)
            assert np.array_equal(t["k"], t["u"]) and np.array_equal(t["n_kappa"], ref["n_kappa"])
            if "value" in ref:
                assert abs(t["value"] - ref["value"]) <= 1e-12 * ref["value"] and abs(t["coverage"] - ref["coverage"]) <= 1e-12
                assert t["inlier_mass"] == 1.0


@pytest.mark.parametrize("label", ["d", "e", "i", "j"])
def test_weights_of_one_are_the_robust_statement(oracle_mod, label):
    """Every weight 1, every loss, both scales: {c, k, r} are robust_terms' {c, u, r} to 1e-12, u == 1, r's scale is r; value and
    inlier_mass are its value and inlier_mass, coverage == 1."""
    Ps, n_u, n_v, data, weights, K01s = W.case_inputs(label)
    ones = [np.ones_like(w) for w in weights]
    smp = WR.scan_samples(Ps, data, ones, n_u, n_v, K01s, pairs=T.case_pairs(W.CASES[label]), derivative=W.settings(label)[6])
    for scale in WR.SCALES:
        for loss in WR.LOSSES:
            ref = R.case_terms(label, loss, scale)
            t = WR.scan_terms(smp, loss, float(R.case_delta(label, scale)))
            for mine, theirs in (("c", "c"), ("k", "u"), ("r", "r"), ("s", "s"), ("raw", "r")):
                assert np.all(np.abs(t[mine] - ref[theirs]) <= 1e-12 * np.abs(ref[theirs])), (label, scale, loss, mine)
            assert np.all(t["u"] == 1.0)
            if "value" in ref:
                assert abs(t["value"] - ref["value"]) <= 1e-12 * ref["value"] and t["coverage"] == 1.0
                assert abs(t["inlier_mass"] - ref["inlier_mass"]) <= 1e-12


# the share of listed pairs that must exercise both mechanisms at once, per scale
BOTH_AT_LEAST = {"median": 0.85, "p90": 0.50}


@pytest.mark.parametrize("label", sorted(WR.CASES))
def test_cases_exercise_both_mechanisms_in_the_same_pair(oracle_mod, label):
    """Under Huber, the listed pairs with u < 1 - 1e-3 (weights at work) and 0 < k < u (1 - 1e-3) (the loss at work among the trusted
    lines): at least 85 % of the listed pairs at the median scale and 50 % at p90.  Cases e and j each hold one listed pair with
    sum mu = 0, whose row is {0, 0, 0, 0}; every other listed pair has samples and u > 0."""
    for scale in WR.SCALES:
        t = WR.case_terms(label, "huber", scale)
        both = (t["u"] < 1 - 1e-3) & (t["k"] > 0) & (t["k"] < t["u"] * (1 - 1e-3))
        share = both.sum() / len(both)
        print("case %s %-6s: %d of %d listed pairs exercise both (%.0f %%)" % (label, scale, both.sum(), len(both), 100 * share))
        assert share >= BOTH_AT_LEAST[scale], (label, scale, share)
        dead = t["u"] == 0
        assert dead.sum() == (1 if label in ("e", "j") else 0), (label, dead.sum())
        rows, _ = WR.columns(t)
        assert np.all(rows[dead] == 0.0) and np.all(t["n_kappa"][dead] > 0)
        assert np.all(t["k"] <= t["u"]) and np.all(t["r"] <= t["raw"] * (1 + 1e-12))


@pytest.mark.parametrize("label", ["a", "g"])
def test_the_comparison_rejects_the_slips(oracle_mod, label):
    """The GPU test's comparison (channel_terms.compare at the throughput bar, the loosest; scales s, 1, 1 and the raw mean; the three
    means at TOL_MEAN) fed with the oracle's own outputs, each slip of weighted_robust_terms.SLIPS applied: every one is rejected
    under every loss, in the columns (or means) it changes, and leaves the others exactly alone.  Nothing runs on a GPU."""
    tol = T.TOL_THROUGHPUT
    Ps, n_u, n_v, data, weights, K01s = W.case_inputs(label)
    smp = WR.case_samples(label)
    swapped = WR.scan_samples(Ps, data, weights, n_u, n_v, K01s, pairs=T.case_pairs(W.CASES[label]), derivative=W.settings(label)[6],
                              slip="wj_from_view_i")
    changes = {"w_of_weighted_residual": (0, 2), "k_without_mu": (2,), "r_without_mu": (3,), "wj_from_view_i": (0, 1, 2, 3)}
    mean_changes = {"inlier_mass_over_n_pairs": (2,), "value_over_kept": (0,)}
    for slip in WR.SLIPS:
        for loss in WR.LOSSES:
            folds, mean_folds = [], []
            for scale in WR.SCALES:
                ref = WR.case_terms(label, loss, scale)
                want, scales = WR.columns(ref)
                assert T.compare(want, want, scales, tol).max() == 0.0
                got_t = WR.scan_terms(swapped if slip == "wj_from_view_i" else smp, loss, float(R.case_delta(label, scale)), slip=slip)
                folds.append(T.compare(WR.columns(got_t)[0], want, scales, tol))
                mean_folds.append(np.abs(WR.means(got_t) - WR.means(ref)) / (T.TOL_MEAN * WR.means(ref)))
            folds, mean_folds = np.array(folds), np.array(mean_folds)
            print("case %s, %-26s %-13s rejected %.3g-fold in the columns, %.3g-fold in the means" % (label, slip, loss, folds.max(), mean_folds.max()))
            if slip in changes:
                for col in range(4):
                    if col in changes[slip]:
                        assert folds[:, col].max() > 1.0, (slip, loss, col, folds)
                    else:
                        assert folds[:, col].max() == 0.0, (slip, loss, col, folds)
            else:
                assert folds.max() == 0.0, (slip, loss, folds)
                for col in range(3):
                    if col in mean_changes[slip]:
                        assert mean_folds[:, col].max() > 1.0, (slip, loss, col, mean_folds)
                    else:
                        assert mean_folds[:, col].max() == 0.0, (slip, loss, col, mean_folds)


def test_scale_rule_in_numpy():
    """weighted_robust_scale: the median of sqrt(r / u) over rows with r > 0 and u > 0; with u == 1 it is robust_terms.robust_scale."""
    rng = np.random.default_rng(23)
    rows = rng.uniform(0.1, 5.0, (11, 4))
    rows[2, 3] = 0.0
    rows[5, 1] = 0.0
    live = np.delete(np.arange(11), [2, 5])
    assert WR.weighted_robust_scale(rows, 1.5) == 1.5 * np.median(np.sqrt(rows[live, 3] / rows[live, 1]))
    rows[:, 1] = 1.0
    assert WR.weighted_robust_scale(rows) == R.robust_scale(rows[:, 3])
    assert WR.weighted_robust_scale(np.zeros((3, 4))) == 0.0
