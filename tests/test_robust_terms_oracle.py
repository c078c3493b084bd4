"""The direct float64 statement of the robust pair sums (tests/robust_terms.py) against channel_terms' statement of the plain ones,
and the cases of tests/test_gpu_robust.py against their own requirements (no GPU): an infinite scale gives the plain value, both
scales of every case leave the share of samples outside delta they are built for, the float32- and float64-position statements agree
far inside the throughput bar, and the comparison the GPU tests make rejects the slips they are there for."""
import numpy as np
import pytest

import channel_terms as T
import robust_terms as R
import weighted_terms as W

THROUGHPUT = [k for k in sorted(R.CASES) if any(T.tolerance(s, W.settings(k)[1] * (W.settings(k)[1] - 1) // 2) == T.TOL_THROUGHPUT
                                                for s, _ in W.settings(k)[7])]


def test_the_weights_are_the_losses():
    """rho = w d^2 is the textbook loss: Huber d^2 | 2 delta |d| - delta^2, truncated min(d^2, delta^2), Geman-McClure
    d^2 delta^2 / (delta^2 + d^2); w == 1 at d = 0 and for every d at an infinite scale; w in (0, 1] and continuous at |d| = delta."""
    d = np.concatenate([[0.0], np.linspace(-9.0, 9.0, 1801)])
    a, delta = np.abs(d), 2.5
    want = {"huber": np.where(a <= delta, d * d, 2 * delta * a - delta * delta), "truncated": np.minimum(d * d, delta * delta),
            "geman_mcclure": d * d * delta * delta / (delta * delta + d * d)}
    for loss in R.LOSSES:
        w = R.loss_weight(a, loss, delta)
        assert np.all(w > 0) and np.all(w <= 1.0) and w[0] == 1.0
        assert np.max(np.abs(w * d * d - want[loss])) <= 1e-12
        assert np.all(R.loss_weight(a, loss, np.inf) == 1.0)
        edge = R.loss_weight(np.array([delta * (1 - 1e-9), delta, delta * (1 + 1e-9)]), loss, delta)
        assert np.max(np.abs(np.diff(edge))) <= 1e-8


@pytest.mark.parametrize("label", ["d", "i", "j"])
def test_an_infinite_scale_is_the_plain_value(oracle_mod, label):
    """delta = inf: c and s are channel_terms.pair_terms' value at one channel with coefficient 1, to 1e-12 of it, u == 1, and r is
    that value over w06 2 n_kappa."""
    Ps, n_u, n_v, data, _, K01s = W.case_inputs(label)
    n, derivative = len(Ps), W.settings(label)[6]
    for positions in ("float32", "float64"):
        res = R.scan_residuals(Ps, data, n_u, n_v, K01s, derivative=derivative, positions=positions)
        ref = T.scan_terms(Ps, data[:n], np.ones((1, n)), n_u, n_v, derivative=derivative, positions=positions, K01s=K01s)
        for loss in R.LOSSES:
            t = R.scan_terms(res, loss, np.inf)
            assert np.all(np.abs(t["c"] - ref["value"]) <= 1e-12 * ref["value"])
            assert np.all(np.abs(t["s"] - ref["value"]) <= 1e-12 * ref["value"])
            assert np.all(t["u"] == 1.0) and t["inlier_mass"] == 1.0 and np.all(t["outside"] == 0)
            live = t["n_kappa"] > 0
            assert np.all(np.abs(t["r"][live] * res["w06"][live] * 2 * t["n_kappa"][live] - t["s"][live]) <= 1e-12 * t["s"][live])
            assert abs(t["value"] - ref["mean"]) <= 1e-12 * ref["mean"] and (t["c"] > 0).sum() >= 0.8 * len(t["c"])


@pytest.mark.parametrize("label", sorted(R.CASES))
def test_cases_are_sharp(oracle_mod, label):
    """Both scales of a case are float32 and leave the share of samples outside delta they are built for -- a half, a tenth, to one
    sample in a thousand -- so no case degenerates to all-inlier; and the loss matters: on the live pairs the medians of c / s and of
    u lie below 1 for every loss at either scale, with every u in (0, 1]."""
    res = R.case_residuals(label)
    total = sum(len(d) for d in res["d"])
    for scale in R.SCALES:
        delta = R.case_delta(label, scale)
        assert isinstance(delta, np.float32) and np.isfinite(delta) and delta > 0
        for loss in R.LOSSES:
            t = R.case_terms(label, loss, scale)
            share = t["outside"].sum() / total
            assert abs(share - R.OUTSIDE[scale]) <= 1e-3, (scale, share)
            live = t["s"] > 0
            ratio = t["c"][live] / t["s"][live]
            print("case %s %-13s %-6s delta %.6g: %d pairs, %d live; outside %.4f; c / s median %.3f (min %.3g, max %.3g); u in [%.3f, %.3f]" % (
                label, loss, scale, delta, len(live), live.sum(), share, np.median(ratio), ratio.min(), ratio.max(), t["u"].min(), t["u"].max()))
            assert live.sum() >= 0.8 * len(live)
            assert np.median(ratio) < 1.0 and ratio.max() <= 1.0 + 1e-12 and ratio.min() > 0.0
            assert t["u"].min() > 0.0 and t["u"].max() <= 1.0 and np.median(t["u"][live]) < 1.0


@pytest.mark.parametrize("label", THROUGHPUT)
def test_reference_alone_floor_of_the_throughput_cases(oracle_mod, label):
    """The float32- and float64-position statements differ per pair by at most 0.1 of the throughput bar, 1e-4 of the scale (s for c
    and r, 1 for u), for every loss at both scales.  (The weighted terms' 5e-5 would leave too little room: Huber tends to the plain
    sum as delta grows.)  Measured worst per case in DESIGN.md 4.19."""
    bar = 0.1 * T.TOL_THROUGHPUT
    worst_all = np.zeros(3)
    for scale in R.SCALES:
        for loss in R.LOSSES:
            c32, scales = R.columns(R.case_terms(label, loss, scale, "float32"))
            c64, _ = R.columns(R.case_terms(label, loss, scale, "float64"))
            worst = T.compare(c64, c32, scales, bar)
            print("case %s %-13s %-6s: float32 against float64 positions: c %.3g of the scale, u %.3g, r %.3g" % (
                label, loss, scale, worst[0] * bar, worst[1] * bar, worst[2] * bar))
            worst_all = np.maximum(worst_all, worst)
    assert worst_all.max() <= 1.0, worst_all


@pytest.mark.parametrize("label", ["a", "g"])
def test_the_comparison_rejects_the_slips(oracle_mod, label):
    """The GPU tests' comparison (channel_terms.compare at the throughput bar, the loosest; scale s for c and r, 1 for u) fed with the
    oracle's own outputs, each slip of robust_terms.SLIPS applied: every one is rejected under every loss it changes, at the scale
    where it shows most, by the printed factor; a loss it does not change keeps its columns.  Nothing runs on a GPU."""
    res = R.case_residuals(label)
    tol = T.TOL_THROUGHPUT
    for slip, losses in R.SLIPS.items():
        for loss in R.LOSSES:
            folds = []
            for scale in R.SCALES:
                want, scales = R.columns(R.case_terms(label, loss, scale))
                assert T.compare(want, want, scales, tol).max() == 0.0
                got, _ = R.columns(R.scan_terms(res, loss, float(R.case_delta(label, scale)), slip=slip))
                folds.append(T.compare(got, want, scales, tol))
            folds = np.array(folds)
            if loss not in losses:
                assert folds.max() == 0.0, (slip, loss, folds)
                continue
            print("case %s, %-22s %-13s rejected %.3g-fold (median scale: c %.3g, u %.3g; p90: c %.3g, u %.3g)" % (
                label, slip, loss, folds.max(), folds[0, 0], folds[0, 1], folds[1, 0], folds[1, 1]))
            assert folds.max() > 1.0, (slip, loss, folds)
            assert np.all(folds[:, 2] == 0.0)            # r has no loss in it
            if slip == "u_counts_inliers":
                assert np.all(folds[:, 0] == 0.0)        # the value column is not touched by it
            else:
                assert folds[:, 0].max() > 1.0, (slip, loss, folds)
