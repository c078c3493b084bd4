"""The direct float64 statement of the variance form's pair sums (tests/variance_terms.py) against channel_terms' statement of the
unweighted ones, and the cases of tests/test_gpu_variance.py against their own requirements (no GPU): constant fields give the
unweighted value or a quarter of it, the float32- and float64-position statements agree far inside the throughput bar on these
variance fields, every case is sharp, the comparison the GPU tests make rejects the slips they are there for, and the statement
computes the demonstration of DESIGN.md 4.28."""
import numpy as np
import pytest

import channel_terms as T
import variance_terms as V

THROUGHPUT = [k for k in sorted(V.CASES) if any(T.tolerance(s, V.settings(k)[1] * (V.settings(k)[1] - 1) // 2) == T.TOL_THROUGHPUT
                                                for s, _ in V.settings(k)[7])]


def test_the_variance_fields_have_every_kind_of_block():
    """Per view 64 blocks of exactly 0.5, exactly 2.0 and 0.25 * 16^U(0, 1): all three kinds in every view of case a, every entry in
    [0.25, 4), and 0.5 <-> 2 steps between neighbouring blocks exist."""
    fields = V.variance_fields(16, 768, 768)
    assert len(fields) == 16
    steps = 0
    for f in fields:
        assert f.dtype == np.float32 and f.shape == (768, 768) and f.min() >= V.V_MIN and f.max() < 4.0
        blocks = f.reshape(8, 96, 8, 96)
        flat_half = (blocks == 0.5).all(axis=(1, 3))
        flat_two = (blocks == 2.0).all(axis=(1, 3))
        rough = ~flat_half & ~flat_two
        assert flat_half.any() and flat_two.any() and rough.any()
        assert np.all(blocks.transpose(0, 2, 1, 3)[rough].std(axis=(1, 2)) > 0.5)
        steps += int((np.abs(np.diff(f[48::96, :], axis=1)) == 1.5).sum())
    assert steps >= 16
    assert V.variance_fields(2, 64, 96)[1].shape == (64, 96) and V.variance_fields(1, 767, 1000)[0].shape == (767, 1000)
    assert V.omega_max(0.125) == 2.0 and V.omega_max(1.5) == 1.0 / 1.5


@pytest.mark.parametrize("label", ["d", "i", "j"])
def test_constant_fields(oracle_mod, label):
    """V == 0.5 (s == 1, omega == 1 with a floor <= 1): c is the unweighted statement's value exactly and u == 1.  V == 0 with floor
    4 (omega == 1/4): exactly a quarter of it, u == 1/4, and the same value."""
    Ps, n_u, n_v, data, _, K01s = V.case_inputs(label)
    n, derivative = len(Ps), V.settings(label)[6]
    half = [np.full_like(d, 0.5) for d in data]
    zero = [np.zeros_like(d) for d in data]
    for positions in ("float32", "float64"):
        ref = T.scan_terms(Ps, data, np.ones((1, n)), n_u, n_v, derivative=derivative, positions=positions, K01s=K01s)
        for floor in (0.25, 1.0):
            t = V.scan_terms(Ps, data, half, floor, n_u, n_v, K01s, derivative=derivative, positions=positions)
            assert np.all(np.abs(t["c"] - ref["value"]) <= 1e-12 * ref["value"]) and np.all(np.abs(t["s"] - ref["value"]) <= 1e-12 * ref["value"])
            assert np.all(t["u"] == 1.0) and t["mean_weight"] == 1.0
            assert abs(t["value"] - ref["mean"]) <= 1e-12 * ref["mean"] and (t["c"] > 0).sum() >= 0.8 * len(t["c"])
        q = V.scan_terms(Ps, data, zero, 4.0, n_u, n_v, K01s, derivative=derivative, positions=positions)
        assert np.all(np.abs(q["c"] - 0.25 * q["s"]) <= 1e-12 * q["s"]) and np.all(q["u"] == 0.25) and q["mean_weight"] == 0.25
        assert abs(q["value"] - ref["mean"]) <= 1e-12 * ref["mean"]


@pytest.mark.parametrize("label", THROUGHPUT)
def test_reference_alone_floor_of_the_throughput_cases(oracle_mod, label):
    """The float32- and float64-position statements differ per pair by at most 0.05 of the throughput bar, 5e-5 of the scale
    (s omega_max for c, omega_max for u), on these variance fields and at both floors -- the bar tests/test_weighted_terms_oracle.py
    holds the weight fields to."""
    bar = 0.05 * T.TOL_THROUGHPUT
    for floor in V.FLOORS:
        t32, t64 = V.case_terms(label, floor, "float32"), V.case_terms(label, floor, "float64")
        c32, scales = V.columns(t32)
        c64, _ = V.columns(t64)
        worst = T.compare(c64, c32, scales, bar)
        live = t32["c"] > 0
        rel = np.max(np.abs(t64["c"][live] - t32["c"][live]) / t32["c"][live])
        print("case %s floor %g: float32 against float64 positions: c %.3g of the scale (%.3g of c itself), u %.3g" % (
            label, floor, worst[0] * bar, rel, worst[1] * bar))
        assert worst.max() <= 1.0, (floor, worst)


@pytest.mark.parametrize("label", sorted(V.CASES))
def test_cases_are_sharp(oracle_mod, label):
    """The variances matter in every case and at both floors: on the live pairs the median of c / (s omega_max) lies in [0.05, 0.9]
    (a constant field at the bound: 1), no pair exceeds 1, and u lies in (0, omega_max]."""
    for floor in V.FLOORS:
        t = V.case_terms(label, floor)
        om = V.omega_max(floor)
        live = t["s"] > 0
        ratio = t["c"][live] / (t["s"][live] * om)
        print("case %s floor %g: %d pairs, %d live; c / (s omega_max) median %.3f (min %.3g, max %.3g); u / omega_max in [%.3f, %.3f]; folds %s" % (
            label, floor, len(live), live.sum(), np.median(ratio), ratio.min(), ratio.max(), t["u"].min() / om, t["u"].max() / om,
            {f: int((t["fold"] == f).sum()) for f in ("same", "opposite", "mixed", "dead")}))
        assert live.sum() >= 0.8 * len(live)
        assert 0.05 <= np.median(ratio) <= 0.9 and ratio.max() <= 1.0 + 1e-12
        assert t["u"][live].min() > 0.0 and t["u"][live].max() <= om * (1.0 + 1e-12)
    # the floor 1.5 is active on part of the samples, 0.125 on none: u is never larger under it, smaller in most pairs, and not by
    # a constant factor
    lo, hi = V.case_terms(label, V.FLOORS[0]), V.case_terms(label, V.FLOORS[1])
    live = lo["s"] > 0
    assert np.all(hi["u"][live] <= lo["u"][live]) and (hi["u"][live] < lo["u"][live]).mean() >= 0.5
    assert np.ptp(hi["u"][live] / lo["u"][live]) > 1e-3


@pytest.mark.parametrize("label", ["a", "g"])
def test_the_comparison_rejects_the_slips(oracle_mod, label):
    """The GPU tests' comparison (channel_terms.compare at the throughput bar, the loosest; scales s omega_max for c and omega_max for
    u) fed with the statement's own outputs of a case with mixed folds (`mirrored` at 16 views; `scattered` with a 450-mm object),
    each slip of variance_terms.SLIPS applied, at the floor the slip shows at: every one is rejected, by the printed factor (at least
    10 is asserted).  Nothing runs on a GPU."""
    Ps, n_u, n_v, data, variances, K01s = V.case_inputs(label)
    derivative = V.settings(label)[6]
    tol = T.TOL_THROUGHPUT
    for floor in V.FLOORS:
        t = V.case_terms(label, floor)
        want, scales = V.columns(t)
        assert T.compare(want, want, scales, tol).max() == 0.0
        assert (t["fold"] == "mixed").sum() >= 5 and derivative
        for slip in V.SLIPS:
            got, _ = V.columns(V.scan_terms(Ps, data, variances, floor, n_u, n_v, K01s, derivative=derivative, slip=slip))
            ratio = T.compare(got, want, scales, tol)
            print("case %s floor %-5g %-26s rejected %.3g-fold (c %.3g, u %.3g)" % (label, floor, slip, ratio.max(), ratio[0], ratio[1]))
            assert ratio.max() >= 10.0, (floor, slip, ratio)
            if slip == "mean_weight_over_n_kappa":
                assert ratio[0] == 0.0   # the value column is not touched by it
            else:
                assert ratio[0] >= 10.0, (floor, slip, ratio)


def test_the_demonstration(oracle_mod):
    """What the form buys, by the statement: the 8-view 128^2 sphere scan at 96^2 bins, Gaussian noise of 5 % of the
    view's maximum on the left half of view 3; V = the FILTER_NONE transform of the pixel variances, floor = 1e-3 x the median of
    V_3's positive entries.  evaluate() grows at least 2-fold (measured 6.50), the variance form's value stays within 5 % (measured
    0.8 %).  The input is deterministic; the margins are for a builder's choice of summation order only."""
    from conftest import make_small_scan
    Ps, imgs = make_small_scan()
    noisy, var = V.demo_images(imgs)
    B = V.DEMO_BINS
    clean_d = [oracle_mod.radon(im, B, B) for im in imgs]
    noisy_d = [d if k != V.DEMO_VIEW else oracle_mod.radon(noisy[k], B, B) for k, d in enumerate(clean_d)]
    fields = [oracle_mod.radon(v, B, B, filter=2) for v in var]
    import epipolarconsistency_amd as E
    assert E.FILTER_NONE == 2
    floor = V.demo_floor(fields)
    assert floor > 0 and all(not f.any() for k, f in enumerate(fields) if k != V.DEMO_VIEW)
    K = [oracle_mod.evaluate_all(Ps, d, 128, 128, want_K01=True)["K01s"] for d in (clean_d, noisy_d)]
    p0, p1, v0, v1 = V.demo_ratios(Ps, clean_d, noisy_d, fields, floor, 128, 128, K[0], K[1])
    print("evaluate() %.1f -> %.1f, a factor of %.3f; variance form %.1f -> %.1f, a factor of %.4f (floor %.4g)" % (
        p0, p1, p1 / p0, v0, v1, v1 / v0, floor))
    assert p1 / p0 >= 2.0, (p0, p1)
    assert abs(v1 / v0 - 1.0) <= 0.05, (v0, v1)
