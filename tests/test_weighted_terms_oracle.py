"""The direct float64 statement of the weighted pair sums (tests/weighted_terms.py) against channel_terms' statement of the
unweighted ones, and the cases of tests/test_gpu_weighted.py against their own requirements (no GPU): ones give the unweighted
value, an excluded view removes exactly its pairs, the float32- and float64-position statements agree far inside the throughput
bar on these weight fields, and the comparison the GPU tests make rejects the slips they are there for."""
import numpy as np
import pytest

import channel_terms as T
import weighted_terms as W

THROUGHPUT = [k for k in sorted(W.CASES) if any(T.tolerance(s, W.settings(k)[1] * (W.settings(k)[1] - 1) // 2) == T.TOL_THROUGHPUT
                                                for s, _ in W.settings(k)[7])]


def test_the_weight_fields_have_every_kind_of_block():
    """Per view 64 blocks of exactly 0, exactly 1 and U(0, 1): all three kinds in every view of case a, values in [0, 1], and 0 <-> 1
    edges between neighbouring blocks exist."""
    fields = W.weight_fields(16, 768, 768)
    assert len(fields) == 16
    edges = 0
    for f in fields:
        assert f.dtype == np.float32 and f.shape == (768, 768) and f.min() == 0.0 and f.max() == 1.0
        corners = f[::96, ::96]
        assert (corners == 0).any() and (corners == 1).any() and ((corners > 0) & (corners < 1)).any()
        edges += int((np.abs(np.diff(f[48::96, :], axis=1)) == 1).sum())
    assert edges >= 16
    assert W.weight_fields(2, 64, 96)[1].shape == (64, 96) and W.weight_fields(1, 767, 1000)[0].shape == (767, 1000)


@pytest.mark.parametrize("label", ["d", "i", "j"])
def test_ones_are_the_unweighted_value(oracle_mod, label):
    """All weights 1: c is channel_terms.pair_terms' value at one channel with coefficient 1, to 1e-12 of it, and u == 1."""
    Ps, n_u, n_v, data, _, K01s = W.case_inputs(label)
    n, derivative = len(Ps), W.settings(label)[6]
    ones = [np.ones_like(d) for d in data]
    for positions in ("float32", "float64"):
        t = W.scan_terms(Ps, data, ones, n_u, n_v, K01s, derivative=derivative, positions=positions)
        ref = T.scan_terms(Ps, data, np.ones((1, n)), n_u, n_v, derivative=derivative, positions=positions, K01s=K01s)
        assert np.all(np.abs(t["c"] - ref["value"]) <= 1e-12 * ref["value"])
        assert np.all(np.abs(t["s"] - ref["value"]) <= 1e-12 * ref["value"])
        assert np.all(t["u"] == 1.0) and t["coverage"] == 1.0
        assert abs(t["value"] - ref["mean"]) <= 1e-12 * ref["mean"] and (t["c"] > 0).sum() >= 0.8 * len(t["c"])


def test_an_excluded_view_removes_exactly_its_pairs(oracle_mod):
    """W_v = 0 for one view, 1 elsewhere: every pair with v has c = u = 0, every other pair is unchanged, and the value is the mean
    of the others."""
    label, v = "d", 3
    Ps, n_u, n_v, data, _, K01s = W.case_inputs(label)
    ones = [np.ones_like(d) for d in data]
    full = W.scan_terms(Ps, data, ones, n_u, n_v, K01s)
    ones[v] = np.zeros_like(data[v])
    t = W.scan_terms(Ps, data, ones, n_u, n_v, K01s)
    hit = (t["ij"] == v).any(axis=1)
    assert hit.sum() == len(Ps) - 1
    assert np.all(t["c"][hit] == 0.0) and np.all(t["u"][hit] == 0.0)
    assert np.array_equal(t["c"][~hit], full["c"][~hit]) and np.all(t["u"][~hit] == 1.0)
    assert abs(t["value"] - full["c"][~hit].mean()) <= 1e-12 * t["value"]
    assert t["coverage"] == (~hit).sum() / len(hit)


@pytest.mark.parametrize("label", THROUGHPUT)
def test_reference_alone_floor_of_the_throughput_cases(oracle_mod, label):
    """The float32- and float64-position statements differ per pair by at most 0.05 of the throughput bar, 5e-5 of the scale (s for c,
    1 for u), with these weight fields too -- the bar tests/test_channel_terms_oracle.py holds the data to.  Measured (c / u): 6.6e-6 /
    5.1e-7 on `mirrored` and 6.7e-6 / 7.0e-7 on `near_opposite` at 768 x 768, 9.9e-6 / 9.5e-7 on `scattered` at 1000 x 767, 7.2e-6 / 1.0e-6
    at 2621 x 768, at most 3.6e-6 / 6.1e-7 at 96 x 64."""
    t32, t64 = W.case_terms(label, "float32"), W.case_terms(label, "float64")
    bar = 0.05 * T.TOL_THROUGHPUT
    c32, scales = W.columns(t32)
    c64, _ = W.columns(t64)
    worst = T.compare(c64, c32, scales, bar)
    print("case %s: float32 against float64 positions: c %.3g of the scale, u %.3g" % (label, worst[0] * bar, worst[1] * bar))
    assert worst.max() <= 1.0, worst


@pytest.mark.parametrize("label", sorted(W.CASES))
def test_cases_are_sharp(oracle_mod, label):
    """The weights matter in every case: on the live pairs the medians of c / s and of u lie in [0.05, 0.6] (all ones: 1; the mean of a
    product of two independent weights of mean 1/2: 1/4), so neither column is a near-0 or a near-1 that its scale would hide."""
    t = W.case_terms(label)
    live = t["s"] > 0
    ratio = t["c"][live] / t["s"][live]
    print("case %s: %d pairs, %d live; c / s median %.3f (min %.3g, max %.3g); u in [%.3f, %.3f]; folds %s" % (
        label, len(live), live.sum(), np.median(ratio), ratio.min(), ratio.max(), t["u"].min(), t["u"].max(),
        {f: int((t["fold"] == f).sum()) for f in ("same", "opposite", "mixed", "dead")}))
    assert live.sum() >= 0.8 * len(live)
    assert 0.05 <= np.median(ratio) <= 0.6 and ratio.max() <= 1.0 + 1e-12
    assert 0.05 <= np.median(t["u"][live]) <= 0.6 and t["u"].min() >= 0.0 and t["u"].max() <= 1.0


@pytest.mark.parametrize("label", ["a", "g"])
def test_the_comparison_rejects_the_slips(oracle_mod, label):
    """The GPU tests' comparison (channel_terms.compare at the throughput bar, the loosest; scale s for c and 1 for u) fed with the
    oracle's own outputs of a case with mixed folds (`mirrored` at 16 views; `scattered` with a 450-mm object), each slip of
    weighted_terms.SLIPS applied: every one is rejected, by the printed factor (at least 10 is asserted).  Nothing runs on a GPU."""
    Ps, n_u, n_v, data, weights, K01s = W.case_inputs(label)
    derivative = W.settings(label)[6]
    t = W.case_terms(label)
    want, scales = W.columns(t)
    tol = T.TOL_THROUGHPUT
    assert T.compare(want, want, scales, tol).max() == 0.0
    assert (t["fold"] == "mixed").sum() >= 5 and derivative
    for slip in W.SLIPS:
        got, _ = W.columns(W.scan_terms(Ps, data, weights, n_u, n_v, K01s, derivative=derivative, slip=slip))
        ratio = T.compare(got, want, scales, tol)
        print("case %s, %-24s rejected %.3g-fold (c %.3g, u %.3g)" % (label, slip, ratio.max(), ratio[0], ratio[1]))
        assert ratio.max() >= 10.0, (slip, ratio)
        if slip == "coverage_over_n_kappa":
            assert ratio[0] == 0.0   # the value column is not touched by it
        elif slip in ("fold_sign_on_weights", "difference_of_weighted"):
            assert ratio[0] >= 10.0, (slip, ratio)
