"""The oracle's differences between poses (tests/pose_response.py) against evaluate_all on full matrix sets (no GPU).

The GPU tests of tests/test_gpu_pose_response.py measure the library's S(+h) - S(-h) against these moved-pair sums; this file
holds the helper itself to the plain all-pairs oracle."""
import numpy as np
import pytest

import pose_response as R
from conftest import make_small_scan

N, S, BINS, V = 24, 128, 96, 13  # (view 13: the weakest DoF, rz, still resolved 9.7e3-fold)


@pytest.fixture(scope="module")
def scan(oracle_mod):
    Ps, imgs = make_small_scan(N, S, S)
    return Ps, [oracle_mod.radon(im, BINS, BINS) for im in imgs]


def test_moved_pair_sums_equal_full_evaluations(oracle_mod, scan):
    """Every pose of the 6-DoF grid of view V: the helper's pair values are evaluate_all's bit for bit (both variants), and its
    differences of moved-pair sums are the differences of the all-pairs float64 sums to 1e-12 of the total; the largest step of
    every DoF is resolved: |D_64| >= 1e3 |D_0 - D_64|."""
    Ps, dtrs = scan
    labels, mats = R.pose_grid(Ps[V])
    res = R.moved_pair_response(oracle_mod, Ps, dtrs, S, S, V, mats)
    q = res["pairs"][:, 0]
    assert len(q) == N - 1 and ((res["pairs"][:, 1] == V) | (res["pairs"][:, 2] == V)).all()
    full = {}
    try:
        for var in (0, 1):
            oracle_mod.set_variant(var)
            sums = []
            for k, P in enumerate(mats):
                Pk = list(Ps)
                Pk[V] = P
                r = oracle_mod.evaluate_all(Pk, dtrs, S, S)
                assert np.array_equal(r["pairs"][q], res[var]["values"][k]), (var, labels[k])
                sums.append(r["pairs"].astype(np.float64).sum())
            full[var] = np.array(sums)
    finally:
        oracle_mod.set_variant(0)
    total = abs(full[0][0])
    for var in (0, 1):
        mine, theirs = R.cells(labels, res[var]["sums"]), R.cells(labels, full[var])
        for key in mine:
            for a, b in zip(mine[key], theirs[key]):
                assert abs(a - b) <= 1e-12 * total, (var, key, a, b)
    c0, c64 = R.cells(labels, res[0]["sums"]), R.cells(labels, res[1]["sums"])
    for dof in R.DOFS:
        h = R.steps(dof)[0]
        D0, D64 = c0[(dof, h)][0], c64[(dof, h)][0]
        print("%s %g: D_64 %.4e, |D_0 - D_64| %.2e" % (dof, h, D64, abs(D0 - D64)))
        assert abs(D64) >= 1e3 * abs(D0 - D64), (dof, h, D0, D64)


def test_moved_view_zero_is_refused(oracle_mod, scan):
    """View 0 sets the automatic object radius of every pair: the moved-pair form does not apply (all_pairs_response does)."""
    Ps, dtrs = scan
    with pytest.raises(ValueError):
        R.moved_pair_response(oracle_mod, Ps, dtrs, S, S, 0, [Ps[0]])
    r = R.all_pairs_response(oracle_mod, Ps, dtrs, S, S, 0, [Ps[0]])
    assert np.array_equal(r[0]["values"][0], oracle_mod.evaluate_all(Ps, dtrs, S, S)["pairs"])


def test_kappa_sample_count_rule(oracle_mod, scan):
    """kappa_samples applies the pair loop's rule to K01: its total over all pairs is the oracle's own count of loop trips."""
    Ps, dtrs = scan
    for dkappa in (0.0, 0.004):
        r = oracle_mod.evaluate_all(Ps, dtrs, S, S, dkappa=dkappa, want_K01=True)
        got = R.kappa_samples(r["K01s"], dkappa, S, S, BINS)
        assert got.sum() == r["n_kappa"] and (got > 0).all(), (dkappa, got.sum(), r["n_kappa"])
