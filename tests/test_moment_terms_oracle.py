"""The direct float64 statement of the three moment blocks per pair (tests/moment_terms.py) against channel_terms.pair_terms and
against the C oracle (no GPU).

tests/test_gpu_view_hessian.py compares every pair-block entry ecc_metric_evaluate_view_hessian returns with
moment_terms.scan_moments; this file holds that helper to the statement of the per-view call through the one-hot identity, to
oracle.evaluate_pairs through zeroed intermediates and the polarisation of the exactly quadratic pair value, and shows that the
comparison the GPU test makes rejects the slips it is there for."""
import numpy as np
import pytest

import channel_terms as T
import geometry_catalog
import moment_terms as M


def _scan(name, n, n_alpha, n_t, K, seed=5):
    """A catalog geometry and K * n intermediates, channel-major, mixed like channel_terms.case_data's (correlated channels)."""
    Ps, n_u, n_v = geometry_catalog.make(name, n)
    rng = np.random.default_rng(seed)
    host = [None] * (K * n)
    for i in range(n):
        noise = rng.standard_normal((K, n_t, n_alpha))
        for c in range(K):
            host[c * n + i] = np.tensordot(T.MIX[c, :K], noise, axes=1).astype(np.float32)
    return Ps, n_u, n_v, host


@pytest.mark.parametrize("positions", ["float32", "float64"])
@pytest.mark.parametrize("derivative", [True, False])
def test_blocks_are_pair_terms_at_one_hot_coefficients(oracle_mod, derivative, positions):
    """a0 = e_c, a1 = 0: delta = v0_c, so h0 = P00[c, :] and h1 = P01[c, :]; a0 = 0, a1 = e_c: delta = -v1_c, so h1 = P11[c, :] and
    h0 = P01[:, c] -- to 1e-12 of the entries' Cauchy-Schwarz scales (float64 rounding of sums of a few thousand terms), on every
    pair of `mirrored` at 8 views, K = 4 (opposite and mixed folds among them)."""
    K, n = 4, 8
    Ps, n_u, n_v, host = _scan("mirrored", n, 96, 64, K)
    K01s = oracle_mod.evaluate_all(Ps, host[:n], n_u, n_v, is_derivative=derivative, want_K01=True)["K01s"]
    m = M.scan_moments(Ps, host, K, n_u, n_v, derivative=derivative, positions=positions, K01s=K01s)
    D = [np.stack([np.asarray(host[c * n + i], np.float64) for c in range(K)]) for i in range(n)]
    worst, live = 0.0, 0
    for r, (i, j) in enumerate(m["ij"]):
        for c in range(K):
            e, z = np.eye(K)[c], np.zeros(K)
            t = T.pair_terms(K01s[r], D[i], D[j], e, z, n_u, n_v, derivative, positions)
            worst = max(worst, float(T.compare(t["h0"], m["P00"][r, c], m["S00"][r, c], 1e-12).max()),
                        float(T.compare(t["h1"], m["P01"][r, c], m["S01"][r, c], 1e-12).max()))
            t = T.pair_terms(K01s[r], D[i], D[j], z, e, n_u, n_v, derivative, positions)
            worst = max(worst, float(T.compare(t["h1"], m["P11"][r, c], m["S11"][r, c], 1e-12).max()),
                        float(T.compare(t["h0"], m["P01"][r, :, c], m["S01"][r, :, c], 1e-12).max()))
        live += m["P00"][r, 0, 0] > 0
    print("derivative %s, %s positions: worst one-hot difference %.3g of the scale, %d live pairs" % (derivative, positions, worst * 1e-12, live))
    assert worst <= 1.0 and live >= 20, (worst, live)


def test_blocks_are_symmetric_and_compose_the_pair_value(oracle_mod):
    """P00 and P11 are symmetric and positive semi-definite; the pair value of channel_terms at random coefficients is
    a_i^T P00 a_i + a_j^T P11 a_j + 2 a_i^T P01 a_j to 1e-12 of the same expression on magnitudes; columns / blocks / assemble are
    consistent: a^T H a is the mean of the pair values."""
    K, n = 3, 8
    Ps, n_u, n_v, host = _scan("mirrored", n, 96, 64, K)
    a = np.random.default_rng(2).uniform(0.5, 1.5, (K, n))
    t = T.scan_terms(Ps, host, a, n_u, n_v)
    m = M.scan_moments(Ps, host, K, n_u, n_v, K01s=t["K01s"])
    for r, (i, j) in enumerate(m["ij"]):
        assert np.array_equal(m["P00"][r], m["P00"][r].T) and np.array_equal(m["P11"][r], m["P11"][r].T)
        assert np.linalg.eigvalsh(m["P00"][r])[0] >= -1e-12 * np.trace(m["P00"][r])
        form = a[:, i] @ m["P00"][r] @ a[:, i] + a[:, j] @ m["P11"][r] @ a[:, j] + 2.0 * a[:, i] @ m["P01"][r] @ a[:, j]
        mag = a[:, i] @ np.abs(m["P00"][r]) @ a[:, i] + a[:, j] @ np.abs(m["P11"][r]) @ a[:, j] + 2.0 * a[:, i] @ np.abs(m["P01"][r]) @ a[:, j]
        assert abs(form - t["value"][r]) <= 1e-12 * mag, (r, form, t["value"][r])
    rows, _ = M.columns(m)
    assert rows.shape == (n * (n - 1) // 2, M.n_columns(K)) and len(M.column_names(K)) == M.n_columns(K)
    P00, P11, P01 = M.blocks(rows, K)
    assert np.array_equal(P00, m["P00"]) and np.array_equal(P11, m["P11"]) and np.array_equal(P01, m["P01"])
    H, A = M.assemble(rows, n, K)
    assert np.array_equal(H, H.T) and np.all(np.abs(H) <= A)
    flat = a.reshape(-1)
    assert abs(flat @ H @ flat - t["mean"]) <= 1e-12 * (flat @ A @ flat)
    assert np.max(np.abs(2.0 * (H @ flat) - t["grad"].reshape(-1))) <= 1e-12 * np.max(A @ flat)


@pytest.mark.parametrize("name,n,n_alpha,n_t,radius", [("mirrored", 16, 768, 768, 0.0), ("near_opposite", 16, 768, 768, 185.0),
                                                       ("scattered", 12, 1000, 767, 0.0)])
def test_blocks_are_the_c_oracles(oracle_mod, name, n, n_alpha, n_t, radius):
    """K = 3, every pair, one index-list call of the C oracle.  With view j's intermediate zero the oracle's pair value on channel c
    of view i is P00[c, c]; with view i's zero it is P11[c, c] -- to 2e-7 relative, the float rounding of the stored pair value
    (tests/test_channel_terms_oracle.py::test_values_are_the_c_oracles).  The pair value is exactly quadratic, so with channel c in
    view i and +-channel d in view j (a negated float32 array is exact), P01[c, d] = (p+ - p-) / 4 -- to 1e-6 of sqrt(P00_cc P11_dd)
    (test_gradient_terms_are_the_c_oracles_polarisation's bar: the float32 rounding of two pair values of about twice the scale)."""
    K = 3
    Ps, n_u, n_v, host = _scan(name, n, n_alpha, n_t, K)
    K01s = oracle_mod.evaluate_all(Ps, host[:n], n_u, n_v, object_radius_mm=radius, want_K01=True)["K01s"]
    m = M.scan_moments(Ps, host, K, n_u, n_v, object_radius_mm=radius, K01s=K01s)
    dtrs = list(host) + [-h for h in host] + [np.zeros_like(host[0])]
    minus, zero = K * n, 2 * K * n
    rows, labels = [], []
    for r, (i, j) in enumerate(m["ij"]):
        for c in range(K):
            rows.append((i, j, c * n + i, zero))
            labels.append(("P00", r, c, c, 1.0))
            rows.append((i, j, zero, c * n + j))
            labels.append(("P11", r, c, c, 1.0))
            for d in range(K):
                rows.append((i, j, c * n + i, d * n + j))
                labels.append(("P01", r, c, d, 0.25))
                rows.append((i, j, c * n + i, minus + d * n + j))
                labels.append(("P01", r, c, d, -0.25))
    vals = oracle_mod.evaluate_pairs(Ps, dtrs, n_u, n_v, rows, object_radius_mm=radius)["pairs"].astype(np.float64)
    got = {}
    for (block, r, c, d, s), v in zip(labels, vals):
        got[block, r, c, d] = got.get((block, r, c, d), 0.0) + s * v
    worst = dict(P00=0.0, P11=0.0, P01=0.0)
    for (block, r, c, d), v in got.items():
        want = m[block][r, c, d]
        scale, tol = (abs(want), 2e-7) if block != "P01" else (m["S01"][r, c, d], 1e-6)
        worst[block] = max(worst[block], float(T.compare(want, v, scale, tol)))
    live = int((m["P00"][:, 0, 0] > 0).sum())
    print("%s %d: worst P00 %.3g, P11 %.3g relative; P01 against the polarisation %.3g of the scale; %d live pairs"
          % (name, n, worst["P00"] * 2e-7, worst["P11"] * 2e-7, worst["P01"] * 1e-6, live))
    assert len(got) == len(m["ij"]) * (2 * K + K * K) and live >= 0.8 * len(m["ij"])
    assert max(worst.values()) <= 1.0, worst


def test_the_comparison_rejects_the_slips(oracle_mod):
    """The GPU test's comparison (channel_terms.compare at the throughput bar, the loosest) fed with the oracle's own blocks of case a
    (`mirrored`, 16 views, 46 opposite-fold pairs), each of these slips applied: every one is rejected at least 100-fold.  The
    views' noise fields are independent, so P01 is about 0.03 of its scale and P00 differs from P11 by a few per cent: the 1e-3 bar
    is still 100 times below what a slip moves.  Measured: 176-, 392- and 287-fold.  Nothing runs on a GPU."""
    key = "a"
    K = T.CASES[key][4]
    t, m = T.case_terms(key), M.case_moments(key)
    want, scales = M.columns(m)
    tri, tol = K * (K + 1) // 2, T.TOL_THROUGHPUT
    assert T.compare(want, want, scales, tol).max() == 0.0

    def rejected(label, got):
        worst = float(np.max(T.compare(got, want, scales, tol)))
        print("%-50s rejected %.3g-fold" % (label, worst))
        assert worst >= 100.0, (label, worst)

    P00, P11, P01 = M.blocks(want, K)
    got = want.copy()
    got[:, 2 * tri:] = P01.transpose(0, 2, 1).reshape(len(want), K * K)
    rejected("P01 transposed", got)
    got = want.copy()
    got[:, :tri], got[:, tri:2 * tri] = want[:, tri:2 * tri], want[:, :tri]
    rejected("P00 and P11 exchanged", got)
    opposite = t["fold"] == "opposite"
    got = want.copy()
    got[opposite, 2 * tri:] *= -1.0
    rejected("P01 without the relative sign on opposite folds", got)
    assert np.array_equal(got[~opposite], want[~opposite]) and opposite.sum() >= 30
