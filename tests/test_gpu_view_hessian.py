"""ecc_metric_evaluate_view_hessian (csrc/ecc_view_hessian.hip, csrc/view_hessian_kernel.hip): the quadratic form of per-view channel
coefficients as a matrix -- three moment blocks P00, P11, P01 per pair in float64 and the (n K) x (n K) matrix H assembled from them.

The contract (include/ecc_hip.h): (1) every pair-block entry agrees with the direct float64 statement of tests/moment_terms.py on
the cases of channel_terms.CASES, relative to its Cauchy-Schwarz scale, at the project's bars; (2) it agrees with the n K one-hot
calls of evaluate_view_coefficients, which read identical samples, to 1e-6 of the same scale; (3) H is assembled without atomics:
symmetric bit for bit, off-diagonal entries the bits of P01 / N, diagonal blocks one fixed-order float64 sum, the same bits on every
run, nothing else on the metric moved; (4) a^T H a and 2 H a are evaluate_view_coefficients' value and gradient; (5) where the form
is a 10^6 times smaller difference of its moments it still has the value's digits -- what float32 products could not give; (6) the
direct solve reaches conjugate gradients' minimum; (7) its argument errors on a live metric."""
import ctypes as C

import numpy as np
import pytest

import channel_terms as T
import moment_terms as M

pytestmark = pytest.mark.gpu

STEPS = np.array([0.5, 0.5, 0.5, np.deg2rad(0.1), np.deg2rad(0.1), np.deg2rad(0.1)])


def _scan(gpu_ctx, n, K, S=128, B=48, seed=5):
    """tests/test_gpu_view_coefficients.py::_scan: the planar short scan and K * n DIFFERENT random-normal intermediates."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import synthetic
    rng = np.random.default_rng(seed)
    Ps = synthetic.short_scan(n, S, S, 0.308 * 1024 / S)
    host = [rng.standard_normal((B, B)).astype(np.float32) for _ in range(K * n)]
    dtrs = [E.RadonIntermediate.from_host(gpu_ctx, h, S, S) for h in host]
    return Ps, dtrs, host


def _close(dtrs):
    for d in dtrs:
        d.close()


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# ---- 1. the blocks against the direct oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(T.CASES))
def test_blocks_against_the_direct_oracle(gpu_ctx, oracle_mod, key):
    """One case of channel_terms.CASES with its sampling and quad settings: every pair-block entry against moment_terms, relative to
    its scale, at channel_terms.tolerance's bar; the records say that the case reached its loop (tests/test_gpu_channel_terms.py's
    assertions, imported)."""
    import epipolarconsistency_amd as E
    import test_gpu_channel_terms as G
    name, n, n_alpha, n_t, K, radius, dkappa, derivative, setups = T.CASES[key]
    Ps, n_u, n_v, host, _ = T.case_data(key)
    t, mo = T.case_terms(key), M.case_moments(key)
    N = n * (n - 1) // 2
    rows = mo["pairs"]
    want, scale = M.columns(mo)
    names = M.column_names(K)
    kw = {} if derivative else dict(filter=E.FILTER_NONE)
    failures = []
    gpu_ctx.setQuadCopies(setups[0][1])
    try:
        dtrs = [E.RadonIntermediate.from_host(gpu_ctx, h, n_u, n_v, **kw) for h in host]
        rec = G._records(gpu_ctx, Ps, dtrs, radius, dkappa)
        for sampling, _ in setups:
            G._reached(key, sampling, rec, t, N)
            tol = T.tolerance(sampling, N)
            m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling(sampling)
            m.setObjectRadius(radius)
            m.setEpipolarPlaneStep(dkappa)
            H, blocks = m.evaluate_view_hessian(K, want_pairs=True)
            m.close()
            assert blocks.shape == (N, M.n_columns(K)) and H.shape == (n * K, n * K) and np.all(np.isfinite(H))
            worst, line = G._worst("case %s %s, pair blocks" % (key, sampling), blocks[rows], want, scale, tol, t, names)
            if not worst <= 1.0:
                failures.append(line)
            if tol == T.TOL_THROUGHPUT:   # reported: the same against the float64-position statement
                w64, _ = M.columns(M.case_moments(key, "float64"))
                print("case %s %s, against float64 positions: %.3g of the bar" % (key, sampling, T.compare(blocks[rows], w64, scale, tol).max()))
    finally:
        gpu_ctx.setQuadCopies("auto")
    _close(dtrs)
    assert not failures, "\n".join(failures)


# ---- 2. the blocks against the existing call -----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("mode", ["auto", "polynomial"])
def test_blocks_against_one_hot_view_coefficients(gpu_ctx, mode, K):
    """8 views, 48 x 48 bins: the n K calls of evaluate_view_coefficients(want_pairs=True) at one-hot coefficients.  With the 1 at
    (c, i): in a pair (i, j) h0 = P00[c, :] and h1 = P01[c, :]; in a pair (w, i) h1 = P11[c, :] and h0 = P01[:, c].  Both sides read
    identical samples; the comparator rounds each sample term at most three times in float32 and the pair entry once (<= 4 * 2^-24 of
    the scale), this side rounds nothing in float32: 1e-6 of the Cauchy-Schwarz scale."""
    import epipolarconsistency_amd as E
    n = 8
    Ps, dtrs, _ = _scan(gpu_ctx, n, K)
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling(mode)
    _, blocks = m.evaluate_view_hessian(K, want_pairs=True)
    P00, P11, P01 = M.blocks(blocks, K)
    d0, d1 = np.einsum("pcc->pc", P00), np.einsum("pcc->pc", P11)
    iu = np.triu_indices(n, 1)
    worst, checked = 0.0, 0
    for c in range(K):
        for i in range(n):
            a = np.zeros((K, n), np.float32)
            a[c, i] = 1.0
            pairs = m.evaluate_view_coefficients(a, want_pairs=True)[2].astype(np.float64)
            for q in range(len(pairs)):
                h0, h1 = pairs[q, 1:1 + K], pairs[q, 1 + K:]
                if iu[0][q] == i:
                    checks = [(h0, P00[q, c], np.sqrt(d0[q, c] * d0[q])), (h1, P01[q, c], np.sqrt(d0[q, c] * d1[q]))]
                elif iu[1][q] == i:
                    checks = [(h1, P11[q, c], np.sqrt(d1[q, c] * d1[q])), (h0, P01[q, :, c], np.sqrt(d0[q] * d1[q, c]))]
                else:
                    assert not pairs[q].any()   # the pair holds no view with a coefficient
                    continue
                for got, want, scale in checks:
                    worst = max(worst, float(T.compare(want, got, scale, 1e-6).max()))
                    checked += K
    m.close()
    _close(dtrs)
    print("%s, K = %d: %d entries, worst |block - one-hot term| %.3g of the scale" % (mode, K, checked, worst * 1e-6))
    assert checked == 2 * K * K * n * (n - 1) and (d0 > 0).all() and worst <= 1.0, worst


# ---- 3. assembly -----------------------------------------------------------------------------------------------------------------
def _rigid_probes(P34):
    from epipolarconsistency_amd import geometry as Gm, pack_projection_matrices
    names = ("tx", "ty", "tz", "rx", "ry", "rz")
    return pack_projection_matrices([Gm.compose_transform(P34, Gm.rigid_transform(**{names[k]: s * STEPS[k]}))
                                     for k in range(6) for s in (1.0, -1.0)])


@pytest.mark.parametrize("n,K", [(20, 3), (100, 2), (9, 4), (13, 1)])
def test_assembly_and_nothing_else_moved(gpu_ctx, n, K):
    """H == H^T bit for bit; every off-diagonal entry has the bits of P01 / N of the returned pair blocks; every diagonal-block entry
    is within 4 n 2^-53 sum |terms| of numpy's float64 sum of the returned blocks (n - 1 additions in another order); two calls
    return identical bits; evaluate() (one view moved and back: the kept records of the reuse path are in play at n = 100), a pose
    batch (evaluate_gradient) and a Gram call on the same metric have the same bits before and after the call."""
    import epipolarconsistency_amd as E
    Ps, dtrs, _ = _scan(gpu_ctx, n, K, B=32)
    P0 = E.pack_projection_matrices(Ps)
    view = n // 2
    rows = _rigid_probes(P0[view].reshape(4, 3).T)
    P1 = P0.copy()
    P1[view] = rows[0]
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs)

    def observe(q):
        base = q.setProjectionMatrices(P0).evaluate()
        moved = q.setProjectionMatrices(P1).evaluate()
        back = q.setProjectionMatrices(P0).evaluate()
        value, grad = q.evaluate_gradient(view, rows[0::2], rows[1::2], STEPS)
        G = q.evaluate_gram(K)
        cost = np.zeros((n, n), np.float32)
        with_cost = q.evaluate(cost)
        return np.concatenate([[base, moved, back, value, with_cost], grad, G.reshape(-1)]), cost
    before, cost_b = observe(m)
    H, blocks = m.evaluate_view_hessian(K, want_pairs=True)
    after, cost_a = observe(m)
    assert np.array_equal(_u64(before), _u64(after)) and np.array_equal(_u32(cost_b), _u32(cost_a))
    N = n * (n - 1) // 2
    assert H.shape == (n * K, n * K) and blocks.shape == (N, M.n_columns(K)) and np.all(np.isfinite(H))
    assert np.array_equal(_u64(H), _u64(H.T))
    want, mag = M.assemble(blocks, n, K)
    diag = np.zeros((K, n, K, n), bool)
    diag[:, np.arange(n), :, np.arange(n)] = True
    diag = diag.reshape(n * K, n * K)
    assert np.array_equal(_u64(H[~diag]), _u64(want[~diag]))   # P01 / N, one IEEE division each
    bound = 4.0 * n * 2.0 ** -53 * mag[diag]
    err = np.abs(H[diag] - want[diag])
    print("%d views, K = %d: diagonal blocks: worst |H - numpy's sum| %.3g of the bound 4 n 2^-53 sum |terms|" % (
        n, K, float(np.max(err / np.where(bound > 0, bound, 1.0)))))
    assert np.all(err <= bound) and np.all(np.diag(H) > 0)
    # in the middle of a sequence: matrices moved, then the call, then back; H alone and H with blocks
    m.setProjectionMatrices(P1).evaluate()
    moved = m.evaluate_view_hessian(K)
    assert _u64(m.evaluate())[()] == _u64(before[1])[()]          # the moved matrices are still current
    assert _u64(m.setProjectionMatrices(P0).evaluate())[()] == _u64(before[0])[()]
    H2, blocks2 = m.evaluate_view_hessian(K, want_pairs=True)
    assert np.array_equal(_u64(H2), _u64(H)) and np.array_equal(_u64(blocks2), _u64(blocks))
    assert np.array_equal(_u64(m.evaluate_view_hessian(K)), _u64(H)) and not np.array_equal(moved, H)
    assert np.array_equal(_u64(m.evaluate_view_hessian(K, want_pairs=True, want_matrix=False)), _u64(blocks))   # the blocks alone
    with pytest.raises(ValueError):
        m.evaluate_view_hessian(K, want_pairs=False, want_matrix=False)
    m.close()
    _close(dtrs)


def test_a_large_matrix_is_not_kept_on_the_device(gpu_ctx):
    """725 views of four channels: n K = 2 900, H is 67 MB -- above the 64 MB the metric keeps between calls, so this is the path on
    which the device matrix is freed when the call returns and allocated again by the next (four tiny intermediates over and over:
    262 450 pairs of 16 x 16 bins).  The test cannot tell freed from kept -- nothing public reports the metric's device memory, and
    the 64 MB are a judgement, not a measurement; a repeated large call pays an allocation every time -- it checks that the path
    works: both calls return the same bits, symmetric, with a positive diagonal, and a blocks-only call on the same metric follows."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import synthetic
    n, K = 725, 4
    rng = np.random.default_rng(9)
    tiny = [E.RadonIntermediate.from_host(gpu_ctx, rng.standard_normal((16, 16)).astype(np.float32), 128, 128) for _ in range(7)]
    m = E.MetricRadonIntermediate(gpu_ctx, synthetic.short_scan(n, 128, 128, 0.308 * 1024 / 128), [tiny[(3 * (k // n) + k % n) % 7] for k in range(n * K)])
    H = m.evaluate_view_hessian(K)
    assert H.shape == (n * K, n * K) and H.nbytes > 64 << 20
    assert np.array_equal(H, H.T) and np.all(np.isfinite(H)) and np.all(np.diag(H) > 0)
    again = m.evaluate_view_hessian(K)
    assert np.array_equal(_u64(again), _u64(H))
    blocks = m.evaluate_view_hessian(K, want_pairs=True, want_matrix=False)
    assert np.array_equal(_u64(blocks[:, -K * K:].reshape(-1, K, K)[0] / (n * (n - 1) // 2)), _u64(H[0::n, 1::n][:, :K]))   # pair (0, 1): P01 / N
    m.close()
    _close(tiny)


# ---- 4. the form -----------------------------------------------------------------------------------------------------------------
def test_the_form_is_the_per_view_call(gpu_ctx):
    """12 views, K = 3, polynomial, a ~ U(0.5, 1.5): a^T H a against evaluate_view_coefficients' value to 1e-6 M, M the same sum with
    every term's magnitude; 2 H a against its gradient to 1e-6 of the per-entry sum of magnitudes."""
    import epipolarconsistency_amd as E
    n, K = 12, 3
    Ps, dtrs, _ = _scan(gpu_ctx, n, K)
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling("polynomial")
    a = np.random.default_rng(5).uniform(0.5, 1.5, (K, n)).astype(np.float32)
    value, grad = m.evaluate_view_coefficients(a)
    H = m.evaluate_view_hessian(K)
    m.close()
    _close(dtrs)
    flat = a.astype(np.float64).reshape(-1)
    f, Mag = E.view_hessian_value(H, a), float(np.abs(flat) @ np.abs(H) @ np.abs(flat))
    g, gmag = 2.0 * (H @ flat), 2.0 * (np.abs(H) @ np.abs(flat))
    print("a^T H a = %.9g, the call's value %.9g: %.3g of M = %.6g; 2 H a: worst %.3g of its magnitudes" % (
        f, value, abs(f - value) / Mag, Mag, float(np.max(np.abs(g - grad.reshape(-1)) / gmag))))
    assert value > 0 and abs(f - value) <= 1e-6 * Mag
    assert np.all(np.abs(g - grad.reshape(-1)) <= 1e-6 * gmag)


# ---- 5. cancellation -------------------------------------------------------------------------------------------------------------
def test_the_form_keeps_its_digits_under_cancellation(gpu_ctx):
    """The test float32 products cannot pass.  K = 2, 8 views, 48 x 48 bins, D_1,i = D_0,i + 2^-10 N_i (mixed in float64, rounded
    once) and a = (1, -1) for every view: f(a) is the metric of the 2^-10 N_i, about 10^6 times smaller than the moments it is the
    difference of.  The comparator, evaluate_view_coefficients, forms v0 - v1 per sample (exact for nearly equal floats) and has no
    cancellation; f from H must agree with it to 1e-5 of the value, the project's bar for means.  With float32 products or float32
    pair entries the moments' error, 6e-8 of M, would be 6e-8 M / f >= 6e-3 of the value."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import synthetic
    n, K, S, B = 8, 2, 128, 48
    rng = np.random.default_rng(5)
    Ps = synthetic.short_scan(n, S, S, 0.308 * 1024 / S)
    D0 = [rng.standard_normal((B, B)) for _ in range(n)]
    D1 = [d + 2.0 ** -10 * rng.standard_normal((B, B)) for d in D0]
    host = [d.astype(np.float32) for d in D0 + D1]
    dtrs = [E.RadonIntermediate.from_host(gpu_ctx, h, S, S) for h in host]
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs)
    a = np.stack([np.ones(n), -np.ones(n)]).astype(np.float32)
    value = m.evaluate_view_coefficients(a)[0]
    H = m.evaluate_view_hessian(K)
    m.close()
    _close(dtrs)
    flat = a.astype(np.float64).reshape(-1)
    f, Mag = E.view_hessian_value(H, a), float(np.abs(flat) @ np.abs(H) @ np.abs(flat))
    print("f from H %.9g, the call's value %.9g: relative difference %.3g; cancellation factor M / f = %.3g" % (
        f, value, abs(f - value) / value, Mag / f))
    assert value > 0 and Mag / f >= 1e5, Mag / f   # or the test does not mean what it says
    assert abs(f - value) <= 1e-5 * value, (f, value)


# ---- 6. the solve ----------------------------------------------------------------------------------------------------------------
class _ExactForm:
    """The device's H behind minimize_view_coefficients' interface, with float64 products: value a^T H a, gradient 2 H a."""

    def __init__(self, H, K, n):
        self.H, self.K, self.n = H, K, n

    def evaluate_view_coefficients(self, coeffs, want_pairs=False):
        a = np.asarray(coeffs, np.float64).reshape(-1)
        assert a.size == self.K * self.n and not want_pairs
        return float(a @ self.H @ a), (2.0 * (self.H @ a)).reshape(self.K, self.n)


def _gradient_floor(m, a, K, n):
    """What float32 allows the device call's gradient at coefficients a, per entry, from the per-view call alone (nothing here reads
    H).  A term h0[c] of the pair q = (i, j) is w sum_s fl(delta_s) v0_c,s: delta is formed in float32 in K roundings per side and one
    for the difference, each at most 2^-24 of mu_s = sum_d |a_d,i v0_d,s| + |a_d,j v1_d,s|; the product pair takes two roundings, the
    weight one, the float32 pair entry one, each at most 2^-24 of mu_s |v0_c,s| or of their sum; the coefficients arrive as float32,
    one more.  By Cauchy-Schwarz and Minkowski w sum_s mu_s |v0_c,s| <= m_q sqrt(P00_cc), m_q = sum_d |a_d,i| sqrt(P00_dd) +
    |a_d,j| sqrt(P11_dd), so a term is within (2 K + 6) 2^-24 m_q sqrt(P00_cc) (h1: P11_cc), and a gradient entry within 2 / N times the
    sum over the view's pairs.  P00_dd / P11_dd of a pair are the pair values of the call at one-hot coefficients (contract 1 of the
    per-view call: evaluate()'s bits on that channel alone)."""
    iu = np.triu_indices(n, 1)
    N = len(iu[0])
    d0, d1 = np.zeros((N, K)), np.zeros((N, K))
    for c in range(K):
        for i in range(n):
            e = np.zeros((K, n), np.float32)
            e[c, i] = 1.0
            values = m.evaluate_view_coefficients(e, want_pairs=True)[2][:, 0].astype(np.float64)
            d0[iu[0] == i, c] = values[iu[0] == i]
            d1[iu[1] == i, c] = values[iu[1] == i]
    mag = np.abs(a)
    m_q = (mag[:, iu[0]].T * np.sqrt(d0)).sum(axis=1) + (mag[:, iu[1]].T * np.sqrt(d1)).sum(axis=1)
    floor = np.zeros((K, n))
    for c in range(K):
        np.add.at(floor[c], iu[0], m_q * np.sqrt(d0[:, c]))
        np.add.at(floor[c], iu[1], m_q * np.sqrt(d1[:, c]))
    return (2 * K + 6) * 2.0 ** -24 * 2.0 / N * floor


def test_direct_solve_against_conjugate_gradients(gpu_ctx):
    """8 views, K = 2, channel 0 fixed at 1 and channel 1 free, H from the device.

    (a) view_hessian_minimizer(H) and minimize_view_coefficients(tol=1e-9) reach the same coefficients within the latter's bound: it
    stops at |r|_inf <= tol |g0|_inf, so it is within sqrt(n_free) tol |g0|_inf / lambda_min(2 H[F, F]) of the minimiser, twice that
    asserted (tests/test_view_coefficients_abi.py).  The bound presumes the helper's operator products are the form's, so the helper
    is given the form itself: the device's H with float64 products.  Through the DEVICE call its products are float32 (the direction
    is passed as float32, every pair term rounded to float32) and the same comparison cannot hold: measured on an MI355X the
    coefficients differ by 3.25e-08 against a bound of 5.07e-09; that figure is printed, not asserted.
    (b) What the float32 call can reach, asserted instead of it: the device call's free gradient at the direct solution is within
    the call's float32 floor (_gradient_floor, formed from the per-view call alone) -- the direct solution IS the minimum of the form
    the device evaluates, to what the device can tell.  (The floor must itself be at least 10^4 times below the gradient at the start, or
    being under it would say nothing.)
    (c) The metric at the direct solution is no larger than at the device's conjugate-gradient solution plus 1e-6 M.
    Measured on an MI355X: (a) 6.3e-17 against the bound 5.07e-09; (b) |g| <= 4.87e-07 against a floor >= 5.02e-05, worst entry 0.009
    of its floor, the gradient at the start 28.7."""
    import epipolarconsistency_amd as E
    n, K, tol = 8, 2, 1e-9
    Ps, dtrs, _ = _scan(gpu_ctx, n, K)
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs)
    start = np.ones((K, n))
    start[1] = np.random.default_rng(3).uniform(-0.5, 0.5, n)
    free = np.zeros((K, n), bool)
    free[1] = True
    H = m.evaluate_view_hessian(K)
    a, f = E.view_hessian_minimizer(H, start, free)
    b, _, its = E.minimize_view_coefficients(_ExactForm(H, K, n), K, start, free, tol=tol)
    b_dev, value_cg, its_dev = E.minimize_view_coefficients(m, K, start, free, tol=tol)
    a32 = a.astype(np.float32)
    value_direct, grad_direct = m.evaluate_view_coefficients(a32)
    g_start = m.evaluate_view_coefficients(start.astype(np.float32))[1]
    floor = _gradient_floor(m, a32.astype(np.float64), K, n)
    m.close()
    _close(dtrs)
    F = free.reshape(-1)
    g0 = (2.0 * H @ start.reshape(-1))[F]
    bound = 2.0 * np.sqrt(F.sum()) * tol * np.max(np.abs(g0)) / np.linalg.eigvalsh(2.0 * H[np.ix_(F, F)])[0]
    flat = np.abs(a.reshape(-1))
    Mag = float(flat @ np.abs(H) @ flat)
    print("direct solve against %d conjugate-gradient products on H: coefficients differ by %.3g (bound %.3g); against %d products of "
          "the device call: %.3g (not asserted)" % (its, np.max(np.abs(a - b)), bound, its_dev, np.max(np.abs(a - b_dev))))
    print("free gradient of the device call at the direct solution: worst %.3g of its float32 floor (|g| <= %.3g, floor >= %.3g, at "
          "the start |g| = %.3g); value %.9g (from H %.9g) against conjugate gradients' %.9g, M = %.6g" % (
              float(np.max(np.abs(grad_direct[free]) / floor[free])), np.abs(grad_direct[free]).max(), floor[free].min(),
              np.abs(g_start[free]).max(), value_direct, f, value_cg, Mag))
    assert np.array_equal(_u64(a[0]), _u64(start[0])) and not np.array_equal(a[1], start[1])
    assert its >= 1 and np.max(np.abs(a - b)) <= bound, (np.max(np.abs(a - b)), bound)                       # (a)
    assert np.all(np.abs(grad_direct[free]) <= floor[free]) and floor[free].max() <= 1e-4 * np.abs(g_start[free]).max()   # (b)
    assert value_direct <= value_cg + 1e-6 * Mag, (value_direct, value_cg)                                   # (c)


# ---- 7. argument errors on a live metric -----------------------------------------------------------------------------------------
def test_errors(gpu_ctx):
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib, synthetic
    n, K = 8, 2
    Ps, dtrs, _ = _scan(gpu_ctx, n, K)
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs)
    want = m.evaluate()
    H = m.evaluate_view_hessian(K)
    for bad in (1, 3, 4, 5):   # 1, 3, 4: not the metric's dtr count; 5: outside [1, ECC_VIEW_HESSIAN_MAX_CHANNELS]
        with pytest.raises(E.EccError) as e:
            m.evaluate_view_hessian(bad)
        assert e.value.code == 1, (bad, e.value)
    assert _lib.lib().ecc_metric_evaluate_view_hessian(m._h, K, None, None) == 1   # both outputs null
    m.useCorrelation(True)
    canary = np.full((n * K, n * K), -1.0)
    assert _lib.lib().ecc_metric_evaluate_view_hessian(m._h, K, C.c_void_p(canary.ctypes.data), None) == 5   # ECC_ERR_UNSUPPORTED
    assert np.all(canary == -1.0)   # nothing written
    with pytest.raises(E.EccError) as e:
        m.evaluate_view_hessian(K)
    assert e.value.code == 5, e.value
    m.useCorrelation(False)
    assert _u64(m.evaluate())[()] == _u64(want)[()] and np.array_equal(_u64(m.evaluate_view_hessian(K)), _u64(H))
    m.close()
    one = E.MetricRadonIntermediate(gpu_ctx, Ps[:1], dtrs[:2])   # fewer than two views
    with pytest.raises(E.EccError) as e:
        one.evaluate_view_hessian(2)
    assert e.value.code == 1
    one.close()
    # n K above ECC_VIEW_HESSIAN_MAX_DIM with the matrix asked for: 2 049 views of four channels (four tiny intermediates over and
    # over: nothing is evaluated)
    big_n, big_K = 2049, 4
    tiny = [E.RadonIntermediate.from_host(gpu_ctx, np.full((16, 16), 1.0 + k, np.float32), 128, 128) for k in range(4)]
    big = E.MetricRadonIntermediate(gpu_ctx, synthetic.short_scan(big_n, 128, 128, 0.308 * 1024 / 128), [tiny[k % 4] for k in range(big_n * big_K)])
    canary = np.full(4, -1.0)
    assert _lib.lib().ecc_metric_evaluate_view_hessian(big._h, big_K, C.c_void_p(canary.ctypes.data), None) == 5
    assert np.all(canary == -1.0)
    with pytest.raises(E.EccError) as e:
        big.evaluate_view_hessian(big_K)
    assert e.value.code == 5, e.value
    big.close()
    _close(tiny)
    _close(dtrs)
