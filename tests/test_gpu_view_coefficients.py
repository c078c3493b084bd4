"""ecc_metric_evaluate_view_coefficients (csrc/ecc_view_coeff.hip, csrc/view_coeff_kernel.hip): the metric of the corrected
intermediates sum_c a_c,i D_c,i at per-view channel coefficients, and its gradient by all n K of them, over a metric that holds
K * n Radon intermediates channel-major.

The contract (include/ecc_hip.h): (1) with one coefficient 1.0 per view and the rest 0.0, value and pair values have THE BITS of
evaluate(cost) on a metric of the selected intermediates alone; (2) the gradient is 2 / n_pairs times the float64 sum of its
returned pair terms, bit-identical from run to run; (3) value and gradient agree with the CPU oracle on intermediates combined on
the host, to the project's bars; Euler's identity holds on the call's own outputs; conjugate gradients driven by the call as the
Hessian-vector product reach their tolerance; the call changes nothing a later call can see; its argument errors."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEPS = np.array([0.5, 0.5, 0.5, np.deg2rad(0.1), np.deg2rad(0.1), np.deg2rad(0.1)])
KAPPA_FIT_MAX = float(np.float32(0.98))   # csrc/ecc_layout.h: ecc_kappa_fit
# (tests/test_gpu_gram.py) geometry, views and object radius of the two production grids: every loop class occurs
GRID_768 = ("near_opposite", 16, 185.0)
GRID_WIDE = ("angulated", 4, 0.0)


def _scan(gpu_ctx, n, K, S=128, B=48, seed=5, filt=None):
    """tests/test_gpu_gram.py::_scan: K * n DIFFERENT random-normal intermediates (a channel mix-up cannot pass); the host arrays too."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import synthetic
    rng = np.random.default_rng(seed)
    Ps = synthetic.short_scan(n, S, S, 0.308 * 1024 / S)
    kw = {} if filt is None else dict(filter=filt)
    host = [rng.standard_normal((B, B)).astype(np.float32) for _ in range(K * n)]
    dtrs = [E.RadonIntermediate.from_host(gpu_ctx, h, S, S, **kw) for h in host]
    return Ps, dtrs, host


def _catalog_scan(gpu_ctx, name, n, K, n_alpha, n_t, seed=5):
    """n views of tests/geometry_catalog.py and K * n DIFFERENT random-normal intermediates of n_alpha x n_t bins."""
    import epipolarconsistency_amd as E
    import geometry_catalog
    rng = np.random.default_rng(seed)
    Ps, n_u, n_v = geometry_catalog.make(name, n)
    dtrs = [E.RadonIntermediate.from_host(gpu_ctx, rng.standard_normal((n_t, n_alpha), dtype=np.float32), n_u, n_v) for _ in range(K * n)]
    return Ps, dtrs


def _pair_classes(gpu_ctx, Ps, dtrs, radius):
    """The classes of the scan's pairs, from the records of a single-channel metric (tests/test_gpu_gram.py)."""
    import epipolarconsistency_amd as E
    n = len(Ps)
    n_pairs = n * (n - 1) // 2
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs[:n]).setSampling("polynomial")
    m.setObjectRadius(radius)
    recs = m.debug_polynomials(0, n_pairs)
    kmax = m.debug_K01(0, n_pairs)[:, 15]
    m.close()
    ok = np.array([r["poly_ok"] for r in recs])
    free = np.array([r["clamp_free"] for r in recs])
    live = kmax > 0
    return dict(clamp_free=int((ok & free).sum()), clamped=int((ok & ~free).sum()), refused=int((~ok & live).sum()),
                partial=int((ok & (kmax > KAPPA_FIT_MAX)).sum()), above=int((kmax > np.pi / 4).sum()),
                below=int((live & (kmax <= np.pi / 4)).sum()))


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _single(gpu_ctx, Ps, dtrs, configure):
    """evaluate(cost) on a metric of these intermediates alone: (mean, pair values in pair order)"""
    import epipolarconsistency_amd as E
    n = len(Ps)
    m = configure(E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs))
    cost = np.full((n, n), -2.0, np.float32)
    mean = m.evaluate(cost)
    m.close()
    iu = np.triu_indices(n, 1)
    return mean, cost[iu[1], iu[0]].copy()


def _close(dtrs):
    for d in dtrs:
        d.close()


def _configure(setup):
    def configure(m):
        m.setSampling({"auto": "auto", "per_sample": "per_sample", "reference": "reference"}.get(setup, "polynomial"))
        if setup == "dkappa":
            m.setEpipolarPlaneStep(0.004)
        elif setup == "radius":
            m.setObjectRadius(60.0)
        elif setup == "no_record_reuse":
            m.setRecordReuse(False)
        return m
    return configure


def _view_sums(pairs, n, K):
    """float64 numpy sums of the returned terms per (channel, view), and of their magnitudes"""
    iu = np.triu_indices(n, 1)
    S, A = np.zeros((K, n)), np.zeros((K, n))
    for c in range(K):
        h0, h1 = pairs[:, 1 + c].astype(np.float64), pairs[:, 1 + K + c].astype(np.float64)
        np.add.at(S[c], iu[0], h0)
        np.add.at(S[c], iu[1], h1)
        np.add.at(A[c], iu[0], np.abs(h0))
        np.add.at(A[c], iu[1], np.abs(h1))
    return S, A


# ---- 4. bits, one channel, all coefficients 1.0 ----------------------------------------------------------------------------
@pytest.mark.parametrize("n,setup", [(8, "auto"), (10, "auto"), (64, "polynomial"), (64, "per_sample"), (66, "reference"), (258, "polynomial"),
                                     (20, "dkappa"), (20, "radius"), (20, "filter_none"), (20, "no_record_reuse")])
def test_one_channel_of_ones_is_evaluate(gpu_ctx, n, setup):
    """n = 8, 10 under "auto": 28 and 45 pairs, the reference arithmetic with four waves per pair, a sum with a tail; 66 views
    "reference": one wave per pair; 258: 33 153 pairs, the sixteen-slice sum.  1.0f * v is v: value and pair values are evaluate()'s."""
    import epipolarconsistency_amd as E
    Ps, dtrs, _ = _scan(gpu_ctx, n, 1, B=32 if n >= 60 else 48, filt=E.FILTER_NONE if setup == "filter_none" else None)
    configure = _configure(setup)
    m = configure(E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs))
    value, grad, pairs = m.evaluate_view_coefficients(np.ones((1, n)), want_pairs=True)
    m.close()
    mean, vals = _single(gpu_ctx, Ps, dtrs, configure)
    assert pairs.shape == (n * (n - 1) // 2, 3) and pairs.dtype == np.float32 and grad.shape == (1, n) and grad.dtype == np.float64
    assert np.array_equal(_u32(pairs[:, 0]), _u32(vals)), np.max(np.abs(pairs[:, 0] - vals))
    assert _u64(value)[()] == _u64(mean)[()], (value, mean)
    assert np.all(np.isfinite(grad)) and np.all(np.isfinite(pairs))
    _close(dtrs)


# ---- 5. bits, one-hot per view -----------------------------------------------------------------------------------------------
def _check_one_hot(gpu_ctx, Ps, dtrs, K, configure):
    """View i takes channel s_i (a[s_i, i] = 1, the others 0; s_i varies over the views): 0 * v and fmaf(1, v, +-0) are exact, so value
    and pair values have the bits of evaluate(cost) on the metric of the dtrs [D_{s_i, i}].  Any mix-up of channel offset, view index
    or side selects another intermediate."""
    import epipolarconsistency_amd as E
    n = len(Ps)
    s = (np.arange(n) * 2 + np.arange(n) // 3 + 1) % K
    assert len(set(s.tolist())) == K
    a = np.zeros((K, n), np.float32)
    a[s, np.arange(n)] = 1.0
    m = configure(E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs))
    value, grad, pairs = m.evaluate_view_coefficients(a, want_pairs=True)
    m.close()
    mean, vals = _single(gpu_ctx, Ps, [dtrs[int(s[i]) * n + i] for i in range(n)], configure)
    assert np.array_equal(_u32(pairs[:, 0]), _u32(vals)), np.max(np.abs(pairs[:, 0] - vals))
    assert _u64(value)[()] == _u64(mean)[()], (value, mean)
    assert np.all(np.isfinite(grad)) and np.all(np.isfinite(pairs))
    return value, grad, pairs, a


@pytest.mark.parametrize("n,setup", [(8, "auto"), (64, "polynomial"), (64, "per_sample"), (66, "reference"), (258, "polynomial")])
def test_one_hot_coefficients_select_intermediates(gpu_ctx, n, setup):
    K = 3
    Ps, dtrs, _ = _scan(gpu_ctx, n, K, B=32 if n >= 60 else 48)
    _check_one_hot(gpu_ctx, Ps, dtrs, K, _configure(setup))
    _close(dtrs)


@pytest.mark.parametrize("mode,quads", [("polynomial", False), ("per_sample", False), ("polynomial", True)])
def test_one_hot_on_the_default_grid(gpu_ctx, mode, quads):
    """768 x 768 bins (row pitch 6400 bytes): the clamp-free and the clamped polynomial loops of that pitch, the exact loops with and
    without the pi/4 reduction and, with row-quad copies, the row-quad loop in the exact tails -- each reached by at least one pair."""
    name, n, radius = GRID_768
    K = 3
    gpu_ctx.setQuadCopies("on" if quads else "off")
    try:
        Ps, dtrs = _catalog_scan(gpu_ctx, name, n, K, 768, 768)
        cls = _pair_classes(gpu_ctx, Ps, dtrs, radius)
        print("classes of %s, %d views, radius %.0f mm at 768 x 768:" % (name, n, radius), cls)
        if mode == "polynomial":
            assert cls["clamp_free"] > 0 and cls["clamped"] > 0 and cls["refused"] > 0 and cls["partial"] > 0, cls
        else:
            assert cls["above"] > 0 and cls["below"] > 0, cls
        _check_one_hot(gpu_ctx, Ps, dtrs, K, lambda m: m.setSampling(mode).setObjectRadius(radius))
    finally:
        gpu_ctx.setQuadCopies("auto")
    _close(dtrs)


def test_one_hot_on_the_first_wide_offset_grid(gpu_ctx):
    """2621 x 768 bins: the first grid whose copies need integer offsets; 12 slabs of 8 MB."""
    name, n, radius = GRID_WIDE
    K = 3
    Ps, dtrs = _catalog_scan(gpu_ctx, name, n, K, 2621, 768)
    cls = _pair_classes(gpu_ctx, Ps, dtrs, radius)
    print("classes of %s, %d views, radius %.0f mm at 2621 x 768:" % (name, n, radius), cls)
    assert cls["clamp_free"] + cls["clamped"] > 0, cls
    _check_one_hot(gpu_ctx, Ps, dtrs, K, lambda m: m.setSampling("polynomial").setObjectRadius(radius))
    _close(dtrs)


# ---- 6. the gradient is the sum of its terms; 8. Euler's identity ---------------------------------------------------------------
@pytest.mark.parametrize("n,K,setup", [(8, 2, "auto"), (10, 4, "auto"), (64, 3, "polynomial"), (64, 1, "per_sample"), (66, 2, "reference"),
                                       (258, 2, "polynomial"), (1030, 1, "polynomial"), (64, 4, "polynomial"), (20, 2, "filter_none")])
def test_gradient_is_the_sum_of_its_terms(gpu_ctx, n, K, setup):
    """grad = 2 / n_pairs x the float64 sum of the returned h0 / h1 entries per (view, channel), within 4 n 2^-53 sum |terms| (the
    kernel's order of the n - 1 additions is not numpy's); identical bits from two calls; want_pairs changes nothing.  n = 1030: a
    thread of sum_view_terms_kernel adds more than one term (1024 threads).  And Euler's identity on the call's own outputs, f being
    homogeneous of degree two: |sum a grad - 2 value| <= 1e-5 x (2 / N) sum_pairs sum_c (|a_c,i h0_c| + |a_c,j h1_c|).
    (64, 4, "polynomial"): four channels on the main path (10 views under "auto" take the reference arithmetic); "filter_none":
    non-derivative intermediates, the kernels' DERIV = false."""
    import epipolarconsistency_amd as E
    Ps, dtrs, _ = _scan(gpu_ctx, n, K, B=32 if n >= 60 else 48, filt=E.FILTER_NONE if setup == "filter_none" else None)
    a = np.random.default_rng(7).uniform(0.5, 1.5, (K, n)).astype(np.float32)
    m = _configure(setup)(E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs))
    value, grad, pairs = m.evaluate_view_coefficients(a, want_pairs=True)
    value2, grad2, pairs2 = m.evaluate_view_coefficients(a, want_pairs=True)
    value3, grad3 = m.evaluate_view_coefficients(a)
    m.close()
    N = n * (n - 1) // 2
    assert _u64(value)[()] == _u64(value2)[()] == _u64(value3)[()]
    assert np.array_equal(_u64(grad), _u64(grad2)) and np.array_equal(_u64(grad), _u64(grad3)) and np.array_equal(_u32(pairs), _u32(pairs2))
    S, A = _view_sums(pairs, n, K)
    err = np.abs(grad - 2.0 * S / N)
    bound = 4.0 * n * 2.0 ** -53 * (2.0 * A / N)
    assert np.all(err <= bound), (float(np.max(err / bound)),)
    assert np.all(A > 0) and np.all(grad != 0)
    # the value is the mean of its column (sum order aside: float64 additions of N float32 values)
    assert abs(value - pairs[:, 0].astype(np.float64).sum() / N) <= 4.0 * N * 2.0 ** -53 * value
    iu = np.triu_indices(n, 1)
    a64 = a.astype(np.float64)
    mag = sum(np.abs(a64[c, iu[0]] * pairs[:, 1 + c]) + np.abs(a64[c, iu[1]] * pairs[:, 1 + K + c]) for c in range(K)).sum()
    euler = abs(float((a64 * grad).sum()) - 2.0 * value)
    print("n = %d, K = %d, %s: Euler residual %.3g of the terms' magnitudes" % (n, K, setup, euler / (2.0 * mag / N)))
    assert euler <= 1e-5 * 2.0 * mag / N, (euler, 2.0 * mag / N)
    _close(dtrs)


# ---- 7. against the CPU oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K,B,mode", [(8, 2, 48, "auto"), (12, 3, 48, "polynomial"), (20, 2, 32, "polynomial")])
def test_value_and_gradient_against_the_oracle(gpu_ctx, oracle_mod, n, K, B, mode):
    """The dtrs are combined on the host in float64, rounded once to float32 and given to oracle.evaluate_all.  The metric is exactly
    quadratic in a, so d_or[c, i] = (V_or(a + u_ci) - V_or(a - u_ci)) / 2 with a UNIT step is the gradient entry (no small-h
    cancellation).  a ~ U(0.5, 1.5), random-normal dtrs, default_rng(5).  Hard bars: the value within 1e-5 relative; a
    random direction e ~ U(-1, 1): |<grad, e> - (V_or(a + e) - V_or(a - e)) / 2| <= 1e-5 (V_or(a) + V_or(e)); every entry within
    tol x (1 / N) sum over the pairs q with i of (p_or,q(a) + p_or,q(u_ci)), tol the single-pair bar of the mode (1e-6 reference
    arithmetic, 1e-3 polynomial).  Reported, not asserted: the entry errors against those of the existing path for the same quantity
    -- evaluate() on the combined dtrs uploaded with from_host, central difference, same mode.  Measured on one MI355X (DESIGN.md
    4.13): worst entry 0.021 / 2.6e-4 / 9.6e-5 of its bar; ratio of the maximal entry errors to the existing path's 1.03 and 1.16 in
    polynomial mode; under "auto" (reference arithmetic) the existing path reproduces the oracle bit for bit (error 0), so the ratio
    is infinite there at an error of 2.7e-6: the per-sample combination in fp32 against one rounding of the combined dtr."""
    import epipolarconsistency_amd as E
    S = 128
    Ps, dtrs, host = _scan(gpu_ctx, n, K, S=S, B=B, seed=5)
    rng = np.random.default_rng(5)
    a = rng.uniform(0.5, 1.5, (K, n)).astype(np.float32).astype(np.float64)
    e = rng.uniform(-1.0, 1.0, (K, n)).astype(np.float32).astype(np.float64)
    N = n * (n - 1) // 2
    tol = 1e-6 if mode == "auto" else 1e-3   # 28 pairs under "auto": the reference arithmetic

    def combined(coef, only=None):
        views = range(n) if only is None else [only]
        return {i: sum(coef[c, i] * host[c * n + i].astype(np.float64) for c in range(K)).astype(np.float32) for i in views}

    def oracle(coef):
        r = oracle_mod.evaluate_all(Ps, [combined(coef)[i] for i in range(n)], S, S)
        return float(r["mean"]), r["pairs"].astype(np.float64)

    m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling(mode)
    value, grad = m.evaluate_view_coefficients(a)
    m.close()
    V_a, p_a = oracle(a)
    V_e = oracle(e)[0]
    assert abs(value - V_a) <= 1e-5 * V_a, (value, V_a)
    d_e = 0.5 * (oracle(a + e)[0] - oracle(a - e)[0])
    got_e = float((grad * e).sum())
    print("%d views, K = %d, %s: value error %.3g relative; direction error %.3g of V(a) + V(e)"
          % (n, K, mode, abs(value - V_a) / V_a, abs(got_e - d_e) / (V_a + V_e)))
    assert abs(got_e - d_e) <= 1e-5 * (V_a + V_e), (got_e, d_e, V_a, V_e)

    # the existing path: evaluate() on combined dtrs, one view replaced per probe
    base = combined(a)
    base_dev = {i: E.RadonIntermediate.from_host(gpu_ctx, base[i], S, S) for i in range(n)}

    def existing(coef, i):
        d = E.RadonIntermediate.from_host(gpu_ctx, combined(coef, only=i)[i], S, S)
        q = E.MetricRadonIntermediate(gpu_ctx, Ps, [d if k == i else base_dev[k] for k in range(n)]).setSampling(mode)
        v = q.evaluate()
        q.close()
        d.close()
        return v

    iu = np.triu_indices(n, 1)
    err_new, err_old, worst = np.zeros((K, n)), np.zeros((K, n)), 0.0
    for c in range(K):
        for i in range(n):
            u = np.zeros((K, n))
            u[c, i] = 1.0
            d_or = 0.5 * (oracle(a + u)[0] - oracle(a - u)[0])
            V_u, p_u = oracle(u)
            with_i = (iu[0] == i) | (iu[1] == i)
            bar = tol * (p_a[with_i] + p_u[with_i]).sum() / N
            err_new[c, i] = abs(grad[c, i] - d_or)
            err_old[c, i] = abs(0.5 * (existing(a + u, i) - existing(a - u, i)) - d_or)
            worst = max(worst, err_new[c, i] / bar)
            cs = 2.0 * np.sqrt(V_a * V_u)
            assert abs(d_or) >= 0.01 * cs, (c, i, d_or, cs)   # no entry is a near-zero that the bar would hide
    for d in base_dev.values():
        d.close()
    ratio = float(err_new.max() / err_old.max()) if err_old.max() > 0 else float("inf")
    report = ("%d views, K = %d, %s: worst entry error %.3g of its bar; entry errors max %.3g / median %.3g against the existing path's "
              "%.3g / %.3g: ratio of the maxima %.3g" % (n, K, mode, worst, err_new.max(), np.median(err_new), err_old.max(),
                                                         np.median(err_old), ratio))
    print(report)
    assert worst <= 1.0, report
    _close(dtrs)


# ---- 9. Hessian-vector use ---------------------------------------------------------------------------------------------------------
def test_conjugate_gradients_through_the_call(gpu_ctx):
    """n = 8, K = 2, channel 0 fixed at 1 and channel 1 free: minimize_view_coefficients (every operator product one call at the search
    direction) returns coefficients whose free gradient, recomputed by a fresh call, is within 2 tol of the start's; the value is
    below the start's; the fixed coefficients are untouched."""
    import epipolarconsistency_amd as E
    n, K, tol = 8, 2, 1e-4
    Ps, dtrs, _ = _scan(gpu_ctx, n, K)
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs)
    start = np.ones((K, n))
    start[1] = np.random.default_rng(3).uniform(-0.5, 0.5, n)
    free = np.zeros((K, n), bool)
    free[1] = True
    v0, g0 = m.evaluate_view_coefficients(start)
    a, value, its = E.minimize_view_coefficients(m, K, start, free, tol=tol)
    v1, g1 = m.evaluate_view_coefficients(a)
    m.close()
    print("conjugate gradients: %d products, value %.6g -> %.6g, free gradient %.3g -> %.3g" % (its, v0, value, np.abs(g0[1]).max(), np.abs(g1[1]).max()))
    assert 1 <= its <= 2 * n + 10
    assert np.abs(g1[free]).max() <= 2.0 * tol * np.abs(g0[free]).max(), (np.abs(g1[free]).max(), np.abs(g0[free]).max())
    assert value < v0 and _u64(value)[()] == _u64(v1)[()]
    assert np.array_equal(_u64(a[0]), _u64(start[0])) and not np.array_equal(a[1], start[1])
    _close(dtrs)


# ---- 10. leaves the metric as found; errors -------------------------------------------------------------------------------------
def _rigid_probes(P34):
    from epipolarconsistency_amd import geometry as Gm, pack_projection_matrices
    names = ("tx", "ty", "tz", "rx", "ry", "rz")
    return pack_projection_matrices([Gm.compose_transform(P34, Gm.rigid_transform(**{names[k]: s * STEPS[k]}))
                                     for k in range(6) for s in (1.0, -1.0)])


@pytest.mark.parametrize("n", [20, 100])
def test_nothing_else_moved(gpu_ctx, n):
    """evaluate() (with one view moved and back: the kept records of the reuse path are in play at n = 100), evaluate_gram and one
    evaluate_gradient on the same metric object before and after the call: the same bits."""
    import epipolarconsistency_amd as E
    K = 2
    Ps, dtrs, _ = _scan(gpu_ctx, n, K, B=32)
    P0 = E.pack_projection_matrices(Ps)
    view = n // 2
    rows = _rigid_probes(P0[view].reshape(4, 3).T)
    P1 = P0.copy()
    P1[view] = rows[0]
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs)
    a = np.random.default_rng(11).uniform(0.5, 1.5, (K, n))

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
    first = m.evaluate_view_coefficients(a, want_pairs=True)
    after, cost_a = observe(m)
    assert np.array_equal(_u64(before), _u64(after)) and np.array_equal(_u32(cost_b), _u32(cost_a))
    # in the middle of a sequence: matrices moved, then the call, then back
    m.setProjectionMatrices(P1).evaluate()
    moved = m.evaluate_view_coefficients(a)
    assert _u64(m.evaluate())[()] == _u64(before[1])[()]          # the moved matrices are still current
    assert _u64(m.setProjectionMatrices(P0).evaluate())[()] == _u64(before[0])[()]
    again = m.evaluate_view_coefficients(a, want_pairs=True)
    assert _u64(again[0])[()] == _u64(first[0])[()] and np.array_equal(_u64(again[1]), _u64(first[1])) and np.array_equal(_u32(again[2]), _u32(first[2]))
    assert moved[0] != first[0] and not np.array_equal(moved[1], first[1])
    m.close()
    _close(dtrs)


def test_errors(gpu_ctx):
    import epipolarconsistency_amd as E
    n, K = 8, 2
    Ps, dtrs, _ = _scan(gpu_ctx, n, K)
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs)
    want = m.evaluate()
    value, grad = m.evaluate_view_coefficients(np.ones((K, n)))
    for bad in (1, 3, 4, 5):   # 1, 3, 4: not the metric's dtr count; 5: outside [1, ECC_VIEW_COEFF_MAX_CHANNELS]
        with pytest.raises(E.EccError) as e:
            m.evaluate_view_coefficients(np.ones((bad, n)))
        assert e.value.code == 1, (bad, e.value)
    with pytest.raises(ValueError):
        m.evaluate_view_coefficients(np.ones((K, n + 1)))
    m.useCorrelation(True)
    with pytest.raises(E.EccError) as e:
        m.evaluate_view_coefficients(np.ones((K, n)))
    assert e.value.code == 5, e.value   # ECC_ERR_UNSUPPORTED
    m.useCorrelation(False)
    again = m.evaluate_view_coefficients(np.ones((K, n)))
    assert _u64(m.evaluate())[()] == _u64(want)[()] and _u64(again[0])[()] == _u64(value)[()] and np.array_equal(_u64(again[1]), _u64(grad))
    m.close()
    one = E.MetricRadonIntermediate(gpu_ctx, Ps[:1], dtrs[:2])   # fewer than two views
    with pytest.raises(E.EccError) as e:
        one.evaluate_view_coefficients(np.ones((2, 1)))
    assert e.value.code == 1
    one.close()
    _close(dtrs)
