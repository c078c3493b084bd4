"""Pair kernels against the float64 / normative oracle on general C-arm geometries (tests/geometry_catalog.py) at the bin grids
that select the pair kernel's special cases (csrc/ecc_pairs_device.h, pair_accumulate):

  (768, 768)    the default grid
  (512, 790)    the 6400-byte row-pitch loops with non-square bins (pitch4 == 6400 for every n_t in 767 .. 798)
  (1000, 767)   the same, n_t below 768
  (640, 799)    the generic loop, just past that pitch
  (96, 64)      a small ragged grid
  (2620, 768)   the last grid below wide_offsets ((n_alpha + 1) * pitch * 8 >= 2^24, csrc/ecc_evaluate.hip)
  (2621, 768)   the first grid on the wide-offset path

Real data: projections of a sphere phantom made on the device, Radon intermediates from the HIP kernel (bit-exact to the
oracle), read back for the oracle.  Each case prints its class coverage and the pair-value errors next to the oracle's own."""
import numpy as np
import pytest

import geometry_catalog as G
import pose_response

pytestmark = pytest.mark.gpu

N_VIEWS = 40
# (geometry, n_alpha, n_t): every geometry on a 6400-pitch grid, every grid with a geometry other than the short scan
CASES = [("near_opposite", 768, 768), ("mirrored", 768, 768), ("angulated", 512, 790), ("rolled", 512, 790),
         ("scattered", 1000, 767), ("rolled", 1000, 767), ("mirrored", 640, 799), ("near_opposite", 96, 64),
         ("angulated", 2620, 768), ("scattered", 2621, 768)]
KAPPA_FIT_MAX = float(np.float32(0.98))
T_BAD = 1e-4  # the smallest economisation bound measured to fail the per-pair bar (test_negative_control_...)


def _pitch_bytes(n_t):
    return ((n_t + 2) + 31) // 32 * 32 * 8  # csrc/ecc_layout.h: ecc_layout_pitch, paired copies (two floats per bin)


def _wide(n_alpha, n_t):
    return (n_alpha + 1) * _pitch_bytes(n_t) >= 1 << 24


def test_grid_table_selects_the_paths_it_names():
    assert _pitch_bytes(768) == _pitch_bytes(790) == _pitch_bytes(767) == 6400 and _pitch_bytes(799) != 6400
    assert not _wide(2620, 768) and _wide(2621, 768) and not _wide(1000, 767)


def _range_t(n_u, n_v, n_t):
    step_t = np.float32(np.sqrt(float(n_v) * n_v + float(n_u) * n_u) / n_t)  # csrc/ecc_metric_api.hip: m->step_t
    return np.float32(step_t * np.float32(n_t))


def _exact_coords(K, kappa, n_alpha, n_t, range_t):
    """float64 line -> padded texel coordinates with the reference's float constants (as tests/test_gpu_parity.py)."""
    K = K.astype(np.float64)
    c, s = np.cos(kappa), np.sin(kappa)
    l0, l1, l2 = K[0] * c + K[3] * s, K[1] * c + K[4] * s, K[2] * c + K[5] * s
    a = np.arctan2(l1, l0) / np.float64(np.float32(3.14159265359))
    a = np.where(a < 0, a + 2, a)
    d = -(l2 / np.hypot(l0, l1)) / np.float64(range_t) + 0.5
    fold = a > 1
    a = np.where(fold, a - 1, a)
    d = np.where(fold, 1 - d, d)
    return a * n_alpha + 0.5, d * n_t + 0.5, fold


def _turns_90(K, kappa):
    """The line at some kappa turns by 90 degrees or more against kappa = 0 (the fit's validity rule)."""
    K = K.astype(np.float64)
    c, s = np.cos(kappa), np.sin(kappa)
    return bool(((K[0] * c + K[3] * s) * K[0] + (K[1] * c + K[4] * s) * K[1] <= 0).any())


def _poly(ca, cd, sgn, x):
    c0 = ca[0] + (ca[11] if sgn == 1 else ca[12])
    pa = np.polyval(np.concatenate([ca[10:0:-1], [c0]]), sgn * x)
    pd = np.polyval(np.concatenate([cd[10:0:-1], [cd[0] + cd[11]]]), sgn * x)
    return pa, pd


def _check_fits(recs, K01, n_alpha, n_t, range_t, cov):
    """The fitted polynomials of every accepted pair against the exact mapping on a dense kappa grid, both sides; clamp-free
    pairs never reach a clamp; every refused pair explained.  Adds the class counts to cov; returns the worst error (bins) and the
    worst error beyond the float32 storage of the curve's coefficients (sum_k>=1 |c_k| 2^-24: the constant has a low part)."""
    worst = excess = 0.0
    for ij, (r, K) in enumerate(zip(recs, K01)):
        kmax = float(K[15])
        kfit = min(kmax, KAPPA_FIT_MAX)
        if not (kmax > 0):
            continue
        if not r["poly_ok"]:
            kap = np.linspace(-kfit, kfit, 2001)
            sw = any(len(np.unique(_exact_coords(K[8 * v:8 * v + 8], kap, n_alpha, n_t, range_t)[2])) > 1 for v in (0, 1))
            turn = any(_turns_90(K[8 * v:8 * v + 8], kap) for v in (0, 1))
            assert sw or turn or kmax > 1.5, (ij, kmax)
            cov["refused"] += 1
            continue
        cov["deg%d" % r["degree"]] += 1
        cov["partial"] += kfit < kmax
        cov["free" if r["clamp_free"] else "clamped"] += 1
        assert abs(r["x_scale"] * kfit - 1) < 1e-6
        kap = np.linspace(1e-4, kfit, 1025)
        x = kap * r["x_scale"]
        for v in (0, 1):
            Kv = K[8 * v:8 * v + 8]
            ca, cd = r["ca"][v], r["cd"][v]
            assert r["degree"] in (4, 6, 8, 10)
            assert not ca[r["degree"] + 1:11].any() and not cd[r["degree"] + 1:11].any()
            for sgn in (1, -1):
                Ks = Kv.copy().astype(np.float64)
                Ks[0:3] *= sgn  # the -kappa sample is the negated line of plane -kappa
                xa, yd, fold = _exact_coords(Ks, kap, n_alpha, n_t, range_t)
                assert np.all(fold == (r["fold"][v] if sgn == 1 else not r["fold"][v])), (ij, v, sgn)
                pa, pd = _poly(ca, cd, sgn, x)
                ea, ed = np.abs(pa - xa).max(), np.abs(pd - yd).max()
                worst = max(worst, ea, ed)
                excess = max(excess, ea - np.abs(ca[1:11]).sum() * 2.0 ** -24, ed - np.abs(cd[1:11]).sum() * 2.0 ** -24)
                if r["clamp_free"]:  # angle [0.5, n_alpha + 0.5], distance [0.5, n_t] are never reached
                    qa, qd = _poly(ca, cd, sgn, np.linspace(0.0, 1.0, 1025))
                    assert qa.min() > 0.5 + 0.04 and qa.max() < n_alpha + 0.5 - 0.04, (ij, v, sgn, qa.min(), qa.max())
                    assert qd.min() > 0.5 + 0.04 and qd.max() < n_t - 0.04, (ij, v, sgn, qd.min(), qd.max())
    return worst, excess


def test_fitted_polynomials_on_every_geometry(gpu_ctx):
    """Data-independent: the fits of the pair-geometry kernel on every (geometry, grid) case stay within 2e-5 bins of the exact
    float64 mapping between (not only at) the ECC_POLY_CHECKS check points, on top of the float32 rounding of the stored
    coefficients; and the catalogue reaches every class.
    Measured: the stored polynomials are up to 3.4e-5 bins off at the end of the range (x = 1) from 512 bins on -- the float32
    coefficients of a distance curve sum to ~320 bins, so their rounding alone is worth ~1.9e-5 bins there, the same size as
    the fp32 evaluation's own rounding of a coordinate near 768 (half an ulp, 3e-5); the fit itself is within 1.5e-5 bins
    everywhere (tests/test_gpu_parity.py holds the plain 2e-5 at 384 bins, where the coefficients are half as large)."""
    import epipolarconsistency_amd as E
    from collections import Counter
    total = Counter()
    free_6400_not_768 = 0
    for name, n_alpha, n_t in CASES:
        Ps, n_u, n_v = G.make(name, N_VIEWS)
        d = E.RadonIntermediate.from_host(gpu_ctx, np.zeros((n_t, n_alpha), np.float32), n_u, n_v)
        m = E.MetricRadonIntermediate(gpu_ctx, Ps, [d] * N_VIEWS)
        n_pairs = N_VIEWS * (N_VIEWS - 1) // 2
        # the automatic object radius, and small ones: short kappa ranges, where economisation lowers the degree to 6 and 4
        for radius in (0.0, 20.0, 5.0):
            m.setObjectRadius(radius)
            recs = m.debug_polynomials(0, n_pairs)
            K01 = m.debug_K01(0, n_pairs)
            cov = Counter()
            worst, excess = _check_fits(recs, K01, n_alpha, n_t, _range_t(n_u, n_v, n_t), cov)
            print("fits %-13s (%4d, %3d) radius %4.1f: worst %.2e bins, %.2e beyond coefficient rounding, %s"
                  % (name, n_alpha, n_t, radius, worst, excess, dict(sorted(cov.items()))))
            assert excess < 2e-5 and worst < 5e-5, (name, n_alpha, n_t, radius, worst, excess)
            total.update(cov)
            if _pitch_bytes(n_t) == 6400 and n_t != 768 and not _wide(n_alpha, n_t):
                free_6400_not_768 += cov["free"]
        m.close()
        d.close()
    print("fits, all cases:", dict(sorted(total.items())), "clamp-free on 6400-pitch n_t != 768:", free_6400_not_768)
    for k in ("deg4", "deg6", "deg8", "deg10", "free", "clamped", "refused", "partial"):
        assert total[k] > 0, (k, dict(total))
    assert free_6400_not_768 > 0


# ---- pair values against the oracle -------------------------------------------------------------------------------------
def _make_case(gpu_ctx, name, n_alpha, n_t, n=N_VIEWS):
    """Ps, n_u, n_v, device dtrs (aliasing the returned slabs) and their read-back copies."""
    Ps, n_u, n_v = G.make(name, n)
    slabs, dtrs, host = pose_response.device_case(gpu_ctx, Ps, n_u, n_v, n_alpha, n_t, G.phantom())
    return Ps, n_u, n_v, slabs, dtrs, host


class _Oracle:
    """Normative (variant 0) and float64-geometry (variant 1) oracle values of one problem, and the bars of the pair values."""

    def __init__(self, oracle_mod, Ps, host, n_u, n_v, mask, idx=None, want_K01=False):
        if idx is None:
            self.ref = oracle_mod.evaluate_all(Ps, host, n_u, n_v, want_K01=want_K01)
        else:
            self.ref = oracle_mod.evaluate_pairs(Ps, host, n_u, n_v, idx)
        oracle_mod.set_variant(1)
        try:
            r64 = oracle_mod.evaluate_all(Ps, host, n_u, n_v) if idx is None else oracle_mod.evaluate_pairs(Ps, host, n_u, n_v, idx)
        finally:
            oracle_mod.set_variant(0)
        self.mask = mask
        self.p0 = np.asarray(self.ref["pairs"], np.float64)[mask]
        self.p64 = np.asarray(r64["pairs"], np.float64)[mask]
        self.scale = np.maximum(np.abs(self.p64), 1e-3 * np.abs(self.p64).max())
        noise = np.abs(self.p0 - self.p64) / self.scale
        self.noise = (np.percentile(noise, 50), np.percentile(noise, 99), noise.max())
        self.mean = self.p0.mean()

    def errors(self, vals):
        e = np.abs(np.asarray(vals, np.float64)[self.mask] - self.p64) / self.scale
        return np.percentile(e, 50), np.percentile(e, 99), e.max()

    def bar_ok(self, vals, q=1.1):
        p50, p99, mx = self.errors(vals)
        return p50 <= q * self.noise[0] and p99 <= q * self.noise[1] and mx <= 2 * self.noise[2]

    def check(self, vals, what, q=1.1):
        """The per-pair bar and the mean within 1e-5 of the normative oracle (well-posed pairs)."""
        got = np.asarray(vals, np.float64)[self.mask]
        assert np.isfinite(got).all(), what
        rel_mean = abs(got.mean() - self.mean) / abs(self.mean)
        p50, p99, mx = self.errors(vals)
        print("  %-28s ours p50 %.2e p99 %.2e max %.2e | oracle p50 %.2e p99 %.2e max %.2e | mean rel %.1e"
              % (what, p50, p99, mx, self.noise[0], self.noise[1], self.noise[2], rel_mean))
        assert rel_mean <= 1e-5, (what, rel_mean)
        assert self.bar_ok(vals, q), (what, (p50, p99, mx), self.noise)


@pytest.mark.parametrize("name,n_alpha,n_t", CASES)
def test_pair_values_against_the_oracle(gpu_ctx, oracle_mod, name, n_alpha, n_t):
    """K01 at rtol 3e-7; reference mode: every pair within 1e-6, mean within 1e-7; polynomial and per-sample modes: mean within
    1e-5, per-pair error against the float64-geometry oracle no worse than the normative oracle's own (p50 / p99 1.1x, max 2x);
    the cost image equals the pair values, untouched entries kept.
    The per-sample path is held to 1.25x at p50 / p99: its own fp32 line mapping measured up to 1.16x the oracle's p50 (mirrored,
    768 x 768: 9.6e-7 against 8.2e-7) and 1.11x (scattered, 2621 x 768); the polynomial path meets 1.1x on every case."""
    import epipolarconsistency_amd as E
    Ps, n_u, n_v, slabs, dtrs, host = _make_case(gpu_ctx, name, n_alpha, n_t)
    n = len(Ps)
    n_pairs = n * (n - 1) // 2
    mask = G.well_posed(Ps)
    orc = _Oracle(oracle_mod, Ps, host, n_u, n_v, mask, want_K01=True)
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs)
    K01 = m.debug_K01(0, n_pairs)
    np.testing.assert_allclose(K01[mask], orc.ref["K01s"][mask], rtol=3e-7, atol=1e-12)
    recs = m.setSampling("polynomial").debug_polynomials(0, n_pairs)
    degs = np.array([r["degree"] for r in recs])
    free = np.array([r["clamp_free"] for r in recs])
    print("case %s (%d, %d): %d pairs, degrees %s, clamp-free %d, refused %d, kappa_max > pi/4: %d"
          % (name, n_alpha, n_t, n_pairs, {int(k): int((degs == k).sum()) for k in (4, 6, 8, 10)}, free.sum(), (degs == 0).sum(),
             (K01[:, 15] > np.pi / 4).sum()))
    # reference arithmetic: every pair
    total_r, vals_r = m.setSampling("reference").evaluate_range(0, n_pairs, want_pairs=True)
    np.testing.assert_allclose(vals_r[mask], orc.ref["pairs"][mask], rtol=1e-6)
    assert abs(vals_r[mask].astype(np.float64).mean() - orc.mean) <= 1e-7 * abs(orc.mean)
    for mode in ("polynomial", "per_sample"):
        m.setSampling(mode)
        total, vals = m.evaluate_range(0, n_pairs, want_pairs=True)
        orc.check(vals, mode, 1.1 if mode == "polynomial" else 1.25)
        cost = np.full((n, n), 7.0, np.float32)
        mean = m.evaluate(cost)
        iu = np.triu_indices(n, 1)
        assert np.array_equal(cost[iu[1], iu[0]], vals) and (cost[iu] == 7.0).all() and (np.diag(cost) == 7.0).all()
        assert mean == total / n_pairs
    m.close()
    for d in dtrs:
        d.close()
    del slabs


def test_negative_control_coarse_economisation_fails_the_bar(gpu_ctx, oracle_mod):
    """The per-pair bar above is sharp enough to catch a subtly worse polynomial path: with the economisation bound raised from
    2e-8 bins (ECC_POLY_ECONOMISE_TOL_BINS) to T_BAD = 1e-4 bins the fitted coordinates move by up to 1e-4 bins and the bar fails.
    Measured on (angulated, 512 x 790): p99 9.1e-5 against the oracle's 7.1e-5 (p50 1.8e-5 / 1.6e-5) at 1e-4; 3e-5 still passes
    (p99 6.8e-5), 2e-8 gives p99 6.6e-5."""
    import epipolarconsistency_amd as E
    Ps, n_u, n_v, slabs, dtrs, host = _make_case(gpu_ctx, "angulated", 512, 790)
    n_pairs = len(Ps) * (len(Ps) - 1) // 2
    orc = _Oracle(oracle_mod, Ps, host, n_u, n_v, G.well_posed(Ps))
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling("polynomial")
    verdict = {}
    for tol in (2e-8, 3e-5, T_BAD, 1e-3):
        m.debugSetPolyTolerance(tol)
        _, vals = m.evaluate_range(0, n_pairs, want_pairs=True)
        degs = np.array([r["degree"] for r in m.debug_polynomials(0, n_pairs)])
        verdict[tol] = orc.bar_ok(vals)
        print("  tol %.0e: p50 %.2e p99 %.2e max %.2e (oracle %.2e %.2e %.2e), mean degree %.2f, bar %s"
              % ((tol,) + orc.errors(vals) + orc.noise + (degs[degs > 0].mean(), verdict[tol])))
    assert verdict[2e-8] and not verdict[T_BAD] and not verdict[1e-3]
    m.close()
    for d in dtrs:
        d.close()
    del slabs


# ---- launch forms, pose batch and incremental mode on the angulated orbit ------------------------------------------------
def test_launch_forms_on_the_angulated_orbit(gpu_ctx, oracle_mod):
    """258 views at (512, 790): 33 153 pairs (the sixteen-slice sum, the beside-one-wave refit).  All-pairs with a cost image,
    ranges on both sides of every launch threshold, shuffled / repeated / swapped index lists, setSmallEval(False), quad copies
    on, and three steps of moved views with record reuse on and off: identical bits wherever the library promises them, and
    every form's own values within the oracle bar."""
    import epipolarconsistency_amd as E
    n_alpha, n_t = 512, 790
    Ps, n_u, n_v, slabs, dtrs, host = _make_case(gpu_ctx, "angulated", n_alpha, n_t, n=258)
    n = len(Ps)
    n_pairs = n * (n - 1) // 2
    assert n_pairs > 32768
    mask = G.well_posed(Ps)
    orc = _Oracle(oracle_mod, Ps, host, n_u, n_v, mask)
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling("polynomial")
    cost = np.full((n, n), -1.0, np.float32)
    mean = m.evaluate(cost)
    total, vals = m.evaluate_range(0, n_pairs, want_pairs=True)
    assert mean == total / n_pairs
    iu = np.triu_indices(n, 1)
    assert np.array_equal(cost[iu[1], iu[0]], vals) and (cost[iu] == -1.0).all()
    orc.check(vals, "all pairs")
    # ranges: counts on both sides of the launch thresholds
    rng = np.random.default_rng(11)
    for c0 in (192, 512, 768, 2048, 4096, 8192, 16384, 32768):
        for count in (c0 - 1, c0, c0 + 1):
            first = int(rng.integers(0, n_pairs - count + 1))
            s, v = m.evaluate_range(first, count, want_pairs=True)
            assert np.array_equal(v, vals[first:first + count]), (first, count)
            assert abs(s - vals[first:first + count].astype(np.float64).sum()) <= 1e-9 * abs(s)
    # index lists: shuffled and repeated pairs take the all-pairs bits; swapped pairs are pairs of their own (oracle)
    ij = G.pair_indices(n)
    sel = rng.permutation(n_pairs)[:5000]
    sel = np.concatenate([sel, sel[:700]])
    idx = np.stack([ij[sel, 0], ij[sel, 1], ij[sel, 0], ij[sel, 1]], 1).astype(np.int32)
    out = np.empty(len(idx), np.float32)
    m.evaluate(idx, out)
    assert np.array_equal(out, vals[sel])
    sw = np.ascontiguousarray(idx[:3000][:, [1, 0, 3, 2]])
    out_sw = np.empty(len(sw), np.float32)
    m.evaluate(sw, out_sw)
    orc_sw = _Oracle(oracle_mod, Ps, host, n_u, n_v, mask[sel[:3000]], idx=sw)
    orc_sw.check(out_sw, "swapped list")
    # setSmallEval(False): the multi-launch path for small evaluations
    m.setSmallEval(False)
    for first, count in ((5, 150), (1000, 192), (30000, 7)):
        s, v = m.evaluate_range(first, count, want_pairs=True)
        assert np.array_equal(v, vals[first:first + count]), (first, count)
    m.setSmallEval(True)
    # quad copies on
    gpu_ctx.setQuadCopies("on")
    try:
        q = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling("polynomial")
    finally:
        gpu_ctx.setQuadCopies("auto")
    _, vq = q.evaluate_range(0, n_pairs, want_pairs=True)
    assert np.array_equal(vq, vals)
    q.close()
    # three steps of moved views, record reuse on and off: the same bits, each step at the oracle's mean
    on = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling("polynomial").setRecordReuse(True, always=True)
    off = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling("polynomial").setRecordReuse(False)
    on.evaluate(), off.evaluate()
    P = [np.array(p) for p in Ps]
    for step, views in enumerate(([7], [130, 131], [0, 200, 257])):
        for v in views:
            P[v] = P[v] @ E.geometry.rigid_transform(tx=0.4 * (step + 1), ry=1e-3, rz=-2e-3 * (step + 1))
        a = on.setProjectionMatrices(P).evaluate()
        _, va = on.evaluate_range(0, n_pairs, want_pairs=True)
        b = off.setProjectionMatrices(P).evaluate()
        assert a == b, (step, a, b)
        _, vb = off.evaluate_range(0, n_pairs, want_pairs=True)
        assert np.array_equal(va, vb)
        want = oracle_mod.evaluate_all(P, host, n_u, n_v)["mean"]
        assert abs(a - want) <= 1e-5 * abs(want), (step, a, want)
    on.close(); off.close(); m.close()
    for d in dtrs:
        d.close()
    del slabs


def test_pose_batch_and_incremental_against_the_oracle(gpu_ctx, oracle_mod):
    """130 views of the angulated orbit at (512, 790): evaluate_pose_deltas for the 12 central-difference 6-DoF poses of one view
    and a pose that moves two, evaluate_poses strided, and five incremental single-view moves -- each mean against the oracle
    evaluated on that pose's full matrices (1e-5)."""
    import epipolarconsistency_amd as E
    Ps, n_u, n_v, slabs, dtrs, host = _make_case(gpu_ctx, "angulated", 512, 790, n=130)
    n = len(Ps)
    P0 = E.pack_projection_matrices(Ps)
    v = 65
    steps = [dict(tx=0.5), dict(ty=0.5), dict(tz=0.5), dict(rx=1e-3), dict(ry=1e-3), dict(rz=1e-3)]
    poses, views, rows = [], [], []
    for st in steps:
        for sgn in (1, -1):
            T = E.geometry.rigid_transform(**{k: sgn * x for k, x in st.items()})
            P = [np.array(p) for p in Ps]
            P[v] = P[v] @ T
            poses.append(P)
            views.append([v])
            rows.append([P[v]])
    P = [np.array(p) for p in Ps]
    P[3] = P[3] @ E.geometry.rigid_transform(tx=-0.7, rz=2e-3)
    P[100] = P[100] @ E.geometry.rigid_transform(ty=0.3, rx=-1e-3)
    poses.append(P)
    views.append([3, 100])
    rows.append([P[3], P[100]])
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling("polynomial")
    base = m.evaluate()
    got = m.evaluate_pose_deltas(views, rows)
    want = np.array([oracle_mod.evaluate_all(P, host, n_u, n_v)["mean"] for P in poses])
    rel = np.abs(got - want) / np.abs(want)
    print("pose deltas: max rel %.2e over %d poses" % (rel.max(), len(want)))
    assert rel.max() <= 1e-5, rel
    assert m.evaluate() == base  # the current matrices stay
    # the strided form: poses 1, 4, 7, ... as full matrices; the others' means stay 0
    packed = np.stack([E.pack_projection_matrices(P) for P in poses])
    strided = m.evaluate_poses(packed, first=1, stride=3)
    mine = np.arange(1, len(poses), 3)
    assert np.array_equal(strided[mine], got[mine]) and not strided[np.setdiff1d(np.arange(len(poses)), mine)].any()
    # incremental mode: five single-view moves
    inc = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling("polynomial").setIncremental(True)
    inc.evaluate()
    P = [np.array(p) for p in Ps]
    for k, view in enumerate((0, 17, 64, 65, 129)):
        P[view] = P[view] @ E.geometry.rigid_transform(tx=0.3 * (k + 1), rz=1e-3, ry=-5e-4 * k)
        a = inc.setProjectionMatrices(P).evaluate()
        # (view 0 sets the automatic object radius: moving it changes every pair)
        assert inc.last_evaluated_pairs() == (n * (n - 1) // 2 if view == 0 else n - 1)
        w = oracle_mod.evaluate_all(P, host, n_u, n_v)["mean"]
        assert abs(a - w) <= 1e-5 * abs(w), (k, view, a, w)
        assert a == m.setProjectionMatrices(P).evaluate()  # bit-identical to a full evaluation
    inc.close(); m.close()
    for d in dtrs:
        d.close()
    del slabs
