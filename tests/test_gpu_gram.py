"""ecc_metric_evaluate_gram (csrc/ecc_gram.hip, csrc/gram_kernel.hip): the metric of corrected images sum_c a_c I_c,i as the
quadratic form a^T G a of the channel coefficients, over a metric that holds K * n Radon intermediates channel-major.

The contract (include/ecc_hip.h): (1) the diagonal entries, per pair and in the mean, have THE BITS of evaluate(cost) on a metric of
that channel's intermediates alone; (2) G is symmetric by construction; (3) the off-diagonal entries agree with the polarisation of
the CPU oracle's pair values to the comparator's own floor, which is measured here; the form predicts the metric of intermediates
computed from the combined images; the call changes nothing a later call can see; its argument errors."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEPS = np.array([0.5, 0.5, 0.5, np.deg2rad(0.1), np.deg2rad(0.1), np.deg2rad(0.1)])


def _scan(gpu_ctx, n, K, S=128, B=48, seed=5, filt=None):
    """tests/test_gpu_gradient.py::_scan with K * n DIFFERENT random-normal intermediates (a channel mix-up cannot pass)."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import synthetic
    rng = np.random.default_rng(seed)
    Ps = synthetic.short_scan(n, S, S, 0.308 * 1024 / S)
    kw = {} if filt is None else dict(filter=filt)
    dtrs = [E.RadonIntermediate.from_host(gpu_ctx, rng.standard_normal((B, B)).astype(np.float32), S, S, **kw) for _ in range(K * n)]
    return Ps, dtrs


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _entry(K, c, d):
    """column of entry (c, d), c <= d, in the order (0,0), (0,1) .. (0,K-1), (1,1) .. (K-1,K-1)"""
    return c * K - c * (c - 1) // 2 + (d - c)


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


def _check_diagonal(gpu_ctx, Ps, dtrs, K, configure):
    import epipolarconsistency_amd as E
    n = len(Ps)
    m = configure(E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs))
    G, pairs = m.evaluate_gram(K, want_pairs=True)
    G2 = m.evaluate_gram(K)   # without the pair entries: the same matrix
    m.close()
    assert G.shape == (K, K) and G.dtype == np.float64 and pairs.shape == (n * (n - 1) // 2, K * (K + 1) // 2) and pairs.dtype == np.float32
    assert np.array_equal(_u64(G), _u64(G.T)) and np.array_equal(_u64(G), _u64(G2))
    assert np.all(np.isfinite(G)) and np.all(np.isfinite(pairs))
    for c in range(K):
        mean, vals = _single(gpu_ctx, Ps, dtrs[c * n:(c + 1) * n], configure)
        assert np.array_equal(_u32(pairs[:, _entry(K, c, c)]), _u32(vals)), (c, np.max(np.abs(pairs[:, _entry(K, c, c)] - vals)))
        assert _u64(G[c, c])[()] == _u64(mean)[()], (c, G[c, c], mean)
    # the channels are different arrays: different diagonal entries, off-diagonal entries that are not copies of them
    for c in range(K):
        for d in range(c + 1, K):
            assert G[c, c] != G[d, d] and G[c, d] != G[c, c] and abs(G[c, d]) <= np.sqrt(G[c, c] * G[d, d])
            assert np.all(np.abs(pairs[:, _entry(K, c, d)].astype(np.float64))
                          <= np.sqrt(pairs[:, _entry(K, c, c)].astype(np.float64) * pairs[:, _entry(K, d, d)]) * (1 + 1e-6))
    return G, pairs


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("n,mode", [(8, "auto"), (8, "polynomial"), (64, "polynomial"), (64, "per_sample"), (258, "polynomial")])
def test_diagonal_entries_have_the_bits_of_evaluate(gpu_ctx, n, mode, K):
    """n = 8 under "auto": 28 pairs, the reference arithmetic (four waves per pair); 64: 2 016 pairs; 258: 33 153 pairs, the
    sixteen-slice sum."""
    Ps, dtrs = _scan(gpu_ctx, n, K, B=32 if n > 100 else 48)
    _check_diagonal(gpu_ctx, Ps, dtrs, K, lambda m: m.setSampling(mode))
    for d in dtrs:
        d.close()


@pytest.mark.parametrize("setup", ["dkappa", "radius", "filter_none", "no_record_reuse", "reference_one_wave", "reference_20"])
def test_diagonal_bits_in_other_states(gpu_ctx, setup):
    """A user dkappa, a fixed radius, non-derivative intermediates, record reuse off; the reference arithmetic with one wave per pair
    (more than 2 048 pairs) and with four."""
    import epipolarconsistency_amd as E
    K = 3
    n = 66 if setup == "reference_one_wave" else 20
    Ps, dtrs = _scan(gpu_ctx, n, K, B=32 if n > 60 else 48, filt=E.FILTER_NONE if setup == "filter_none" else None)

    def configure(m):
        m.setSampling("reference" if setup.startswith("reference") else "polynomial")
        if setup == "dkappa":
            m.setEpipolarPlaneStep(0.004)
        elif setup == "radius":
            m.setObjectRadius(60.0)
        elif setup == "no_record_reuse":
            m.setRecordReuse(False)
        return m
    _check_diagonal(gpu_ctx, Ps, dtrs, K, configure)
    for d in dtrs:
        d.close()


# ---- the loops of the production grids (csrc/ecc_pairs_device.h: poly_loop_dispatch, exact_loop_dispatch) --------------------
KAPPA_FIT_MAX = float(np.float32(0.98))   # csrc/ecc_layout.h: ecc_kappa_fit


def _catalog_scan(gpu_ctx, name, n, K, n_alpha, n_t, seed=5):
    """n views of tests/geometry_catalog.py and K * n DIFFERENT random-normal intermediates of n_alpha x n_t bins."""
    import epipolarconsistency_amd as E
    import geometry_catalog
    rng = np.random.default_rng(seed)
    Ps, n_u, n_v = geometry_catalog.make(name, n)
    dtrs = [E.RadonIntermediate.from_host(gpu_ctx, rng.standard_normal((n_t, n_alpha), dtype=np.float32), n_u, n_v) for _ in range(K * n)]
    return Ps, dtrs


def _pair_classes(gpu_ctx, Ps, dtrs, radius):
    """The classes of the scan's pairs, from the records of a single-channel metric (as tests/test_gpu_geometry_parity.py reads them)."""
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


# Geometry, views and object radius (mm; 0: automatic) of the two grids, chosen so that the asserted classes occur with room to
# spare.  16 views of the near-opposite orbit (source at 740 mm) and a 185-mm object: neighbouring views have short ranges in the
# middle of the detector (clamp-free); most others reach the detector's edge (clamped); views seven steps apart (157.5 deg) have their
# baseline 144 mm from the centre, inside the object, so kappa_max = pi/2 and the fit ends at 0.98 before the range does (partial);
# views eight steps apart face each other, the baseline passes within millimetres of the centre and no fit is accepted (refused).
GRID_768 = ("near_opposite", 16, 185.0)
GRID_WIDE = ("angulated", 4, 0.0)


@pytest.mark.parametrize("mode,quads", [("polynomial", False), ("per_sample", False), ("polynomial", True)])
def test_diagonal_bits_on_the_default_grid(gpu_ctx, mode, quads):
    """768 x 768 bins (row pitch 6400 bytes): the clamp-free and the clamped polynomial loops of that pitch, the exact loops with and
    without the pi/4 reduction and, with row-quad copies, the row-quad loop in the exact tails -- each reached by at least one pair."""
    name, n, radius = GRID_768
    K = 2
    gpu_ctx.setQuadCopies("on" if quads else "off")
    try:
        Ps, dtrs = _catalog_scan(gpu_ctx, name, n, K, 768, 768)
        cls = _pair_classes(gpu_ctx, Ps, dtrs, radius)
        print("classes of %s, %d views, radius %.0f mm at 768 x 768:" % (name, n, radius), cls)
        if mode == "polynomial":
            assert cls["clamp_free"] > 0 and cls["clamped"] > 0 and cls["refused"] > 0 and cls["partial"] > 0, cls
        else:
            assert cls["above"] > 0 and cls["below"] > 0, cls
        _check_diagonal(gpu_ctx, Ps, dtrs, K, lambda m: m.setSampling(mode).setObjectRadius(radius))
    finally:
        gpu_ctx.setQuadCopies("auto")
    for d in dtrs:
        d.close()


@pytest.mark.parametrize("mode", ["polynomial", "per_sample"])
def test_diagonal_bits_on_the_first_wide_offset_grid(gpu_ctx, mode):
    """2621 x 768 bins: the first grid whose copies need integer offsets (tests/test_gpu_geometry_parity.py); 8 slabs of 8 MB."""
    name, n, radius = GRID_WIDE
    K = 2
    Ps, dtrs = _catalog_scan(gpu_ctx, name, n, K, 2621, 768)
    cls = _pair_classes(gpu_ctx, Ps, dtrs, radius)
    print("classes of %s, %d views, radius %.0f mm at 2621 x 768:" % (name, n, radius), cls)
    assert cls["clamp_free"] + cls["clamped"] > 0, cls
    _check_diagonal(gpu_ctx, Ps, dtrs, K, lambda m: m.setSampling(mode).setObjectRadius(radius))
    for d in dtrs:
        d.close()


def test_one_channel_is_evaluate(gpu_ctx):
    import epipolarconsistency_amd as E
    for n, mode in ((8, "auto"), (64, "polynomial")):
        Ps, dtrs = _scan(gpu_ctx, n, 1)
        m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling(mode)
        G, pairs = m.evaluate_gram(1, want_pairs=True)
        m.close()
        mean, vals = _single(gpu_ctx, Ps, dtrs, lambda q: q.setSampling(mode))
        assert G.shape == (1, 1) and _u64(G[0, 0])[()] == _u64(mean)[()]
        assert np.array_equal(_u32(pairs[:, 0]), _u32(vals))
        for d in dtrs:
            d.close()


def _channel_images(p):
    """p, p^2 / max, p^3 / max^2, sqrt(p max): channel images of a beam-hardening polynomial and a root"""
    p = np.asarray(p, np.float32)
    mx = np.float32(p.max())
    return [p, p * p / mx, p * p * p / (mx * mx), np.sqrt(np.maximum(p, 0) * mx)]


def test_off_diagonal_entries_against_the_oracle(gpu_ctx, oracle_mod, small_scan):
    """REFERENCE sampling, the 8-view small_scan with real channel intermediates (oracle.radon of p, p^2/max, p^3/max^2, sqrt(p max),
    identity post-process).  Comparator per pair and c < d: g1 = (E(c+d) - E(c) - E(d)) / 2 from oracle.evaluate_all's pair values
    (the sums of intermediates formed in float32 on the host).  Its own floor is MEASURED here as max |g1 - g2| / sqrt(g_cc g_dd),
    g2 = (E(c+d) - E(c-d)) / 4 (on the CPU oracle: 6.9e-7 per pair).  Required: |g_gpu - g1| <= (1e-6 + floor) sqrt(g_cc g_dd) per
    pair -- 1e-6 is what tests/test_gpu_sampling_modes.py holds REFERENCE-mode pair values to -- and |G_gpu - G1| <= 1e-5
    sqrt(G_cc G_dd) on the means, in POLYNOMIAL mode as well (the project's parity target)."""
    import epipolarconsistency_amd as E
    s = small_scan
    n, K = 8, 4
    chans = list(zip(*[_channel_images(im) for im in s["imgs"]]))   # chans[c][i]
    D = [[oracle_mod.radon(chans[c][i], s["n_alpha"], s["n_t"]) for i in range(n)] for c in range(K)]

    def Eo(dtrs):
        r = oracle_mod.evaluate_all(s["Ps"], dtrs, s["n_u"], s["n_v"])
        return r["pairs"].astype(np.float64), float(r["mean"])
    Ec = [Eo(D[c]) for c in range(K)]
    g1, g2, G1 = {}, {}, {}
    for c in range(K):
        for d in range(c + 1, K):
            plus = Eo([(D[c][i] + D[d][i]).astype(np.float32) for i in range(n)])
            minus = Eo([(D[c][i] - D[d][i]).astype(np.float32) for i in range(n)])
            g1[c, d] = 0.5 * (plus[0] - Ec[c][0] - Ec[d][0])
            g2[c, d] = 0.25 * (plus[0] - minus[0])
            G1[c, d] = 0.5 * (plus[1] - Ec[c][1] - Ec[d][1])
    dev = [E.RadonIntermediate.from_host(gpu_ctx, D[c][i], s["n_u"], s["n_v"]) for c in range(K) for i in range(n)]
    m = E.MetricRadonIntermediate(gpu_ctx, s["Ps"], dev)
    G_ref, pairs = m.setSampling("reference").evaluate_gram(K, want_pairs=True)
    G_poly = m.setSampling("polynomial").evaluate_gram(K)
    m.close()
    corr = []
    for c in range(K):
        for d in range(c + 1, K):
            scale = np.sqrt(Ec[c][0] * Ec[d][0])
            floor = float(np.max(np.abs(g1[c, d] - g2[c, d]) / scale))
            err = np.abs(pairs[:, _entry(K, c, d)].astype(np.float64) - g1[c, d]) / scale
            print("entry (%d,%d): comparator floor %.3g, worst pair error %.3g of sqrt(g_cc g_dd)" % (c, d, floor, err.max()))
            assert np.all(err <= 1e-6 + floor), (c, d, float(err.max()), floor)
            mscale = np.sqrt(Ec[c][1] * Ec[d][1])
            for name, G in (("reference", G_ref), ("polynomial", G_poly)):
                merr = abs(G[c, d] - G1[c, d]) / mscale
                print("entry (%d,%d) %s: mean error %.3g of sqrt(G_cc G_dd), correlation %.3f" % (c, d, name, merr, G1[c, d] / mscale))
                assert merr <= 1e-5, (c, d, name, merr)
            corr.append(G1[c, d] / mscale)
    # the cases are sharp: weak and strong cross-correlations of both signs, so a sign or an index error shows
    assert min(np.abs(corr)) < 0.2 and max(np.abs(corr)) > 0.9 and min(corr) < 0 < max(corr), corr
    for c in range(K):   # and the diagonal against the oracle, as everywhere
        assert abs(G_ref[c, c] - Ec[c][1]) <= 1e-6 * Ec[c][1] and abs(G_poly[c, c] - Ec[c][1]) <= 1e-5 * Ec[c][1]
    for d in dev:
        d.close()


def test_the_form_predicts_the_metric_of_combined_images(gpu_ctx):
    """64 views of 256^2, 192^2 bins, channel images p, p^2/max, p^3/max^2, intermediates by compute_batch with POST_IDENTITY: for
    three coefficient vectors (one of them gram_minimizer's) the mean of evaluate() on intermediates computed from the COMBINED
    IMAGES agrees with gram_value(G, a) to 1e-5 of sum |a_c| |a_d| |G_cd|, and the minimiser's value is below the value at e_0."""
    import torch
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import synthetic
    n, S, B, K = 64, 256, 192, 3
    Ps = synthetic.short_scan(n, S, S, 0.308 * 1024 / S)
    dev = torch.device("cuda", gpu_ctx.device)
    p = synthetic.projections_torch(Ps, S, S, synthetic.sphere_phantom(extent_mm=30, rmin=8, rmax=25), dev)
    mx = p.max()
    chans = [p, p * p / mx, p * p * p / (mx * mx)]
    dtrs = []
    for I in chans:
        dtrs += E.RadonIntermediate.compute_batch(gpu_ctx, I.contiguous(), B, B, post_process=E.POST_IDENTITY)
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs)
    G = m.evaluate_gram(K)
    m.close()
    a_min, v_min = E.gram_minimizer(G, fixed=0, value=1.0)
    for a in (np.array([1.0, 0.0, 0.0]), np.array([1.0, -0.3, 0.2]), a_min):
        comb = sum(float(a[c]) * chans[c] for c in range(K)).to(torch.float32).contiguous()
        dc = E.RadonIntermediate.compute_batch(gpu_ctx, comb, B, B, post_process=E.POST_IDENTITY)
        mc = E.MetricRadonIntermediate(gpu_ctx, Ps, dc)
        got = mc.evaluate()
        mc.close()
        for d in dc:
            d.close()
        want = E.gram_value(G, a)
        scale = float(np.abs(a) @ np.abs(G) @ np.abs(a))
        print("a = %s: evaluate() %.9g, form %.9g, difference %.3g of sum |a||a||G|" % (a, got, want, abs(got - want) / scale))
        assert abs(got - want) <= 1e-5 * scale, (a, got, want, scale)
    assert v_min < E.gram_value(G, [1.0, 0.0, 0.0]) and v_min == E.gram_value(G, a_min)
    for d in dtrs:
        d.close()


def _rigid_probes(P34):
    from epipolarconsistency_amd import geometry as Gm, pack_projection_matrices
    names = ("tx", "ty", "tz", "rx", "ry", "rz")
    return pack_projection_matrices([Gm.compose_transform(P34, Gm.rigid_transform(**{names[k]: s * STEPS[k]}))
                                     for k in range(6) for s in (1.0, -1.0)])


@pytest.mark.parametrize("incremental", [False, True])
@pytest.mark.parametrize("n", [20, 100])
def test_nothing_else_moved(gpu_ctx, incremental, n):
    """evaluate(), evaluate_pose_deltas and evaluate_gradient on the same metric object before and after an evaluate_gram: the same
    bits (n = 100: 4 950 pairs, the kept records of the reuse path are in play); a single-channel metric evaluated before and
    after a gram call on ANOTHER metric likewise."""
    import epipolarconsistency_amd as E
    K = 2
    Ps, dtrs = _scan(gpu_ctx, n, K, B=32)
    P0 = E.pack_projection_matrices(Ps)
    view = n // 2
    rows = _rigid_probes(P0[view].reshape(4, 3).T)
    P1 = P0.copy()
    P1[view] = rows[0]
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setIncremental(incremental)
    other = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs[:n])

    def observe(q):
        base = q.setProjectionMatrices(P0).evaluate()
        moved = q.setProjectionMatrices(P1).evaluate()      # one view moved: the reuse path refits its pairs only
        back = q.setProjectionMatrices(P0).evaluate()
        deltas = q.evaluate_pose_deltas([[view]] * 12, list(rows[:, None, :]))
        value, grad = q.evaluate_gradient(view, rows[0::2], rows[1::2], STEPS)
        cost = np.zeros((n, n), np.float32)
        with_cost = q.evaluate(cost)
        return np.concatenate([[base, moved, back, value, with_cost], deltas, grad]), cost
    before, cost_b = observe(m)
    other_before, ocost_b = observe(other)
    G = m.evaluate_gram(K)
    after, cost_a = observe(m)
    assert np.array_equal(_u64(before), _u64(after)) and np.array_equal(_u32(cost_b), _u32(cost_a))
    # in the middle of a sequence: matrices moved, then the gram call, then back
    m.setProjectionMatrices(P1).evaluate()
    G1 = m.evaluate_gram(K)
    assert _u64(m.evaluate())[()] == _u64(before[1])[()]          # the moved matrices are still current
    assert _u64(m.setProjectionMatrices(P0).evaluate())[()] == _u64(before[0])[()]
    assert np.array_equal(_u64(m.evaluate_gram(K)), _u64(G)) and not np.array_equal(_u64(G1), _u64(G))
    assert _u64(G[0, 0])[()] == _u64(before[0])[()]               # channel 0 is what the other calls evaluate
    other_after, ocost_a = observe(other)
    assert np.array_equal(_u64(other_before), _u64(other_after)) and np.array_equal(_u32(ocost_b), _u32(ocost_a))
    m.close()
    other.close()
    for d in dtrs:
        d.close()


def test_errors(gpu_ctx):
    import epipolarconsistency_amd as E
    n, K = 8, 2
    Ps, dtrs = _scan(gpu_ctx, n, K)
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs)
    want = m.evaluate()
    G = m.evaluate_gram(K)
    for bad in (1, 3, 4, 5, 0, -1):   # 1, 3, 4: not the metric's dtr count; 5, 0, -1: outside [1, ECC_GRAM_MAX_CHANNELS]
        with pytest.raises(E.EccError) as e:
            m.evaluate_gram(bad)
        assert e.value.code == 1, (bad, e.value)
    m.useCorrelation(True)
    with pytest.raises(E.EccError) as e:
        m.evaluate_gram(K)
    assert e.value.code == 5, e.value   # ECC_ERR_UNSUPPORTED
    m.useCorrelation(False)
    assert _u64(m.evaluate())[()] == _u64(want)[()] and np.array_equal(_u64(m.evaluate_gram(K)), _u64(G))
    m.close()
    empty = E.MetricRadonIntermediate(gpu_ctx, None, dtrs)   # no matrices set
    with pytest.raises(E.EccError) as e:
        empty.evaluate_gram(K)
    assert e.value.code == 1
    empty.close()
    one = E.MetricRadonIntermediate(gpu_ctx, Ps[:1], dtrs[:2])   # fewer than two views
    with pytest.raises(E.EccError) as e:
        one.evaluate_gram(2)
    assert e.value.code == 1
    one.close()
    for d in dtrs:
        d.close()
