"""ecc_metric_evaluate_robust_map[_pairs] and ecc_metric_robust_map_weights on the GPU (csrc/ecc_robust_map.hip,
csrc/robust_map_kernel.hip): where the robust loss rejects.  The cases are weighted_terms.CASES with the data of
channel 0, as tests/test_gpu_robust.py takes them.

  1 bit links       value, inlier_mass and the rows {c, u, r} equal evaluate_robust / _robust_pairs (==); delta = inf: REJ all zeros and
                    value == evaluate();
  2 the statement   HITS and REJ per bin against robust_map_terms, |got - want| / bin scale: 1e-6 under the reference arithmetic,
                    1e-3 on the throughput paths (tests/test_robust_map_terms_oracle.py shows that this comparison rejects the slips);
  3 conservation    sum HITS = the view's samples (1e-6), sum REJ = sum (1 - u) 2 n_kappa from the rows (1e-5);
  4 reproducible    two calls, a reversed list, a list cut in two and added in fixed point: identical;
  5 subsets         one view, the last view, an unordered list: the all-views planes bit for bit, rows unchanged;
  6 weights         robust_map_weights against numpy bit for bit; ones at delta = inf; accepted by a 2 n metric;
  7 the reason      an opaque block in view 6 that nobody flagged: the map finds the view, the lines, and its weights remove them;
  8 errors."""
import ctypes as C

import numpy as np
import pytest

import channel_terms as T
import robust_map_terms as M
import robust_terms as R
from test_gpu_robust import LOSS_CODES, _Case, _all_pairs_list, _close, _u32, _u64
from test_gpu_weighted import BLOCK, _flag

pytestmark = pytest.mark.gpu


@pytest.fixture
def case(gpu_ctx, oracle_mod, request):
    c = _Case(gpu_ctx, request.param)
    try:
        yield c
    finally:
        c.close()


def _same_scalars(a, b):
    return _u64(a[0])[()] == _u64(b[0])[()] and _u64(a[1])[()] == _u64(b[1])[()]


# ---- 1: bit links --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["d", "e", "i", "j"], indirect=True)
def test_bit_links(case):
    """Every setup of the case and, for case d, the three sampling modes on 2, 3 and all 8 views (1, 3 and 28 pairs); case e has
    2 145 pairs (reference arithmetic, one wave per pair) and its list of 300 (four waves per pair)."""
    E = case.E
    setups = [s for s, _ in case.setups] + (["polynomial", "per_sample", "reference"] if case.label == "d" else [])
    sizes = (2, 3, case.n) if case.label == "d" else (case.n,)
    delta = float(R.case_delta(case.label, "median"))
    for sampling in setups:
        for k in sizes:
            m = E.MetricRadonIntermediate(case.ctx, case.Ps[:k], case.data[:k]).setSampling(sampling)
            m.setObjectRadius(case.radius)
            m.setEpipolarPlaneStep(case.dkappa)
            idx = _all_pairs_list(k)[::-1][:300].copy()
            plain = m.evaluate()
            for loss in R.LOSSES:
                want = m.evaluate_robust(LOSS_CODES[loss], delta, want_pairs=True)
                got = m.evaluate_robust_map(LOSS_CODES[loss], delta, want_pairs=True)
                where = (case.label, sampling, k, loss)
                assert _same_scalars(got, want) and np.array_equal(_u32(got[4]), _u32(want[2])), where
                assert got[2].shape == (k, case.n_t, case.n_alpha) and got[2].dtype == np.float32 and np.all(got[3] <= got[2]), where
                assert got[3].max() > 0.0 and want[1] < 1.0, where                  # the loss rejects something at this delta
                lwant = m.evaluate_robust_pairs(idx, LOSS_CODES[loss], delta, want_pairs=True)
                lgot = m.evaluate_robust_map_pairs(idx, LOSS_CODES[loss], delta, want_pairs=True)
                assert _same_scalars(lgot, lwant) and np.array_equal(_u32(lgot[4]), _u32(lwant[2])), where
                inf = m.evaluate_robust_map(LOSS_CODES[loss], float("inf"))
                assert not inf[3].any() and _u64(inf[0])[()] == _u64(plain)[()] and inf[1] == 1.0, where
                assert np.array_equal(_u32(inf[2]), _u32(got[2])), where            # HITS: no loss and no delta in it
            m.close()


# ---- 2 and 3: the statement, conservation --------------------------------------------------------------------------------------------
def _conserved(hits, rej, rows, ij, n_kappa, where):
    """Per view: sum HITS against sum 2 n_kappa (1e-6), sum REJ against sum (1 - u) 2 n_kappa (1e-5: u is a float32 column)."""
    n = len(hits)
    samples, rejected = np.zeros(n), np.zeros(n)
    for (i, j), u, k in zip(ij, rows[:, 1].astype(np.float64), n_kappa):
        samples[[i, j]] += 2 * k
        rejected[[i, j]] += (1.0 - u) * 2 * k
    h, r = hits.astype(np.float64).sum(axis=(1, 2)), rej.astype(np.float64).sum(axis=(1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        eh = np.max(np.where(samples > 0, np.abs(h - samples) / samples, np.where(h > 0, np.inf, 0.0))) / 1e-6
        er = np.max(np.where(rejected > 0, np.abs(r - rejected) / rejected, np.where(r > 0, np.inf, 0.0))) / 1e-5
    print("%s: conservation, sum HITS %.3g of the bar 1e-6, sum REJ %.3g of the bar 1e-5" % (where, eh, er))
    return eh, er


STATEMENT = {"d": [("truncated", "p90"), ("huber", "median"), ("geman_mcclure", "median")], "e": [("truncated", "p90"), ("huber", "median")],
             "i": [("truncated", "p90"), ("huber", "median"), ("geman_mcclure", "p90")], "j": [("truncated", "p90"), ("geman_mcclure", "median")],
             "c": [("truncated", "p90")], "f": [("truncated", "p90")], "g": [("huber", "p90")]}


@pytest.mark.parametrize("case", sorted(STATEMENT), indirect=True)
def test_planes_against_the_statement(case):
    """Non-square bins (d, i, j: 96 x 64; g: 1000 x 767), plain data (i), kappa_max > pi/4 and = pi/2 (f, g, c with the row-quad
    copies), pairs without samples and footprints at the clamps in both coordinates (asserted from the statement below).  Case e's
    statement covers the oracle's sample of the pairs: the list form over those.  The worst ratios of a GPU run are in DESIGN.md 4.24."""
    failures = []
    n_kappa_all = np.array([len(T.kappa_grid(k)) for k in np.asarray(case.K01s, np.float32)])
    res = R.case_residuals(case.label)
    listed = len(res["pairs"]) != case.N
    idx = np.ascontiguousarray(np.concatenate([res["ij"], res["ij"]], axis=1), np.int32)
    for sampling, _ in case.setups:
        case.reached(sampling)
        m = case.metric(sampling)
        tol = T.tolerance(sampling, len(idx) if listed else case.N)
        for loss, scale in STATEMENT[case.label]:
            delta = float(R.case_delta(case.label, scale))
            want_h, want_r = M.case_map(case.label, loss, scale)
            s = M.bin_scale(want_h)
            if listed:
                _, _, hits, rej, rows = m.evaluate_robust_map_pairs(idx, LOSS_CODES[loss], delta, want_pairs=True)
            else:
                _, _, hits, rej, rows = m.evaluate_robust_map(LOSS_CODES[loss], delta, want_pairs=True)
            assert np.all(np.isfinite(hits)) and np.all(np.isfinite(rej)) and np.all(hits >= 0) and np.all(rej >= 0)
            a, b = M.compare(hits, want_h, s, tol), M.compare(rej, want_r, s, tol)
            where = "case %s %-10s %-13s %-6s" % (case.label, sampling, loss, scale)
            line = "%s (delta %.6g): HITS %.3g, REJ %.3g of the bar %.0e" % (where, delta, a, b, tol)
            if tol == T.TOL_THROUGHPUT:
                h64, r64 = M.case_map(case.label, loss, scale, "float64")
                line += "; against float64 positions HITS %.3g, REJ %.3g" % (M.compare(hits, h64, s, tol), M.compare(rej, r64, s, tol))
            print(line)
            eh, er = _conserved(hits, rej, rows, res["ij"], n_kappa_all[res["pairs"]], where)
            if not max(a, b, eh, er) <= 1.0:
                failures.append(line + "; conservation %.3g, %.3g" % (eh, er))
        m.close()
    if case.label in ("d", "f"):   # what the cases are there for, from the statement itself
        t32 = [M.pair_taps(case.K01s[q], case.n_alpha, case.n_t, case.n_u, case.n_v) for q in res["pairs"] if n_kappa_all[q]]
        i0 = np.concatenate([t[v][0] for t in t32 for v in (0, 1)]), np.concatenate([t[v][1] for t in t32 for v in (0, 1)])
        j0 = np.concatenate([t[v][2] for t in t32 for v in (0, 1)]), np.concatenate([t[v][3] for t in t32 for v in (0, 1)])
        print("case %s: footprints clamped in the angle %d, in the distance %d; pairs without samples %d; kappa_max up to %.4f" % (
            case.label, int((i0[0] == i0[1]).sum()), int((j0[0] == j0[1]).sum()), int((n_kappa_all == 0).sum()), case.K01s[:, 15].max()))
    assert not failures, "\n".join(failures)


def test_conservation_over_2145_pairs(gpu_ctx, oracle_mod):
    """Case e, all pairs (reference arithmetic, one wave per pair), no oracle needed: n_kappa from the C oracle's K01."""
    c = _Case(gpu_ctx, "e")
    try:
        m = c.metric("reference")
        n_kappa = np.array([len(T.kappa_grid(k)) for k in np.asarray(c.K01s, np.float32)])
        ij = _all_pairs_list(c.n)[:, :2]
        for loss in R.LOSSES:
            _, _, hits, rej, rows = m.evaluate_robust_map(LOSS_CODES[loss], float(R.case_delta("e", "median")), want_pairs=True)
            eh, er = _conserved(hits, rej, rows, ij, n_kappa, "case e all pairs %s" % loss)
            assert eh <= 1.0 and er <= 1.0, (loss, eh, er)
        m.close()
    finally:
        c.close()


# ---- 4 and 5: reproducible, subsets ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", ["polynomial", "per_sample", "reference"])
def test_reproducible_and_subsets(gpu_ctx, oracle_mod, sampling):
    """Two calls: identical plane bytes.  The list reversed: identical.  The list cut in two calls: the fixed-point sums (the planes
    before their one rounding to float32, read through ecc_debug_robust_map_fixed) add up to those of the whole list exactly, and every
    float plane is float32(q 2^-32) of its sums; a pair listed twice deposits twice, a pair without samples (P0 == P1) nothing.  views = one view, the last view, an unordered list: the all-views planes bit for
    bit, the rows unchanged."""
    import epipolarconsistency_amd as E
    c = _Case(gpu_ctx, "d")
    try:
        m = c.metric(sampling)
        delta = float(R.case_delta("d", "p90"))
        first = m.evaluate_robust_map(E.LOSS_HUBER, delta, want_pairs=True)
        again = m.evaluate_robust_map(E.LOSS_HUBER, delta, want_pairs=True)
        assert all(np.array_equal(_u32(first[k]), _u32(again[k])) for k in (2, 3, 4)) and _same_scalars(first, again)
        idx = _all_pairs_list(c.n)
        # a fixed mode for the three lists: "reference" for every length, or a throughput path (which does not depend on the length)
        fwd = m.evaluate_robust_map_pairs(idx, E.LOSS_HUBER, delta, want_pairs=True)
        q_fwd = m.robust_map_fixed()
        for k in (0, 1):
            assert np.array_equal(_u32(fwd[2 + k]), _u32((q_fwd[k].astype(np.float64) * 2.0 ** -32).astype(np.float32)))
        assert np.array_equal(_u32(fwd[2]), _u32(first[2])) and np.array_equal(_u32(fwd[3]), _u32(first[3])), sampling
        rev = m.evaluate_robust_map_pairs(idx[::-1].copy(), E.LOSS_HUBER, delta, want_pairs=True)
        assert np.array_equal(_u32(rev[2]), _u32(fwd[2])) and np.array_equal(_u32(rev[3]), _u32(fwd[3]))
        assert np.array_equal(_u32(rev[4]), _u32(fwd[4][::-1]))
        cut = 11
        m.evaluate_robust_map_pairs(idx[:cut], E.LOSS_HUBER, delta)
        q_a = m.robust_map_fixed()
        m.evaluate_robust_map_pairs(idx[cut:], E.LOSS_HUBER, delta)
        q_b = m.robust_map_fixed()
        for k in (0, 1):
            assert np.array_equal(q_a[k] + q_b[k], q_fwd[k]), (sampling, k)
        twice = m.evaluate_robust_map_pairs(np.concatenate([idx, idx[:cut]]), E.LOSS_HUBER, delta)   # a pair listed twice deposits twice
        q_twice = m.robust_map_fixed()
        assert all(np.array_equal(q_twice[k], q_fwd[k] + q_a[k]) for k in (0, 1)) and twice[2].sum() > fwd[2].sum()
        dead = m.evaluate_robust_map_pairs(np.concatenate([idx, [[2, 2, 2, 3]]]).astype(np.int32), E.LOSS_HUBER, delta, want_pairs=True)
        assert np.array_equal(dead[4][-1], [0.0, 1.0, 0.0])            # a pair without samples: its row, and no deposit
        assert all(np.array_equal(a, b) for a, b in zip(m.robust_map_fixed(), q_fwd))
        for views in ([2], [c.n - 1], [5, 0, c.n - 1, 3]):
            part = m.evaluate_robust_map(E.LOSS_HUBER, delta, views=views, want_pairs=True)
            assert part[2].shape[0] == len(views) and _same_scalars(part, first) and np.array_equal(_u32(part[4]), _u32(first[4]))
            for k, v in enumerate(views):
                assert np.array_equal(_u32(part[2][k]), _u32(first[2][v])) and np.array_equal(_u32(part[3][k]), _u32(first[3][v])), (views, v)
            lpart = m.evaluate_robust_map_pairs(idx, E.LOSS_HUBER, delta, views=views)
            assert np.array_equal(_u32(lpart[2]), _u32(part[2])) and np.array_equal(_u32(lpart[3]), _u32(part[3]))
        m.close()
    finally:
        c.close()


# ---- 6: the map as line weights -------------------------------------------------------------------------------------------------------
def test_map_weights(gpu_ctx, oracle_mod):
    import epipolarconsistency_amd as E
    c = _Case(gpu_ctx, "d")
    try:
        m = c.metric("polynomial")
        delta = float(R.case_delta("d", "median"))
        _, _, hits, rej = m.evaluate_robust_map(E.LOSS_TRUNCATED, delta)
        assert (hits < 1.0).any() and (hits >= 4.0).any()
        for min_hits, gain in ((0.0, 1.0), (1.0, 1.0), (4.0, 2.5)):
            ws = m.robust_map_weights(min_hits, gain)
            assert len(ws) == c.n and ws[0].getFilter() == E.FILTER_NONE
            for v, w in enumerate(ws):
                got, want = w.readback(), M.map_weights(hits[v], rej[v], min_hits, gain)
                assert np.array_equal(_u32(got), _u32(want)), (min_hits, gain, v, int((_u32(got) != _u32(want)).sum()))
            assert any((w.readback() < 1.0).any() for w in ws)
            _close(ws)
        part = m.evaluate_robust_map(E.LOSS_TRUNCATED, delta, views=[4, 1])
        ws = m.robust_map_weights()
        assert len(ws) == 2 and np.array_equal(_u32(ws[0].readback()), _u32(M.map_weights(part[2][0], part[3][0])))
        assert np.array_equal(_u32(part[2][0]), _u32(hits[4]))
        _close(ws)
        m.evaluate_robust_map(E.LOSS_TRUNCATED, float("inf"))
        ones = m.robust_map_weights(0.0, 3.0)
        flat = [w.readback() for w in ones]
        assert all(np.all((f == 1.0) | (h == 0.0)) for f, h in zip(flat, hits))    # (0 / 0 under min_hits = 0: weight 0, never sampled)
        ones1 = m.robust_map_weights(1.0, 3.0)
        assert all(np.all(w.readback() == 1.0) for w in ones1)
        m2 = E.MetricRadonIntermediate(gpu_ctx, c.Ps, c.data + ones1).setSampling("polynomial")
        m2.setObjectRadius(c.radius)
        m2.setEpipolarPlaneStep(c.dkappa)
        value, coverage = m2.evaluate_weighted()
        assert _u64(value)[()] == _u64(m.evaluate())[()] and coverage == 1.0
        m2.close()
        _close(ones + ones1)
        m.refreshRadonIntermediates(0, 1)                          # drops the held map
        with pytest.raises(E.EccError) as e:
            m.robust_map_weights()
        assert e.value.code == 1
        m.evaluate_robust_map(E.LOSS_TRUNCATED, delta)
        m.setObjectRadius(c.radius + 1.0)                          # so do the parameters
        with pytest.raises(E.EccError):
            m.robust_map_weights()
        m.close()
    finally:
        c.close()


# ---- 7: the reason the call exists ------------------------------------------------------------------------------------------------------
BAD_VIEW, GAIN, MIN_HITS = 6, 1.0, 1.0


@pytest.mark.parametrize("sampling", ["polynomial", "per_sample", "auto"])
def test_a_block_nobody_flagged_is_found_and_removed(gpu_ctx, small_scan, sampling):
    """8 views of the spheres at 128^2 -> 96^2 bins, the opaque block of tests/test_gpu_weighted.py in view 6, flagged nowhere;
    truncated loss, delta = robust_scale(rows at delta = inf, 0.5).  (a) the view with the largest sum REJ / sum HITS is view 6;
    (b) in view 6 the bins to which line_weights of the block's flagged image gives weight 0 hold a larger share of sum REJ than of
    sum HITS; (c) with mu = robust_map_weights on all 8 views, corrupted / clean of evaluate_weighted is below that of evaluate().
    The statement passes the same three on the CPU (tests/test_robust_map_terms_oracle.py).  The ratio of (c) is measured, not fixed:
    a run's figures are in DESIGN.md 4.24."""
    import epipolarconsistency_amd as E
    imgs, Ps, B = small_scan["imgs"], small_scan["Ps"], 96
    n = len(Ps)
    bad = np.array(imgs, np.float32)
    bad[BAD_VIEW][BLOCK] += 4.0 * float(np.max(imgs[BAD_VIEW]))
    clean_d = E.RadonIntermediate.compute_batch(gpu_ctx, np.asarray(imgs, np.float32), B, B)
    bad_d = E.RadonIntermediate.compute_batch(gpu_ctx, bad, B, B)
    flagged = E.line_weights(gpu_ctx, _flag(imgs[0].shape), B, B, guard_bins=1)
    zero = flagged.readback() == 0.0
    m_bad = E.MetricRadonIntermediate(gpu_ctx, Ps, bad_d).setSampling(sampling)
    m_clean = E.MetricRadonIntermediate(gpu_ctx, Ps, clean_d).setSampling(sampling)
    first = m_bad.evaluate_robust(E.LOSS_TRUNCATED, float("inf"), want_pairs=True)[2]
    delta = E.robust_scale(first, 0.5)
    _, mass, hits, rej = m_bad.evaluate_robust_map(E.LOSS_TRUNCATED, delta)
    h, r = hits.astype(np.float64), rej.astype(np.float64)
    share = r.sum(axis=(1, 2)) / h.sum(axis=(1, 2))
    rej_share, hit_share = r[BAD_VIEW][zero].sum() / r[BAD_VIEW].sum(), h[BAD_VIEW][zero].sum() / h[BAD_VIEW].sum()
    mu = m_bad.robust_map_weights(MIN_HITS, GAIN)
    w_bad = E.MetricRadonIntermediate(gpu_ctx, Ps, bad_d + mu).setSampling(sampling)
    w_clean = E.MetricRadonIntermediate(gpu_ctx, Ps, clean_d + mu).setSampling(sampling)
    weighted = w_bad.evaluate_weighted()[0] / w_clean.evaluate_weighted()[0]
    plain = m_bad.evaluate() / m_clean.evaluate()
    print("%s: delta %.6g, inlier mass %.4f; sum REJ / sum HITS per view: %s; view 6, flagged bins: %.4f of sum REJ, %.4f of sum HITS; "
          "corrupted / clean: evaluate() %.4g, evaluate_weighted under the map's weights (min_hits %g, gain %g) %.4g" % (
              sampling, delta, mass, " ".join("%.4f" % v for v in share), rej_share, hit_share, plain, MIN_HITS, GAIN, weighted))
    for m in (m_bad, m_clean, w_bad, w_clean):
        m.close()
    _close(clean_d + bad_d + mu + [flagged])
    assert int(np.argmax(share)) == BAD_VIEW, share                 # (a)
    assert zero.any() and rej_share > hit_share, (rej_share, hit_share)   # (b)
    assert weighted < plain, (weighted, plain)                     # (c)


# ---- 8: errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors(gpu_ctx, oracle_mod):
    """In the stated order: evaluate_robust's own first, then the views list; robust_map_weights before any map call.  Nothing written."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib
    L = _lib.lib()
    c = _Case(gpu_ctx, "d")
    try:
        m = c.metric("auto")
        delta = float(R.case_delta("d", "p90"))
        handles = (C.c_void_p * c.n)()
        assert L.ecc_metric_robust_map_weights(m._h, 1.0, 1.0, handles) == 1 and b"no robust map held" in L.ecc_last_error()
        with pytest.raises(E.EccError):
            m.robust_map_weights()
        bins = c.n_t * c.n_alpha
        value, mass = C.c_double(-1.0), C.c_double(-1.0)
        terms, hits, rej = np.full((c.N, 3), -1.0, np.float32), np.full(c.n * bins, -1.0, np.float32), np.full(c.n * bins, -1.0, np.float32)
        out = (C.c_void_p(hits.ctypes.data), C.c_void_p(rej.ctypes.data), C.byref(value), C.byref(mass), C.c_void_p(terms.ctypes.data))
        idx = _all_pairs_list(c.n)
        pidx = C.c_void_p(idx.ctypes.data)

        def both(h, loss, d, views, k, outs=out, lst=pidx, count=len(idx)):
            v = None if views is None else C.c_void_p(np.ascontiguousarray(views, np.int32).ctypes.data)
            return (L.ecc_metric_evaluate_robust_map(h, loss, d, v, k, *outs),
                    L.ecc_metric_evaluate_robust_map_pairs(h, lst, count, loss, d, v, k, *outs))
        for views, k in (([0, 1, 1], 3), ([3, 3], 2), ([0, c.n], 2), ([-1], 1), ([0], -1), (None, 2)):
            assert both(m._h, 0, delta, views, k) == (1, 1), (views, k)
        L.ecc_metric_evaluate_robust_map(m._h, 0, delta, C.c_void_p(np.array([3, 3], np.int32).ctypes.data), 2, *out)
        assert b"listed twice" in L.ecc_last_error()
        assert both(m._h, 7, delta, [3, 3], 2) == (1, 1) and b"loss" in L.ecc_last_error()          # the loss comes before the list
        assert both(m._h, 0, -1.0, [0, c.n], 2) == (1, 1) and b"delta" in L.ecc_last_error()
        assert both(m._h, 0, delta, None, 0, outs=(out[0], out[1], None, out[3], out[4])) == (1, 1)   # value == NULL
        assert L.ecc_metric_evaluate_robust_map_pairs(m._h, pidx, -1, 0, delta, None, 0, *out) == 1
        bad = np.concatenate([idx[:3], [[0, 1, c.n, 1]]]).astype(np.int32)
        assert L.ecc_metric_evaluate_robust_map_pairs(m._h, C.c_void_p(bad.ctypes.data), 4, 0, delta, None, 0, *out) == 1
        m.useCorrelation(True)
        assert both(m._h, 0, delta, [3, 3], 2) == (5, 5)                                          # ECC_ERR_UNSUPPORTED, before the list
        m.useCorrelation(False)
        assert value.value == -1.0 and mass.value == -1.0 and np.all(terms == -1.0) and np.all(hits == -1.0) and np.all(rej == -1.0)
        assert L.ecc_metric_robust_map_weights(m._h, 1.0, 1.0, handles) == 1                     # still no map: every call above failed
        got = m.evaluate_robust_map(E.LOSS_HUBER, delta, want_pairs=True)
        want = m.evaluate_robust(E.LOSS_HUBER, delta, want_pairs=True)
        assert _same_scalars(got, want) and np.array_equal(_u32(got[4]), _u32(want[2]))
        for min_hits, gain in ((-1.0, 1.0), (1.0, -0.5), (float("nan"), 1.0), (1.0, float("inf"))):
            assert L.ecc_metric_robust_map_weights(m._h, min_hits, gain, handles) == 1, (min_hits, gain)
        assert L.ecc_metric_robust_map_weights(m._h, 1.0, 1.0, None) == 1
        empty = m.evaluate_robust_map_pairs(np.zeros((0, 4), np.int32), E.LOSS_HUBER, delta)      # an empty list: zeros, no map held
        assert not empty[2].any() and not empty[3].any()
        with pytest.raises(E.EccError):
            m.robust_map_weights()
        m.close()
    finally:
        c.close()
