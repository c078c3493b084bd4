"""ecc_metric_evaluate_weighted_robust_map[_pairs] and ecc_metric_weighted_robust_map_weights on the GPU
(csrc/ecc_weighted_robust_map.hip, csrc/weighted_robust_map_kernel.hip): where the robust loss rejects on a metric
that already carries line weights.  The cases are weighted_terms.CASES with weighted_terms.case_inputs' weights, as
tests/test_gpu_weighted_robust.py takes them.

  1 bit links       value, coverage, inlier_mass and the rows {c, u, k, r} equal evaluate_weighted_robust / _pairs (==); delta = inf:
                    REJ all zeros, value and coverage are evaluate_weighted's; every weight 1.0f: the fixed-point sums are
                    evaluate_robust_map's on the n-metric over the same data, cell for cell;
  2 the statement   HITS and REJ per bin against weighted_robust_map_terms, |got - want| / bin scale: 1e-6 under the reference
                    arithmetic, 1e-3 on the throughput paths (tests/test_weighted_robust_map_terms_oracle.py shows that this
                    comparison rejects the slips);
  3 conservation    sum HITS = sum u 2 n_kappa (1e-6), sum REJ = sum (u - k) 2 n_kappa (1e-5), from the rows;
  4 reproducible    two calls, a reversed list, a list cut in two and added in fixed point: identical;
  5 subsets         one view, the last view, an unordered list: the all-views planes bit for bit, rows unchanged;
  6 a view of weight 0   its planes are exactly 0, the other views' fixed-point sums those of the list without its pairs;
  7 weights         weighted_robust_map_weights against numpy bit for bit; W_old at delta = inf; accepted by a 2 n metric; refused
                    when the held map is the n-metric's;
  8 the reason      a second pass improves on the first; refine_line_weights returns pass 2's weights;
  9 errors."""
import ctypes as C

import numpy as np
import pytest

import channel_terms as T
import robust_map_terms as M
import robust_terms as R
import weighted_robust_map_terms as WM
import weighted_robust_terms as WR
from test_gpu_weighted import BLOCK, _Case
from test_gpu_weighted_robust import LOSS_CODES, _all_pairs_list, _close, _ones, _u32, _u64

pytestmark = pytest.mark.gpu


@pytest.fixture
def case(gpu_ctx, oracle_mod, request):
    c = _Case(gpu_ctx, request.param)
    try:
        yield c
    finally:
        c.close()


def _same_scalars(a, b, k=3):
    return all(_u64(a[q])[()] == _u64(b[q])[()] for q in range(k))


def _same_fixed(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1: bit links --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["d", "e", "i", "j"], indirect=True)
def test_bit_links(case):
    """Every setup of the case and, for case d, the three sampling modes; case e has 2 145 pairs (reference arithmetic, one wave per
    pair) and its list of 300 (four waves per pair)."""
    ws, ones = case.weight_dtrs(case.weights), _ones(case)
    setups = [s for s, _ in case.setups] + (["polynomial", "per_sample", "reference"] if case.label == "d" else [])
    delta = float(R.case_delta(case.label, "median"))
    idx = _all_pairs_list(case.n)[::-1][:300].copy()
    for sampling in setups:
        m, m_ones, m_plain = case.metric(sampling, ws), case.metric(sampling, ones), case.metric(sampling, [])
        weighted = m.evaluate_weighted()
        for loss in R.LOSSES:
            where = (case.label, sampling, loss)
            want = m.evaluate_weighted_robust(LOSS_CODES[loss], delta, want_pairs=True)
            got = m.evaluate_weighted_robust_map(LOSS_CODES[loss], delta, want_pairs=True)
            assert _same_scalars(got, want) and np.array_equal(_u32(got[5]), _u32(want[3])), where
            assert got[3].shape == (case.n, case.n_t, case.n_alpha) and got[3].dtype == np.float32 and np.all(got[4] <= got[3]), where
            assert got[4].max() > 0.0 and want[2] < 1.0 and want[1] < 1.0, where     # the loss rejects, the weights remove
            lwant = m.evaluate_weighted_robust_pairs(idx, LOSS_CODES[loss], delta, want_pairs=True)
            lgot = m.evaluate_weighted_robust_map_pairs(idx, LOSS_CODES[loss], delta, want_pairs=True)
            assert _same_scalars(lgot, lwant) and np.array_equal(_u32(lgot[5]), _u32(lwant[3])), where
            inf = m.evaluate_weighted_robust_map(LOSS_CODES[loss], float("inf"))
            assert not inf[4].any() and _u64(inf[0])[()] == _u64(weighted[0])[()] and _u64(inf[1])[()] == _u64(weighted[1])[()], where
            assert inf[2] == 1.0 and np.array_equal(_u32(inf[3]), _u32(got[3])), where     # HITS: no loss and no delta in it
            # every weight 1.0f: the n-metric's map, in fixed point
            one = m_ones.evaluate_weighted_robust_map(LOSS_CODES[loss], delta, want_pairs=True)
            q_one = m_ones.robust_map_fixed()
            plain = m_plain.evaluate_robust_map(LOSS_CODES[loss], delta, want_pairs=True)
            assert _same_fixed(q_one, m_plain.robust_map_fixed()), where
            assert np.array_equal(_u32(one[3]), _u32(plain[2])) and np.array_equal(_u32(one[4]), _u32(plain[3])), where
            assert np.array_equal(_u32(one[5][:, (0, 2, 3)]), _u32(plain[4])) and one[1] == 1.0, where
            lone = m_ones.evaluate_weighted_robust_map_pairs(idx, LOSS_CODES[loss], delta)
            q_lone = m_ones.robust_map_fixed()
            lplain = m_plain.evaluate_robust_map_pairs(idx, LOSS_CODES[loss], delta)
            assert _same_fixed(q_lone, m_plain.robust_map_fixed()) and _u64(lone[0])[()] == _u64(lplain[0])[()], where
        for x in (m, m_ones, m_plain):
            x.close()


# ---- 2 and 3: the statement, conservation --------------------------------------------------------------------------------------------
def _conserved(hits, rej, rows, ij, n_kappa, where):
    """Per view: sum HITS against sum u 2 n_kappa (1e-6), sum REJ against sum (u - k) 2 n_kappa (1e-5: u and k are float32 columns)."""
    n = len(hits)
    mass, refused = np.zeros(n), np.zeros(n)
    for (i, j), u, kept, k in zip(ij, rows[:, 1].astype(np.float64), rows[:, 2].astype(np.float64), n_kappa):
        mass[[i, j]] += u * 2 * k
        refused[[i, j]] += (u - kept) * 2 * k
    h, r = hits.astype(np.float64).sum(axis=(1, 2)), rej.astype(np.float64).sum(axis=(1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        eh = np.max(np.where(mass > 0, np.abs(h - mass) / mass, np.where(h > 0, np.inf, 0.0))) / 1e-6
        er = np.max(np.where(refused > 0, np.abs(r - refused) / refused, np.where(r > 0, np.inf, 0.0))) / 1e-5
    print("%s: conservation, sum HITS %.3g of the bar 1e-6, sum REJ %.3g of the bar 1e-5" % (where, eh, er))
    return eh, er


STATEMENT = {"d": [("truncated", "p90"), ("huber", "median"), ("geman_mcclure", "median")], "e": [("truncated", "p90"), ("huber", "median")],
             "i": [("truncated", "p90"), ("huber", "median"), ("geman_mcclure", "p90")], "j": [("truncated", "p90"), ("geman_mcclure", "median")],
             "c": [("truncated", "p90")], "f": [("truncated", "p90")]}


@pytest.mark.parametrize("case", sorted(STATEMENT), indirect=True)
def test_planes_against_the_statement(case):
    """Non-square bins (d, i, j: 96 x 64), plain data (i), kappa_max = pi/2 (f) and the row-quad copies (c) at one setting each.
    Case e's statement covers the oracle's sample of the pairs: the list form over those.  The worst ratios of a GPU run are in
    DESIGN.md 4.25."""
    failures = []
    ws = case.weight_dtrs(case.weights)
    n_kappa_all = np.array([len(T.kappa_grid(k)) for k in np.asarray(case.K01s, np.float32)])
    smp = WR.case_samples(case.label)
    listed = len(smp["pairs"]) != case.N
    idx = np.ascontiguousarray(np.concatenate([smp["ij"], smp["ij"]], axis=1), np.int32)
    for sampling, _ in case.setups:
        m = case.metric(sampling, ws)
        tol = T.tolerance(sampling, len(idx) if listed else case.N)
        for loss, scale in STATEMENT[case.label]:
            delta = float(R.case_delta(case.label, scale))
            want_h, want_r = WM.case_map(case.label, loss, scale)
            s = WM.case_scale(case.label, loss, scale)
            if listed:
                _, _, _, hits, rej, rows = m.evaluate_weighted_robust_map_pairs(idx, LOSS_CODES[loss], delta, want_pairs=True)
            else:
                _, _, _, hits, rej, rows = m.evaluate_weighted_robust_map(LOSS_CODES[loss], delta, want_pairs=True)
            assert np.all(np.isfinite(hits)) and np.all(np.isfinite(rej)) and np.all(hits >= 0) and np.all(rej >= 0)
            a, b = M.compare(hits, want_h, s, tol), M.compare(rej, want_r, s, tol)
            where = "case %s %-10s %-13s %-6s" % (case.label, sampling, loss, scale)
            line = "%s (delta %.6g): HITS %.3g, REJ %.3g of the bar %.0e" % (where, delta, a, b, tol)
            if tol == T.TOL_THROUGHPUT and case.label not in ("c", "f"):
                h64, r64 = WM.case_map(case.label, loss, scale, "float64")
                line += "; against float64 positions HITS %.3g, REJ %.3g" % (M.compare(hits, h64, s, tol), M.compare(rej, r64, s, tol))
            print(line)
            eh, er = _conserved(hits, rej, rows, smp["ij"], n_kappa_all[smp["pairs"]], where)
            if not max(a, b, eh, er) <= 1.0:
                failures.append(line + "; conservation %.3g, %.3g" % (eh, er))
        m.close()
    assert not failures, "\n".join(failures)


# ---- 4 and 5: reproducible, subsets ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", ["polynomial", "per_sample", "reference"])
def test_reproducible_and_subsets(gpu_ctx, oracle_mod, sampling):
    """Two calls: identical plane bytes.  The list reversed: identical.  The list cut in two calls: the fixed-point sums add up to
    those of the whole list exactly, and every float plane is float32(q 2^-32) of its sums; a pair listed twice deposits twice, a pair
    without samples (P0 == P1) nothing.  views = one view, the last view, an unordered list: the all-views planes bit for bit, the
    rows unchanged."""
    import epipolarconsistency_amd as E
    c = _Case(gpu_ctx, "d")
    try:
        m = c.metric(sampling, c.weight_dtrs(c.weights))
        delta = float(R.case_delta("d", "p90"))
        first = m.evaluate_weighted_robust_map(E.LOSS_HUBER, delta, want_pairs=True)
        again = m.evaluate_weighted_robust_map(E.LOSS_HUBER, delta, want_pairs=True)
        assert all(np.array_equal(_u32(first[k]), _u32(again[k])) for k in (3, 4, 5)) and _same_scalars(first, again)
        idx = _all_pairs_list(c.n)
        # a fixed mode for the three lists: "reference" for every length, or a throughput path (which does not depend on the length)
        fwd = m.evaluate_weighted_robust_map_pairs(idx, E.LOSS_HUBER, delta, want_pairs=True)
        q_fwd = m.robust_map_fixed()
        for k in (0, 1):
            assert np.array_equal(_u32(fwd[3 + k]), _u32((q_fwd[k].astype(np.float64) * 2.0 ** -32).astype(np.float32)))
        assert np.array_equal(_u32(fwd[3]), _u32(first[3])) and np.array_equal(_u32(fwd[4]), _u32(first[4])), sampling
        rev = m.evaluate_weighted_robust_map_pairs(idx[::-1].copy(), E.LOSS_HUBER, delta, want_pairs=True)
        assert np.array_equal(_u32(rev[3]), _u32(fwd[3])) and np.array_equal(_u32(rev[4]), _u32(fwd[4]))
        assert np.array_equal(_u32(rev[5]), _u32(fwd[5][::-1]))
        cut = 11
        m.evaluate_weighted_robust_map_pairs(idx[:cut], E.LOSS_HUBER, delta)
        q_a = m.robust_map_fixed()
        m.evaluate_weighted_robust_map_pairs(idx[cut:], E.LOSS_HUBER, delta)
        q_b = m.robust_map_fixed()
        for k in (0, 1):
            assert np.array_equal(q_a[k] + q_b[k], q_fwd[k]), (sampling, k)
        twice = m.evaluate_weighted_robust_map_pairs(np.concatenate([idx, idx[:cut]]), E.LOSS_HUBER, delta)
        q_twice = m.robust_map_fixed()
        assert all(np.array_equal(q_twice[k], q_fwd[k] + q_a[k]) for k in (0, 1)) and twice[3].sum() > fwd[3].sum()
        dead = m.evaluate_weighted_robust_map_pairs(np.concatenate([idx, [[2, 2, 2, 3]]]).astype(np.int32), E.LOSS_HUBER, delta, want_pairs=True)
        assert np.array_equal(dead[5][-1], [0.0, 1.0, 1.0, 0.0])        # a pair without samples: its row, and no deposit
        assert _same_fixed(m.robust_map_fixed(), q_fwd)
        for views in ([2], [c.n - 1], [5, 0, c.n - 1, 3]):
            part = m.evaluate_weighted_robust_map(E.LOSS_HUBER, delta, views=views, want_pairs=True)
            assert part[3].shape[0] == len(views) and _same_scalars(part, first) and np.array_equal(_u32(part[5]), _u32(first[5]))
            for k, v in enumerate(views):
                assert np.array_equal(_u32(part[3][k]), _u32(first[3][v])) and np.array_equal(_u32(part[4][k]), _u32(first[4][v])), (views, v)
            lpart = m.evaluate_weighted_robust_map_pairs(idx, E.LOSS_HUBER, delta, views=views)
            assert np.array_equal(_u32(lpart[3]), _u32(part[3])) and np.array_equal(_u32(lpart[4]), _u32(part[4]))
        m.close()
    finally:
        c.close()


# ---- 6: a view whose weights are all 0 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", ["polynomial", "per_sample", "reference"])
def test_a_view_of_weight_zero(gpu_ctx, oracle_mod, sampling):
    """W_v = 0, the case's weights elsewhere: the planes of v are exactly 0 (every sample taken in v has mu = 0), and the other views'
    fixed-point sums are those of the list form over the pairs without v: the pairs with v deposit nothing anywhere."""
    import epipolarconsistency_amd as E
    c = _Case(gpu_ctx, "d")
    try:
        v = 3
        fields = list(c.weights)
        fields[v] = np.zeros((c.n_t, c.n_alpha), np.float32)
        m = c.metric(sampling, c.weight_dtrs(fields))
        delta = float(R.case_delta("d", "median"))
        for loss in (E.LOSS_TRUNCATED, E.LOSS_HUBER):
            got = m.evaluate_weighted_robust_map(loss, delta, want_pairs=True)
            q_all = m.robust_map_fixed()
            assert not got[3][v].any() and not got[4][v].any() and not q_all[0][v].any() and not q_all[1][v].any()
            idx = _all_pairs_list(c.n)
            hit = (idx[:, 0] == v) | (idx[:, 1] == v)
            assert np.all(got[5][hit] == 0.0) and got[3].sum() > 0.0 and got[4].sum() > 0.0
            m.evaluate_weighted_robust_map_pairs(idx[~hit].copy(), loss, delta)
            assert _same_fixed(m.robust_map_fixed(), q_all), (sampling, loss)
        m.close()
    finally:
        c.close()


# ---- 7: the map as the next pass's weights ------------------------------------------------------------------------------------------------
def test_map_weights(gpu_ctx, oracle_mod):
    import epipolarconsistency_amd as E
    c = _Case(gpu_ctx, "d")
    try:
        ws = c.weight_dtrs(c.weights)
        m = c.metric("polynomial", ws)
        delta = float(R.case_delta("d", "median"))
        _, _, _, hits, rej = m.evaluate_weighted_robust_map(E.LOSS_TRUNCATED, delta)
        assert (hits < 1.0).any() and (hits >= 4.0).any()
        for min_hits, gain in ((0.0, 1.0), (1.0, 1.0), (4.0, 2.5)):
            new = m.weighted_robust_map_weights(min_hits, gain)
            assert len(new) == c.n and new[0].getFilter() == E.FILTER_NONE
            for v, w in enumerate(new):
                got, want = w.readback(), WM.map_weights(c.weights[v], hits[v], rej[v], min_hits, gain)
                assert np.array_equal(_u32(got), _u32(want)), (min_hits, gain, v, int((_u32(got) != _u32(want)).sum()))
            assert any((w.readback() < f).any() for w, f in zip(new, c.weights))
            _close(new)
        part = m.evaluate_weighted_robust_map(E.LOSS_TRUNCATED, delta, views=[4, 1])
        new = m.weighted_robust_map_weights()
        assert len(new) == 2 and np.array_equal(_u32(part[3][0]), _u32(hits[4]))
        for k, v in enumerate((4, 1)):                                   # the weight follows the mapped view, not the slot
            assert np.array_equal(_u32(new[k].readback()), _u32(WM.map_weights(c.weights[v], part[3][k], part[4][k])))
        _close(new)
        m.evaluate_weighted_robust_map(E.LOSS_TRUNCATED, float("inf"))
        same = m.weighted_robust_map_weights(1.0, 3.0)                   # nothing rejected: W_old
        assert all(np.array_equal(_u32(w.readback()), _u32(f)) for w, f in zip(same, c.weights))
        m.evaluate_weighted_robust_map(E.LOSS_TRUNCATED, delta)
        second = m.weighted_robust_map_weights()
        m2 = c.metric("polynomial", second)                              # the second half of a new 2 n metric
        value, coverage, mass = m2.evaluate_weighted_robust(E.LOSS_TRUNCATED, delta)
        before = m.evaluate_weighted_robust(E.LOSS_TRUNCATED, delta)
        assert 0.0 < coverage < before[1] and value > 0.0 and 0.0 < mass <= 1.0     # less mass trusted than under the old weights
        m2.close()
        _close(same + second)
        m.evaluate_robust_map(E.LOSS_TRUNCATED, delta)                   # the n-metric's map, held by the same metric
        with pytest.raises(E.EccError) as e:
            m.weighted_robust_map_weights()
        assert e.value.code == 1
        m.evaluate_weighted_robust_map(E.LOSS_TRUNCATED, delta)          # ... and the other way round
        with pytest.raises(E.EccError):
            m.robust_map_weights()
        _close(m.weighted_robust_map_weights())
        m.refreshRadonIntermediates(0, 1)                                # drops the held map
        with pytest.raises(E.EccError):
            m.weighted_robust_map_weights()
        m.close()
        plain = c.metric("polynomial", [])
        plain.evaluate_robust_map(E.LOSS_TRUNCATED, delta)
        with pytest.raises(E.EccError):
            plain.weighted_robust_map_weights()
        plain.close()
    finally:
        c.close()


# ---- 8: the reason the call exists ------------------------------------------------------------------------------------------------------
BAD_VIEW, GAIN, MIN_HITS = 6, 1.0, 1.0


@pytest.mark.parametrize("sampling", ["polynomial", "per_sample", "auto"])
def test_a_second_pass_improves_on_the_first(gpu_ctx, small_scan, sampling):
    """The fixture of tests/test_gpu_robust_map.py's test 7: 8 views of the spheres at 128^2 -> 96^2 bins, the opaque block in view 6,
    flagged nowhere; truncated loss, delta = robust_scale(rows at delta = inf, 0.5), held; gain 1, min_hits 1.  Pass 1: the n-metric's
    map and its weights.  Pass 2: the map of the 2 n metric under those weights, W * factor.  corrupted / clean of evaluate_weighted
    under pass 2's weights is below that under pass 1's.  The ratios are measured, not fixed: a run's figures are in DESIGN.md 4.25.
    refine_line_weights(passes=2) returns pass 2's weights bit for bit."""
    import epipolarconsistency_amd as E
    imgs, Ps, B = small_scan["imgs"], small_scan["Ps"], 96
    bad = np.array(imgs, np.float32)
    bad[BAD_VIEW][BLOCK] += 4.0 * float(np.max(imgs[BAD_VIEW]))
    clean_d = E.RadonIntermediate.compute_batch(gpu_ctx, np.asarray(imgs, np.float32), B, B)
    bad_d = E.RadonIntermediate.compute_batch(gpu_ctx, bad, B, B)

    def metric(dtrs):
        return E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling(sampling)

    def ratio(mu):
        w_bad, w_clean = metric(bad_d + mu), metric(clean_d + mu)
        out = w_bad.evaluate_weighted()[0] / w_clean.evaluate_weighted()[0]
        w_bad.close()
        w_clean.close()
        return out
    m1 = metric(bad_d)
    delta = E.robust_scale(m1.evaluate_robust(E.LOSS_TRUNCATED, float("inf"), want_pairs=True)[2], 0.5)
    m1.evaluate_robust_map(E.LOSS_TRUNCATED, delta)
    mu1 = m1.robust_map_weights(MIN_HITS, GAIN)
    m1.close()
    m2 = metric(bad_d + mu1)
    _, cover, mass, hits, rej = m2.evaluate_weighted_robust_map(E.LOSS_TRUNCATED, delta)
    mu2 = m2.weighted_robust_map_weights(MIN_HITS, GAIN)
    m2.close()
    first, second = ratio(mu1), ratio(mu2)
    share = rej.astype(np.float64).sum(axis=(1, 2)) / hits.astype(np.float64).sum(axis=(1, 2))
    print("%s: delta %.6g; pass 2: coverage %.4f, inlier mass %.4f, sum REJ / sum HITS per view: %s; corrupted / clean of "
          "evaluate_weighted: %.4g under pass 1's weights, %.4g under pass 2's" % (
              sampling, delta, cover, mass, " ".join("%.4f" % v for v in share), first, second))
    refined, records = E.refine_line_weights(gpu_ctx, Ps, bad_d, passes=2, min_hits=MIN_HITS, gain=GAIN, sampling=sampling)
    same = [np.array_equal(_u32(a.readback()), _u32(b.readback())) for a, b in zip(refined, mu2)]
    below = all(np.all(b.readback() <= a.readback()) for a, b in zip(mu1, mu2))
    _close(clean_d + bad_d + mu1 + mu2 + refined)
    assert len(same) == len(Ps) and all(same), same
    assert len(records) == 2 and records[0]["delta"] == records[1]["delta"] == delta and records[0]["coverage"] == 1.0
    assert _u64(records[1]["coverage"])[()] == _u64(cover)[()] and _u64(records[1]["inlier_mass"])[()] == _u64(mass)[()]
    assert np.allclose(records[1]["rejected_share"], share, rtol=1e-12) and int(np.argmax(records[0]["rejected_share"])) == BAD_VIEW
    assert below and second < first, (first, second)


# ---- 9: errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors(gpu_ctx, oracle_mod):
    """In the stated order: evaluate_weighted_robust[_pairs]' own first, in their order, then the views list;
    weighted_robust_map_weights before any map call.  Nothing written."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib
    L = _lib.lib()
    c = _Case(gpu_ctx, "d")
    try:
        ws = c.weight_dtrs(c.weights)
        m = c.metric("auto", ws)
        delta = float(R.case_delta("d", "p90"))
        handles = (C.c_void_p * c.n)()
        assert L.ecc_metric_weighted_robust_map_weights(m._h, 1.0, 1.0, handles) == 1 and b"no weighted robust map held" in L.ecc_last_error()
        with pytest.raises(E.EccError):
            m.weighted_robust_map_weights()
        bins = c.n_t * c.n_alpha
        value, cover, mass = C.c_double(-1.0), C.c_double(-1.0), C.c_double(-1.0)
        terms, hits, rej = np.full((c.N, 4), -1.0, np.float32), np.full(c.n * bins, -1.0, np.float32), np.full(c.n * bins, -1.0, np.float32)
        out = (C.c_void_p(hits.ctypes.data), C.c_void_p(rej.ctypes.data), C.byref(value), C.byref(cover), C.byref(mass), C.c_void_p(terms.ctypes.data))
        idx = _all_pairs_list(c.n)
        pidx = C.c_void_p(idx.ctypes.data)

        def both(h, loss, d, views, k, outs=out, lst=pidx, count=len(idx)):
            v = None if views is None else C.c_void_p(np.ascontiguousarray(views, np.int32).ctypes.data)
            return (L.ecc_metric_evaluate_weighted_robust_map(h, loss, d, v, k, *outs),
                    L.ecc_metric_evaluate_weighted_robust_map_pairs(h, lst, count, loss, d, v, k, *outs))
        for views, k in (([0, 1, 1], 3), ([3, 3], 2), ([0, c.n], 2), ([-1], 1), ([0], -1), (None, 2)):   # (c.n: a weight intermediate is no view)
            assert both(m._h, 0, delta, views, k) == (1, 1), (views, k)
        L.ecc_metric_evaluate_weighted_robust_map(m._h, 0, delta, C.c_void_p(np.array([3, 3], np.int32).ctypes.data), 2, *out)
        assert b"listed twice" in L.ecc_last_error()
        assert both(m._h, 7, delta, [3, 3], 2) == (1, 1) and b"loss" in L.ecc_last_error()          # the loss comes before the list
        assert both(m._h, 0, -1.0, [0, c.n], 2) == (1, 1) and b"delta" in L.ecc_last_error()
        no_value = (out[0], out[1], None, out[3], out[4], out[5])
        assert both(m._h, 0, delta, None, 0, outs=no_value) == (1, 1) and b"value is null" in L.ecc_last_error()
        assert both(m._h, 7, -1.0, [3, 3], 2, outs=no_value) == (1, 1) and b"value is null" in L.ecc_last_error()   # value < loss < delta
        assert L.ecc_metric_evaluate_weighted_robust_map_pairs(m._h, pidx, -1, 7, delta, None, 0, *no_value) == 1
        assert L.ecc_last_error() == b"negative list length"                                       # the list's own checks first
        assert L.ecc_metric_evaluate_weighted_robust_map_pairs(m._h, None, 2, 7, delta, None, 0, *no_value) == 1
        assert L.ecc_last_error() == b"index list is null"
        bad = np.concatenate([idx[:3], [[0, 1, c.n, 1]]]).astype(np.int32)                          # a data index that is a weight's
        assert L.ecc_metric_evaluate_weighted_robust_map_pairs(m._h, C.c_void_p(bad.ctypes.data), 4, 0, delta,
                                                               C.c_void_p(np.array([3, 3], np.int32).ctypes.data), 2, *out) == 1
        assert b"invalid indices" in L.ecc_last_error()                                             # a bad tuple before the views list
        m.useCorrelation(True)
        assert both(m._h, 0, delta, [3, 3], 2) == (5, 5)                                            # ECC_ERR_UNSUPPORTED, before the list
        m.useCorrelation(False)
        plain = c.metric("auto", [])                                                                # n intermediates: no weights
        assert both(plain._h, 0, delta, [3, 3], 2) == (1, 1) and b"2 * n_views" in L.ecc_last_error()
        plain.close()
        assert value.value == -1.0 and cover.value == -1.0 and mass.value == -1.0
        assert np.all(terms == -1.0) and np.all(hits == -1.0) and np.all(rej == -1.0)
        assert L.ecc_metric_weighted_robust_map_weights(m._h, 1.0, 1.0, handles) == 1              # still no map: every call above failed
        got = m.evaluate_weighted_robust_map(E.LOSS_HUBER, delta, want_pairs=True)
        want = m.evaluate_weighted_robust(E.LOSS_HUBER, delta, want_pairs=True)
        assert _same_scalars(got, want) and np.array_equal(_u32(got[5]), _u32(want[3]))
        for min_hits, gain in ((-1.0, 1.0), (1.0, -0.5), (float("nan"), 1.0), (1.0, float("inf"))):
            assert L.ecc_metric_weighted_robust_map_weights(m._h, min_hits, gain, handles) == 1, (min_hits, gain)
        assert L.ecc_metric_weighted_robust_map_weights(m._h, 1.0, 1.0, None) == 1
        assert all(h is None for h in handles)
        empty = m.evaluate_weighted_robust_map_pairs(np.zeros((0, 4), np.int32), E.LOSS_HUBER, delta)   # an empty list: zeros, no map held
        assert not empty[3].any() and not empty[4].any()
        with pytest.raises(E.EccError):
            m.weighted_robust_map_weights()
        m.close()
    finally:
        c.close()
