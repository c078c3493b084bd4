"""ecc_metric_evaluate_weighted_robust[_pairs] on the GPU (csrc/ecc_weighted_robust.hip, csrc/weighted_robust_kernel.hip): line
weights and the robust loss together.  The cases are weighted_terms.CASES with weighted_terms.case_inputs' weights -- the geometries,
grids and settings that select each kernel and loop (labels a .. j); each oracle case asserts from the
records of a single-channel metric that it reached its loop class, as tests/test_gpu_weighted.py does.

  1 infinite scale  delta = +inf and FLT_MAX, every loss: {c, u}, value and coverage have the bits of evaluate_weighted, k the bits
                    of u, inlier_mass == 1.0; r has the same bits for every loss and delta;
  2 weights of one  {c, k, r}, value and inlier_mass have the bits of evaluate_robust on the n-metric over the same data, u == 1;
                    with delta = inf as well the bits of evaluate(); the list form; weighted_robust_scale == robust_scale;
  3 oracle          {c, u, k, r} of every pair against weighted_robust_terms at both scales of the case and for all three losses
                    (tests/test_weighted_robust_terms_oracle.py shows that this comparison rejects the slips it is there for and
                    that the cases exercise both mechanisms in the same pair), the three means to 1e-5;
  4 one view out    W_v = 0, 1 elsewhere, finite delta;
  5 weight 0        data that differ only on lines of weight 0 give the same bits;
  6 both at once    the reason the call exists: one block flagged, one block nobody flagged;
  7 - 9             the list form's edges, repeatability and nothing else moved, every documented error."""
import ctypes as C

import numpy as np
import pytest

import channel_terms as T
import robust_terms as R
import weighted_terms as W
import weighted_robust_terms as WR
from test_gpu_weighted import BLOCK, _Case, _flag

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
LOSS_CODES = {"huber": 0, "truncated": 1, "geman_mcclure": 2}
LABELS = sorted(WR.CASES)


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _close(dtrs):
    for d in dtrs:
        d.close()


def _pair_order(cost):
    n = cost.shape[0]
    iu = np.triu_indices(n, 1)
    return cost[iu[1], iu[0]].copy()


def _all_pairs_list(n):
    iu = np.triu_indices(n, 1)   # get_ij order: i < j, i slow
    return np.ascontiguousarray(np.stack([iu[0], iu[1], iu[0], iu[1]], axis=1), np.int32)


def _same(x, y):
    """Two results (value, coverage, inlier_mass, rows): the same bits."""
    return all(_u64(a)[()] == _u64(b)[()] for a, b in zip(x[:3], y[:3])) and np.array_equal(_u32(x[3]), _u32(y[3]))


def _ones(case):
    return case.weight_dtrs([np.ones((case.n_t, case.n_alpha), np.float32)] * case.n)


@pytest.fixture
def case(gpu_ctx, oracle_mod, request):
    c = _Case(gpu_ctx, request.param)
    try:
        yield c
    finally:
        c.close()


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LABELS, indirect=True)
def test_an_infinite_scale_is_evaluate_weighted_bit_for_bit(case):
    """delta = +inf and delta = FLT_MAX (no |d| exceeds either: every w is 1.0f, f == mu), for every loss, in every case and sampling
    setup of the table, with the case's weights: rows {c, u} have the bits of evaluate_weighted's rows, k the bits of u, value and
    coverage the bits of evaluate_weighted, inlier_mass == 1.0.  r has the same bits for every loss and delta, a finite one
    included."""
    ws = case.weight_dtrs(case.weights)
    finite = float(R.case_delta(case.label, "median"))
    for sampling, _ in case.setups:
        m = case.metric(sampling, ws)
        w_value, w_cover, w_rows = m.evaluate_weighted(want_pairs=True)
        assert 0.0 < w_cover < 1.0 and w_value > 0.0
        rows_r = None
        for loss in WR.LOSSES:
            for delta in (float("inf"), FLT_MAX, finite):
                value, cover, mass, rows = m.evaluate_weighted_robust(LOSS_CODES[loss], delta, want_pairs=True)
                where = (sampling, loss, delta)
                assert rows.shape == (case.N, 4) and rows.dtype == np.float32
                if rows_r is None:
                    rows_r = rows[:, 3].copy()
                    assert np.all(rows_r >= 0.0) and np.all((rows_r > 0) == (w_rows[:, 0] > 0)), where
                assert np.array_equal(_u32(rows[:, 3]), _u32(rows_r)), where          # r: no loss and no delta in it
                assert np.array_equal(_u32(rows[:, 1]), _u32(w_rows[:, 1])) and _u64(cover)[()] == _u64(w_cover)[()], where
                if delta == finite:
                    assert np.all(rows[:, 2] <= rows[:, 1]) and mass < 1.0 and value < w_value, where
                    continue
                assert np.array_equal(_u32(rows[:, 0]), _u32(w_rows[:, 0])), (where, np.max(np.abs(rows[:, 0] - w_rows[:, 0])))
                assert np.array_equal(_u32(rows[:, 2]), _u32(rows[:, 1])), where
                assert _u64(value)[()] == _u64(w_value)[()] and mass == 1.0, (where, value, w_value, mass)
        m.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LABELS, indirect=True)
def test_weights_of_one_are_evaluate_robust_bit_for_bit(case):
    """All weights 1.0f (weight intermediates of ones made with FILTER_NONE; f == w), at both scales of the case and for all losses:
    {c, k, r} have the bits of evaluate_robust's {c, u, r} on the n-metric over the same data, u == 1.0 and coverage == 1.0, value and
    inlier_mass have evaluate_robust's bits, weighted_robust_scale equals robust_scale.  With delta = inf as well the results have the
    bits of evaluate() and evaluate(cost).  The list form with the tuples (i, j, i, j) of all pairs has the bits of the all-pairs rows
    and of evaluate_robust_pairs of that list (the same length, so the same resolved mode)."""
    E = case.E
    ones = _ones(case)
    idx = _all_pairs_list(case.n)
    for sampling, _ in case.setups:
        m2, m1 = case.metric(sampling, ones), case.metric(sampling, [])
        for loss in WR.LOSSES:
            for delta in (R.case_delta(case.label, "median"), R.case_delta(case.label, "p90"), float("inf")):
                where = (sampling, loss, delta)
                value, cover, mass, rows = m2.evaluate_weighted_robust(LOSS_CODES[loss], delta, want_pairs=True)
                r_value, r_mass, r_rows = m1.evaluate_robust(LOSS_CODES[loss], delta, want_pairs=True)
                assert np.array_equal(_u32(rows[:, (0, 2, 3)]), _u32(r_rows)), where
                assert np.all(rows[:, 1] == 1.0) and cover == 1.0, where
                assert _u64(value)[()] == _u64(r_value)[()] and _u64(mass)[()] == _u64(r_mass)[()], (where, value, r_value, mass, r_mass)
                assert E.weighted_robust_scale(rows) == E.robust_scale(r_rows) > 0.0, where
                assert E.weighted_robust_scale(rows, 0.5) == E.robust_scale(r_rows, 0.5), where
                lst = m2.evaluate_weighted_robust_pairs(idx, LOSS_CODES[loss], delta, want_pairs=True)
                l_value, l_mass, l_rows = m1.evaluate_robust_pairs(idx, LOSS_CODES[loss], delta, want_pairs=True)
                assert np.array_equal(_u32(lst[3]), _u32(rows)) and np.array_equal(_u32(lst[3][:, (0, 2, 3)]), _u32(l_rows)), where
                assert _u64(lst[0])[()] == _u64(l_value)[()] and lst[1] == 1.0 and _u64(lst[2])[()] == _u64(l_mass)[()], where
                if np.isinf(delta):
                    plain = m1.evaluate()
                    cost = np.full((case.n, case.n), -2.0, np.float32)
                    with_cost = m1.evaluate(cost)
                    assert np.array_equal(_u32(rows[:, 0]), _u32(_pair_order(cost))), where
                    assert _u64(value)[()] == _u64(plain)[()] == _u64(with_cost)[()] and mass == 1.0, (where, value, plain)
                    assert np.all(rows[:, 2] == 1.0), where
                else:
                    assert mass < 1.0, where
        m2.close()
        m1.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LABELS, indirect=True)
def test_pair_terms_against_the_direct_oracle(case):
    """{c, u, k, r} of every pair (case e: the oracle's sample of the pairs) against the float64 statement, at both scales of the case
    and for all three losses: 1e-6 of the scale under the reference arithmetic, 1e-3 on the throughput paths -- the scale s = w06 sum
    d^2 for c, 1 for u and k, the unweighted raw mean for r; value, coverage and inlier_mass to 1e-5 relative.  The worst ratios of a
    GPU run are recorded in DESIGN.md 4.23."""
    ws = case.weight_dtrs(case.weights)
    failures = []
    for sampling, _ in case.setups:
        rec = case.reached(sampling, W.case_terms(case.label))
        assert np.max(np.abs(rec["kmax"] - case.K01s[:, 15])) <= 1e-3   # the records describe the oracle's ranges, in its pair order
        tol = T.tolerance(sampling, case.N)
        m = case.metric(sampling, ws)
        for scale in WR.SCALES:
            delta = R.case_delta(case.label, scale)
            for loss in WR.LOSSES:
                t = WR.case_terms(case.label, loss, scale)
                listed = t["pairs"]
                want, scales = WR.columns(t)
                value, cover, mass, rows = m.evaluate_weighted_robust(LOSS_CODES[loss], delta, want_pairs=True)
                assert np.all(np.isfinite(rows)) and np.isfinite(value)
                assert np.all(rows[:, 1] >= 0.0) and np.all(rows[:, 1] <= 1.0) and np.all(rows[:, 2] <= rows[:, 1])
                ratio = T.compare(rows[listed], want, scales, tol)
                line = "case %s %-10s %-13s %-6s (delta %.6g): c %.3g of the bar %.0e, u %.3g, k %.3g, r %.3g" % (
                    case.label, sampling, loss, scale, delta, ratio[0], tol, ratio[1], ratio[2], ratio[3])
                if tol == T.TOL_THROUGHPUT:   # reported: the same against the float64-position statement
                    c64, _ = WR.columns(WR.case_terms(case.label, loss, scale, "float64"))
                    r64 = T.compare(rows[listed], c64, scales, tol)
                    line += "; against float64 positions c %.3g, u %.3g, k %.3g, r %.3g" % (r64[0], r64[1], r64[2], r64[3])
                if "value" in t:
                    em = np.abs(np.array([value, cover, mass]) - WR.means(t)) / (T.TOL_MEAN * WR.means(t))
                    line += "; value %.3g of the bar 1e-05, coverage %.3g, inlier mass %.3g" % (em[0], em[1], em[2])
                    ratio = np.append(ratio, em)
                print(line)
                if not ratio.max() <= 1.0:
                    failures.append(line)
        m.close()
    assert not failures, "\n".join(failures)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LABELS, indirect=True)
def test_an_excluded_view(case):
    """W_v = 0 for one view and 1 elsewhere, at the finite median scale of the case, every loss: the pairs with v are {0, 0, 0, 0},
    every other pair has the bits of the all-ones rows (test 2's: evaluate_robust's), value equals the float64 mean of c over the
    other pairs to 1e-12 relative, coverage is their share of the pairs."""
    v = case.n // 3
    fields = [np.ones((case.n_t, case.n_alpha), np.float32)] * case.n
    fields[v] = np.zeros((case.n_t, case.n_alpha), np.float32)
    ws, ones = case.weight_dtrs(fields), _ones(case)
    iu = np.triu_indices(case.n, 1)
    hit = (iu[0] == v) | (iu[1] == v)
    assert hit.sum() == case.n - 1
    delta = R.case_delta(case.label, "median")
    for sampling, _ in case.setups:
        m, m_ones = case.metric(sampling, ws), case.metric(sampling, ones)
        for loss in WR.LOSSES:
            value, cover, mass, rows = m.evaluate_weighted_robust(LOSS_CODES[loss], delta, want_pairs=True)
            _, _, _, full = m_ones.evaluate_weighted_robust(LOSS_CODES[loss], delta, want_pairs=True)
            assert np.all(rows[hit] == 0.0), (sampling, loss, rows[hit])
            assert np.array_equal(_u32(rows[~hit]), _u32(full[~hit])) and np.all(rows[~hit, 1] == 1.0), (sampling, loss)
            mean = full[~hit, 0].astype(np.float64).mean()
            kept = full[~hit, 2].astype(np.float64).mean()
            assert abs(value - mean) <= 1e-12 * mean and abs(mass - kept) <= 1e-12, (sampling, loss, value, mean, mass, kept)
            assert abs(cover - (~hit).sum() / case.N) <= 1e-15 and 0.0 < mass < 1.0, (sampling, loss, cover, mass)
        m.close()
        m_ones.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
BUMP = 1.0e15          # finite, and its square is: r's product mu * (d * d) is 0 * 1e30
TINY_DELTA = 1.0e-6    # s = |d| / delta = 1e21: s * s overflows, Geman-McClure's w is 1 / inf = 0


@pytest.mark.parametrize("label, sampling", [("d", "reference"), ("d", "polynomial"), ("d", "per_sample"), ("i", "polynomial")])
def test_data_on_lines_of_weight_zero_do_not_count(gpu_ctx, oracle_mod, label, sampling):
    """One view's weights are 0 on a band of bins -- the central half of the distances at every angle, which the fold (alpha + pi, -t)
    maps to itself -- and 1 elsewhere; a second copy of its data has BUMP added inside the band, two bins (the bilinear taps and the
    fold's rounding) away from its edges.  At the finite median scale and at TINY_DELTA, for all three losses,
    both scans give the same bits: f = 0 * w with w finite -- Huber's and the truncated loss's w is tiny but positive there,
    Geman-McClure's is exactly 0 at TINY_DELTA, where s * s overflows.  The bump does reach the samples: under weights of one the
    rows of that view's pairs change."""
    import epipolarconsistency_amd as E
    c = _Case(gpu_ctx, label)
    try:
        v = 2
        box = (slice(c.n_t // 4, 3 * c.n_t // 4), slice(None))   # (n_t, n_alpha) fields: the central half of the distances, every angle
        inner = (slice(box[0].start + 2, box[0].stop - 2), slice(None))
        fields = [np.ones((c.n_t, c.n_alpha), np.float32) for _ in range(c.n)]
        fields[v][box] = 0.0
        bumped = np.array(c.host[v], np.float32)
        bumped[inner] += np.float32(BUMP)
        assert np.all(np.isfinite(bumped)) and np.all(np.isfinite(bumped.astype(np.float32) ** 2))
        kw = {} if c.derivative else dict(filter=E.FILTER_NONE)
        bad_v = E.RadonIntermediate.from_host(gpu_ctx, bumped, c.n_u, c.n_v, **kw)
        c.made.append(bad_v)
        bad_data = c.data[:v] + [bad_v] + c.data[v + 1:]
        ws, ones = c.weight_dtrs(fields), _ones(c)

        def metric(data, weights):
            m = E.MetricRadonIntermediate(gpu_ctx, c.Ps, data + weights).setSampling(sampling)
            m.setObjectRadius(c.radius)
            m.setEpipolarPlaneStep(c.dkappa)
            return m
        m_clean, m_bad, m_seen = metric(c.data, ws), metric(bad_data, ws), metric(bad_data, ones)
        iu = np.triu_indices(c.n, 1)
        hit = (iu[0] == v) | (iu[1] == v)
        for delta in (float(R.case_delta(label, "median")), TINY_DELTA):
            for loss in WR.LOSSES:
                clean = m_clean.evaluate_weighted_robust(LOSS_CODES[loss], delta, want_pairs=True)
                bad = m_bad.evaluate_weighted_robust(LOSS_CODES[loss], delta, want_pairs=True)
                assert np.all(np.isfinite(bad[3])) and np.all(np.isfinite(bad[:3])), (loss, delta)
                assert _same(clean, bad), (loss, delta, np.max(np.abs(clean[3] - bad[3]), axis=0))
                assert clean[3][hit, 1].max() < 1.0 and np.all(clean[3][~hit, 1] == 1.0) and clean[0] > 0.0
                seen = m_seen.evaluate_weighted_robust(LOSS_CODES[loss], delta, want_pairs=True)[3]
                assert np.all(seen[hit, 3] > 1e20), (loss, delta)     # under weights of one the bump is in every pair of the view
        for m in (m_clean, m_bad, m_seen):
            m.close()
    finally:
        c.close()


# ---- 6: the reason the call exists -----------------------------------------------------------------------------------------------
FLAGGED_VIEW, UNFLAGGED_VIEW = 3, 6


@pytest.fixture(scope="module")
def two_blocks(gpu_ctx, small_scan):
    """8 views of the spheres at 128^2 -> 96^2 bins, on the device: the clean scan, and a corrupted one with the opaque block of
    tests/test_gpu_weighted.py in view 3 -- flagged: its line weights come from line_weights, ones elsewhere -- and the same block in
    view 6, flagged nowhere.  Made once for the module."""
    import epipolarconsistency_amd as E
    imgs, B = small_scan["imgs"], 96
    bad = np.array(imgs, np.float32)
    for view in (FLAGGED_VIEW, UNFLAGGED_VIEW):
        bad[view][BLOCK] += 4.0 * float(np.max(imgs[view]))
    clean_d = E.RadonIntermediate.compute_batch(gpu_ctx, np.asarray(imgs, np.float32), B, B)
    bad_d = E.RadonIntermediate.compute_batch(gpu_ctx, bad, B, B)
    ones = [E.RadonIntermediate.from_host(gpu_ctx, np.ones((B, B), np.float32), 128, 128, filter=E.FILTER_NONE) for _ in range(len(imgs))]
    w3 = E.line_weights(gpu_ctx, _flag(imgs[0].shape), B, B, guard_bins=1)
    ws = ones[:FLAGGED_VIEW] + [w3] + ones[FLAGGED_VIEW + 1:]
    yield dict(clean=clean_d, bad=bad_d, ws=ws)
    _close(clean_d + bad_d + ones + [w3])


@pytest.mark.parametrize("sampling", ["polynomial", "per_sample", "auto"])
def test_one_block_flagged_and_one_nobody_flagged(gpu_ctx, small_scan, two_blocks, sampling):
    """Under the same weights the pairs that contain neither view 3 nor view 6 keep their bits against the clean scan, for every loss.
    With the truncated loss at delta = weighted_robust_scale(the corrupted scan's rows at delta = inf, 0.5), corrupted / clean of the
    combined call is strictly smaller than corrupted / clean of evaluate_weighted, which still has the unflagged block in it.
    Printed: both ratios and that of evaluate_robust (same loss and delta) on the n-metric, which has both blocks to deal with.  No
    ratio is fixed in advance; a run's figures are in DESIGN.md 4.23 and the README."""
    import epipolarconsistency_amd as E
    Ps, n, b = small_scan["Ps"], len(small_scan["Ps"]), two_blocks
    iu = np.triu_indices(n, 1)
    hit = np.isin(iu[0], (FLAGGED_VIEW, UNFLAGGED_VIEW)) | np.isin(iu[1], (FLAGGED_VIEW, UNFLAGGED_VIEW))
    m_bad = E.MetricRadonIntermediate(gpu_ctx, Ps, b["bad"] + b["ws"]).setSampling(sampling)
    m_clean = E.MetricRadonIntermediate(gpu_ctx, Ps, b["clean"] + b["ws"]).setSampling(sampling)
    n_bad = E.MetricRadonIntermediate(gpu_ctx, Ps, b["bad"]).setSampling(sampling)
    n_clean = E.MetricRadonIntermediate(gpu_ctx, Ps, b["clean"]).setSampling(sampling)
    at_inf = m_bad.evaluate_weighted_robust(E.LOSS_TRUNCATED, float("inf"), want_pairs=True)
    w_bad, w_clean = m_bad.evaluate_weighted(), m_clean.evaluate_weighted()
    assert _u64(at_inf[0])[()] == _u64(w_bad[0])[()] and _u64(at_inf[1])[()] == _u64(w_bad[1])[()] and w_bad[1] < 1.0
    delta = E.weighted_robust_scale(at_inf[3], 0.5)
    assert delta > 0.0
    for loss in WR.LOSSES:
        bad = m_bad.evaluate_weighted_robust(LOSS_CODES[loss], delta, want_pairs=True)
        clean = m_clean.evaluate_weighted_robust(LOSS_CODES[loss], delta, want_pairs=True)
        assert np.array_equal(_u32(bad[3][~hit]), _u32(clean[3][~hit])), loss
        assert not np.array_equal(_u32(bad[3][hit]), _u32(clean[3][hit])), loss
        assert _u64(bad[1])[()] == _u64(clean[1])[()], loss                       # the coverage is the weights' alone
        if loss == "truncated":
            combined = bad[0] / clean[0]
            masses = (clean[2], bad[2])
    weighted = w_bad[0] / w_clean[0]
    robust = n_bad.evaluate_robust(E.LOSS_TRUNCATED, delta)[0] / n_clean.evaluate_robust(E.LOSS_TRUNCATED, delta)[0]
    plain = n_bad.evaluate() / n_clean.evaluate()
    print("%s: delta %.6g, coverage %.4f; corrupted / clean: combined %.4g (inlier mass %.4f -> %.4f), evaluate_weighted %.4g, "
          "evaluate_robust %.4g, evaluate() %.4g" % (sampling, delta, w_bad[1], combined, masses[0], masses[1], weighted, robust, plain))
    for m in (m_bad, m_clean, n_bad, n_clean):
        m.close()
    assert weighted > 1.0 and combined < weighted, (combined, weighted)


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
def test_edge_cases_of_the_list_form(gpu_ctx, oracle_mod):
    """n_pairs == 0: ECC_OK and nothing written; a tuple with P0 == P1 has no samples, {0, 1, 1, 0}, and counts in the sums; a repeated
    tuple carries its row twice; the weight follows D and not P; a D index equal to n_views is an error with nothing written."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib
    c = _Case(gpu_ctx, "d")
    try:
        gone = 2
        fields = [np.ones((c.n_t, c.n_alpha), np.float32)] * c.n
        fields[gone] = np.zeros((c.n_t, c.n_alpha), np.float32)
        m = c.metric("reference", c.weight_dtrs(c.weights))   # fixed, so that every list length resolves alike
        delta = R.case_delta("d", "median")
        _, _, _, rows = m.evaluate_weighted_robust(E.LOSS_TRUNCATED, delta, want_pairs=True)
        value, cover, mass, terms = C.c_double(-1.0), C.c_double(-1.0), C.c_double(-1.0), np.full(4, -1.0, np.float32)
        out = (C.byref(value), C.byref(cover), C.byref(mass), C.c_void_p(terms.ctypes.data))
        idx1 = np.array([[0, 1, 0, 1]], np.int32)
        for lst in (None, C.c_void_p(idx1.ctypes.data)):
            assert _lib.lib().ecc_metric_evaluate_weighted_robust_pairs(m._h, lst, 0, E.LOSS_TRUNCATED, float(delta), *out) == 0
        bad1 = np.array([[0, 1, 0, c.n]], np.int32)           # D1 == n_views: the first weight intermediate is no data
        assert _lib.lib().ecc_metric_evaluate_weighted_robust_pairs(m._h, C.c_void_p(bad1.ctypes.data), 1, E.LOSS_TRUNCATED, float(delta), *out) == 1
        assert value.value == -1.0 and cover.value == -1.0 and mass.value == -1.0 and np.all(terms == -1.0)
        assert m.evaluate_weighted_robust_pairs(np.zeros((0, 4), np.int32), E.LOSS_TRUNCATED, delta, want_pairs=True)[3].shape == (0, 4)
        full = _all_pairs_list(c.n)
        pick = np.array([5, 0, 17, 5, 9])                     # pair 5 twice
        idx = np.concatenate([full[pick], [[2, 2, 2, 3]]]).astype(np.int32)
        v, u, k, p = m.evaluate_weighted_robust_pairs(idx, E.LOSS_TRUNCATED, delta, want_pairs=True)
        assert np.array_equal(_u32(p[:5]), _u32(rows[pick])) and np.array_equal(_u32(p[0]), _u32(p[3])), p
        assert np.array_equal(p[5], [0.0, 1.0, 1.0, 0.0]), p
        sums = p.astype(np.float64).sum(axis=0)
        assert abs(v - sums[0] / sums[1]) <= 1e-12 * v and abs(u - sums[1] / 6) <= 1e-15 and abs(k - sums[2] / sums[1]) <= 1e-15
        m.close()
        m = c.metric("reference", c.weight_dtrs(fields))
        follows = np.array([[0, 1, gone, 3], [gone, 3, 0, 1], [0, 1, 0, 1]], np.int32)
        _, _, _, p = m.evaluate_weighted_robust_pairs(follows, E.LOSS_HUBER, delta, want_pairs=True)
        assert np.all(p[0] == 0.0), p[0]                      # the data -- and so the weights -- of the view that is out
        assert p[1, 1] == 1.0 and p[1, 0] > 0.0 and p[2, 1] == 1.0, p   # its matrix alone: all weights 1
        m.close()
    finally:
        c.close()


def test_all_weights_zero(gpu_ctx, oracle_mod):
    """sum u == 0: value, coverage and inlier_mass are 0.0, no error."""
    c = _Case(gpu_ctx, "d")
    try:
        m = c.metric("auto", c.weight_dtrs([np.zeros((c.n_t, c.n_alpha), np.float32)] * c.n))
        value, cover, mass, rows = m.evaluate_weighted_robust(0, R.case_delta("d", "median"), want_pairs=True)
        lst = m.evaluate_weighted_robust_pairs(_all_pairs_list(c.n)[:5], 0, R.case_delta("d", "median"))
        m.close()
        assert (value, cover, mass) == (0.0, 0.0, 0.0) and np.all(rows == 0.0) and lst == (0.0, 0.0, 0.0)
    finally:
        c.close()


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
def test_repeatable_and_nothing_else_moved(gpu_ctx, oracle_mod):
    """Two calls give identical bits; evaluate() (with one view moved and back), an incremental evaluation after a moved view, a
    pose-delta batch and evaluate_weighted on the same metric keep their bits around calls of both forms."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import geometry as Gm
    c = _Case(gpu_ctx, "i")
    try:
        n = c.n
        m = c.metric("polynomial", c.weight_dtrs(c.weights))
        delta = R.case_delta("i", "median")
        idx = _all_pairs_list(n)[::3]
        P0 = E.pack_projection_matrices(c.Ps)
        P1 = P0.copy()
        P1[n // 2] = E.pack_projection_matrices([Gm.compose_transform(P0[n // 2].reshape(4, 3).T, Gm.rigid_transform(tx=3.0, ry=0.01))])[0]

        def observe(between=lambda: None):
            base = m.setProjectionMatrices(P0).evaluate()
            moved = m.setProjectionMatrices(P1).evaluate()
            back = m.setProjectionMatrices(P0).evaluate()
            m.setIncremental(True)
            kept = m.evaluate()
            between()                                           # (with values kept on the device for the incremental mode)
            inc = m.setProjectionMatrices(P1).evaluate()
            inc_back = m.setProjectionMatrices(P0).evaluate()
            m.setIncremental(False)
            deltas = m.evaluate_pose_deltas([n // 2, 1], np.stack([P1[n // 2], P0[2]]))
            weighted = m.evaluate_weighted(want_pairs=True)
            cost = np.zeros((n, n), np.float32)
            with_cost = m.evaluate(cost)
            return np.concatenate([[base, moved, back, kept, inc, inc_back, with_cost], np.ravel(deltas), weighted[:2]]), cost, weighted[2]
        before, cost_b, wp_b = observe()
        assert _u64(before[4])[()] == _u64(before[1])[()] and _u64(before[5])[()] == _u64(before[0])[()]
        first = m.evaluate_weighted_robust(E.LOSS_HUBER, delta, want_pairs=True)
        second = m.evaluate_weighted_robust(E.LOSS_HUBER, delta, want_pairs=True)
        lfirst = m.evaluate_weighted_robust_pairs(idx, E.LOSS_GEMAN_MCCLURE, delta, want_pairs=True)
        lsecond = m.evaluate_weighted_robust_pairs(idx, E.LOSS_GEMAN_MCCLURE, delta, want_pairs=True)
        after, cost_a, wp_a = observe(lambda: (m.evaluate_weighted_robust(E.LOSS_HUBER, delta),
                                               m.evaluate_weighted_robust_pairs(idx, E.LOSS_GEMAN_MCCLURE, delta)))
        assert np.array_equal(_u64(before), _u64(after)) and np.array_equal(_u32(cost_b), _u32(cost_a)) and np.array_equal(_u32(wp_b), _u32(wp_a))
        assert _same(first, second) and _same(lfirst, lsecond)
        assert m.evaluate_weighted_robust(E.LOSS_HUBER, delta) == first[:3]   # without the pair terms: the same three numbers
        assert first[2] < 1.0 and first[1] < 1.0 and first[0] < before[-2]
        # in the middle of a sequence: matrices moved, then the call, then back
        m.setProjectionMatrices(P1).evaluate()
        moved = m.evaluate_weighted_robust(E.LOSS_HUBER, delta)
        assert _u64(m.evaluate())[()] == _u64(before[1])[()]          # the moved matrices are still current
        assert _u64(m.setProjectionMatrices(P0).evaluate())[()] == _u64(before[0])[()]
        again = m.evaluate_weighted_robust(E.LOSS_HUBER, delta, want_pairs=True)
        assert _same(again, first) and moved[0] != first[0]
        m.close()
    finally:
        c.close()


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------
def test_errors_in_the_documented_order(gpu_ctx, oracle_mod):
    """Every argument error of the header on a live metric, through the C calls themselves: the code, nothing written, and -- by the
    message -- the documented precedence: the list's own checks, then evaluate_robust's conditions in its order, use_corr, the number
    of intermediates, a bad tuple."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib
    L = _lib.lib()
    c = _Case(gpu_ctx, "d")
    try:
        ws = c.weight_dtrs(c.weights)
        m = c.metric("auto", ws)
        delta = float(R.case_delta("d", "p90"))
        want = m.evaluate_weighted_robust(E.LOSS_HUBER, delta, want_pairs=True)
        value, cover, mass, terms = C.c_double(-1.0), C.c_double(-1.0), C.c_double(-1.0), np.full((c.N, 4), -1.0, np.float32)
        out = (C.byref(value), C.byref(cover), C.byref(mass), C.c_void_p(terms.ctypes.data))
        idx = _all_pairs_list(c.n)
        pidx = C.c_void_p(idx.ctypes.data)

        def both(h, loss, d, outs=out, lst=pidx, count=len(idx)):
            a = L.ecc_metric_evaluate_weighted_robust(h, loss, d, *outs)
            b = L.ecc_metric_evaluate_weighted_robust_pairs(h, lst, count, loss, d, *outs)
            return (a, b)

        def pairs(h, lst, count, loss, d, outs=out):
            return L.ecc_metric_evaluate_weighted_robust_pairs(h, lst, count, loss, d, *outs), L.ecc_last_error()
        no_value = (None, out[1], out[2], out[3])
        assert both(m._h, 0, delta, outs=no_value) == (1, 1) and b"value is null" in L.ecc_last_error()
        assert both(m._h, 0, delta, outs=(out[0], None, None, None)) == (0, 0)                   # coverage, inlier_mass, terms: nullable
        value.value = -1.0
        for loss in (-1, 3, 100):
            assert both(m._h, loss, delta) == (1, 1) and b"loss" in L.ecc_last_error(), loss
        for d in (0.0, -1.0, float("nan"), float("-inf")):
            assert both(m._h, 0, d) == (1, 1) and b"delta" in L.ecc_last_error(), d
        assert pairs(m._h, None, 2, 0, delta) == (1, b"index list is null")
        assert pairs(m._h, pidx, -1, 0, delta) == (1, b"negative list length")
        for bad in ([0, c.n, 0, 1], [-1, 1, 0, 1], [0, 1, c.n, 1], [0, 1, 0, -1], [0, 1, 2 * c.n - 1, 1]):   # a bad tuple, behind good ones
            lst = np.concatenate([idx[:3], [bad]]).astype(np.int32)
            code, text = pairs(m._h, C.c_void_p(lst.ctypes.data), 4, 0, delta)
            assert code == 1 and b"invalid indices" in text, bad
            assert text.endswith(b"(matrices and data intermediates lie in [0, n_views))")      # the weighted lists' own text
        # the precedence: list checks < value < loss < delta < use_corr < the number of intermediates < a bad tuple
        lst = np.array([[0, 1, 0, c.n]], np.int32)
        plst = C.c_void_p(lst.ctypes.data)
        assert pairs(m._h, None, -1, 7, -1.0, no_value)[1] == b"negative list length"
        assert pairs(m._h, None, 1, 7, -1.0, no_value)[1] == b"index list is null"
        assert pairs(m._h, plst, 1, 7, -1.0, no_value)[1] == b"value is null"
        assert b"loss" in pairs(m._h, plst, 1, 7, -1.0)[1]
        assert b"delta" in pairs(m._h, plst, 1, 0, -1.0)[1]
        assert b"loss" in pairs(m._h, None, 0, 7, delta)[1] and b"delta" in pairs(m._h, None, 0, 0, -1.0)[1]   # an empty list: the checks first
        m.useCorrelation(True)
        assert pairs(m._h, None, 0, 0, delta)[0] == 5
        assert both(m._h, 0, delta) == (5, 5)                                                   # ECC_ERR_UNSUPPORTED
        assert pairs(m._h, plst, 1, 0, delta)[0] == 5 and b"delta" in pairs(m._h, plst, 1, 0, -1.0)[1]
        with pytest.raises(E.EccError) as e:
            m.evaluate_weighted_robust(E.LOSS_HUBER, delta)
        assert e.value.code == 5, e.value
        m.useCorrelation(False)
        for dtrs in (c.data, c.data + ws[:-1], c.data + ws + ws[:1]):                           # n, 2 n - 1, 2 n + 1 intermediates
            other = E.MetricRadonIntermediate(gpu_ctx, c.Ps, dtrs)
            assert both(other._h, 0, delta) == (1, 1) and b"2 * n_views" in L.ecc_last_error(), len(dtrs)
            code, text = pairs(other._h, plst, 1, 0, delta)
            assert code == 1 and b"2 * n_views" in text, len(dtrs)                               # before the bad tuple
            code, text = pairs(other._h, None, 0, 0, delta)
            assert code == 1 and b"2 * n_views" in text, len(dtrs)                               # ... and before an empty list's return
            other.useCorrelation(True)
            assert both(other._h, 0, delta) == (5, 5), len(dtrs)                                # use_corr before the count
            with pytest.raises(E.EccError) as e:
                other.evaluate_weighted_robust(E.LOSS_HUBER, delta)
            assert e.value.code == 5
            other.close()
        one = E.MetricRadonIntermediate(gpu_ctx, c.Ps[:1], [c.data[0], ws[0]])                  # fewer than two views
        none = E.MetricRadonIntermediate(gpu_ctx, None, c.data + ws)                            # no matrices set
        for other in (one, none):
            assert both(other._h, 0, delta, lst=pidx, count=1) == (1, 1)
            with pytest.raises(E.EccError) as e:
                other.evaluate_weighted_robust(E.LOSS_HUBER, delta)
            assert e.value.code == 1
            other.close()
        assert value.value == -1.0 and cover.value == -1.0 and mass.value == -1.0 and np.all(terms == -1.0)   # nothing written by any
        again = m.evaluate_weighted_robust(E.LOSS_HUBER, delta, want_pairs=True)
        assert _same(again, want)
        m.close()
    finally:
        c.close()
