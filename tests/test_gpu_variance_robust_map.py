"""ecc_metric_evaluate_variance_robust_map[_pairs] and ecc_metric_variance_robust_map_variances on the GPU
(csrc/ecc_variance_robust_map.hip, csrc/variance_robust_map_kernel.hip): where the robust loss rejects in sigma
units, and the held map as the next pass's variance fields.  The cases are variance_terms.CASES with their data, variance fields and
floors, as tests/test_gpu_variance_robust.py takes them.

  1 bit links       value, mean_weight, inlier_mass and the rows {c, u, k, r} equal evaluate_variance_robust / _pairs (==); V == 0.5
                    with floor <= 1: the fixed-point sums are evaluate_robust_map's on the n-metric, cell for cell; delta = inf: REJ
                    all zeros and HITS the n-metric's, whatever V is; V and the floor x 4 with delta x 1/2: both planes keep their bits;
  2 the statement   HITS and REJ per bin against variance_robust_map_terms, |got - want| / bin scale: 1e-6 under the reference
                    arithmetic, 1e-3 on the throughput paths (tests/test_variance_robust_map_terms_oracle.py shows that this
                    comparison rejects the slips); sum HITS per view against the view's sample count; at V == 0.5 sum REJ against
                    sum (u - k) 2 n_kappa from the rows;
  3 reproducible    two calls, a reversed list and four kinds of views subset: identical; a list cut in two adds up in fixed point;
  4 variances       variance_robust_map_variances against numpy bit for bit; V at max_factor 1 and at delta = inf; each of the
                    three kinds of map is refused by the other kinds' calls;
  5 the reason      the map points at the view with the instrument, the feedback makes evaluate_variance robust; refine_variances
                    returns pass 2's fields;
  6 errors."""
import ctypes as C
import functools

import numpy as np
import pytest

import channel_terms as T
import robust_map_terms as M
import robust_terms as R
import variance_robust_map_terms as VM
import variance_robust_terms as VR
import variance_terms as V
from test_gpu_variance import _Case, _close, _u32, _u64

pytestmark = pytest.mark.gpu

INF = float("inf")
LOSS_CODES = {"huber": 0, "truncated": 1, "geman_mcclure": 2}   # ECC_LOSS_* == E.LOSS_*


@pytest.fixture
def case(gpu_ctx, oracle_mod, request):
    c = _Case(gpu_ctx, request.param)
    try:
        yield c
    finally:
        c.close()


def _all_pairs_list(n):
    iu = np.triu_indices(n, 1)   # get_ij order: i < j, i slow
    return np.ascontiguousarray(np.stack([iu[0], iu[1], iu[0], iu[1]], axis=1), np.int32)


def _same_scalars(a, b, k=3):
    return all(_u64(a[q])[()] == _u64(b[q])[()] for q in range(k))


def _same_fixed(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _same_planes(a, b):
    """Two map results (value, mean_weight, inlier_mass, hits, rejected, ...): the same plane bits."""
    return np.array_equal(_u32(a[3]), _u32(b[3])) and np.array_equal(_u32(a[4]), _u32(b[4]))


# ---- 1: bit links --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["d", "e", "i", "j"], indirect=True)
def test_bit_links(case):
    """Every setup of the case and the three sampling modes, for every case: derivative data (d, e, j) and plain data (i) each pass
    through the polynomial, the per-sample and the reference loop.  Case e has 2 145 pairs (reference arithmetic: one wave per pair)
    and its list of 300 (four waves per pair).  Per loss both of variance_robust_terms' (floor, scale) pairings."""
    vs = case.variance_dtrs(case.variances)
    vs4 = case.variance_dtrs([np.float32(4.0) * f for f in case.variances])
    half = case.constant(0.5)
    setups = ["polynomial", "per_sample", "reference"] + [s for s, _ in case.setups if s not in ("polynomial", "per_sample", "reference")]
    idx = _all_pairs_list(case.n)[::-1][:300].copy()
    for sampling in setups:
        m, m4, m_half, m_plain = case.metric(sampling, vs), case.metric(sampling, vs4), case.metric(sampling, half), case.metric(sampling, [])
        for loss, floor, scale in VR.COMBOS:
            code, where = LOSS_CODES[loss], (case.label, sampling, loss, floor, scale)
            delta = VR.case_delta(case.label, scale)
            half_delta = np.float32(0.5) * delta
            assert np.float32(2.0) * half_delta == delta
            delta, half_delta = float(delta), float(half_delta)
            # the evaluation's own bits
            want = m.evaluate_variance_robust(code, delta, floor, want_pairs=True)
            got = m.evaluate_variance_robust_map(code, delta, floor, want_pairs=True)
            q_got = m.robust_map_fixed()
            assert _same_scalars(got, want) and np.array_equal(_u32(got[5]), _u32(want[3])), where
            assert got[3].shape == (case.n, case.n_t, case.n_alpha) and got[3].dtype == np.float32 and np.all(got[4] <= got[3]), where
            assert got[4].max() > 0.0 and want[2] < 1.0, where                 # the loss rejects
            lwant = m.evaluate_variance_robust_pairs(idx, code, delta, floor, want_pairs=True)
            lgot = m.evaluate_variance_robust_map_pairs(idx, code, delta, floor, want_pairs=True)
            q_lgot = m.robust_map_fixed()
            assert _same_scalars(lgot, lwant) and np.array_equal(_u32(lgot[5]), _u32(lwant[3])), where
            # delta = inf: REJ is zero and HITS is the n-metric's, whatever V is
            plain = m_plain.evaluate_robust_map(code, delta)
            q_plain = m_plain.robust_map_fixed()
            inf = m.evaluate_variance_robust_map(code, INF, floor)
            q_inf = m.robust_map_fixed()
            assert not inf[4].any() and not q_inf[1].any() and inf[2] == 1.0, where
            assert np.array_equal(q_inf[0], q_plain[0]) and np.array_equal(_u32(inf[3]), _u32(plain[2])), where
            assert np.array_equal(q_got[0], q_plain[0]), where                  # HITS: no variance, no loss and no delta in it
            # V and the floor x 4, delta x 1/2: both planes keep their bits
            got4 = m4.evaluate_variance_robust_map(code, half_delta, 4.0 * floor)
            assert _same_fixed(m4.robust_map_fixed(), q_got) and _same_planes(got4, got), where
            assert _u64(got4[0])[()] == _u64(got[0])[()] and _u64(got4[2])[()] == _u64(got[2])[()], where
            lgot4 = m4.evaluate_variance_robust_map_pairs(idx, code, half_delta, 4.0 * floor)
            assert _same_fixed(m4.robust_map_fixed(), q_lgot) and _same_planes(lgot4, lgot), where
        # V == 0.5, floor <= 1: the n-metric's map in fixed point, at robust_terms' scales of the raw residual
        for loss in VR.LOSSES:
            code = LOSS_CODES[loss]
            for scale, floor in zip(R.SCALES, (0.25, 1.0)):
                where = (case.label, sampling, loss, scale, floor)
                delta = float(R.case_delta(case.label, scale))
                plain = m_plain.evaluate_robust_map(code, delta, want_pairs=True)
                q_plain = m_plain.robust_map_fixed()
                one = m_half.evaluate_variance_robust_map(code, delta, floor, want_pairs=True)
                assert _same_fixed(m_half.robust_map_fixed(), q_plain), where
                assert np.array_equal(_u32(one[3]), _u32(plain[2])) and np.array_equal(_u32(one[4]), _u32(plain[3])) and plain[3].max() > 0.0, where
                assert np.array_equal(_u32(one[5][:, (0, 2, 3)]), _u32(plain[4])) and one[1] == 1.0, where
                lplain = m_plain.evaluate_robust_map_pairs(idx, code, delta)
                q_lplain = m_plain.robust_map_fixed()
                lone = m_half.evaluate_variance_robust_map_pairs(idx, code, delta, floor)
                assert _same_fixed(m_half.robust_map_fixed(), q_lplain) and _u64(lone[0])[()] == _u64(lplain[0])[()], where
        for x in (m, m4, m_half, m_plain):
            x.close()


# ---- 2: the statement, the sums ------------------------------------------------------------------------------------------------------
# The bars of the sums.  sum HITS of a view is its sample count but for the float32 rounding of the four footprint products (each
# within 2^-24 of its value, their sum within 2^-22 of 1) and the truncation to 2^-32 of each deposit: 1e-6 relative.  At V == 0.5
# sum REJ is sum (u - k) 2 n_kappa but for the float32 rounding of the columns u and k, 2^-25 relative to k <= 1, over a rejected share
# of at least a hundredth: 1e-5 relative.
BAR_HITS, BAR_REJ = 1e-6, 1e-5


def _sums(hits, counts, where):
    h = hits.astype(np.float64).sum(axis=(1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = float(np.max(np.where(counts > 0, np.abs(h - counts) / np.where(counts > 0, counts, 1.0), np.where(h > 0, np.inf, 0.0)))) / BAR_HITS
    print("%s: sum HITS per view against the sample count, %.3g of the bar %.0e" % (where, e, BAR_HITS))
    return e


def _refused(rej, rows, ij, n_kappa, where):
    n = len(rej)
    refused = np.zeros(n)
    for (i, j), u, kept, k in zip(ij, rows[:, 1].astype(np.float64), rows[:, 2].astype(np.float64), n_kappa):
        refused[[i, j]] += (u - kept) * 2 * k
    r = rej.astype(np.float64).sum(axis=(1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = float(np.max(np.where(refused > 0, np.abs(r - refused) / np.where(refused > 0, refused, 1.0), np.where(r > 0, np.inf, 0.0)))) / BAR_REJ
    print("%s: V == 0.5, sum REJ per view against sum (u - k) 2 n_kappa, %.3g of the bar %.0e" % (where, e, BAR_REJ))
    return e


STATEMENT = {"d": list(VR.COMBOS), "e": [("truncated", 1.5, "p90"), ("huber", 0.125, "median")],
             "i": [("truncated", 1.5, "p90"), ("huber", 0.125, "median"), ("geman_mcclure", 1.5, "p90")],
             "j": [("truncated", 1.5, "p90"), ("geman_mcclure", 0.125, "median")],
             "c": [("truncated", 1.5, "p90")], "f": [("truncated", 1.5, "p90")]}


@pytest.mark.parametrize("case", sorted(STATEMENT), indirect=True)
def test_planes_against_the_statement(case):
    """Non-square bins (d, i, j: 96 x 64), plain data (i), kappa_max = pi/2 (f) and the row-quad copies (c) at one setting each.
    Case e's statement covers the oracle's sample of the pairs: the list form over those.  The worst ratios of a GPU run are in
    DESIGN.md 4.31."""
    failures = []
    vs, half = case.variance_dtrs(case.variances), case.constant(0.5)
    n_kappa_all = np.array([len(T.kappa_grid(k)) for k in np.asarray(case.K01s, np.float32)])
    smp = VR.case_samples(case.label)
    listed = len(smp["pairs"]) != case.N
    idx = np.ascontiguousarray(np.concatenate([smp["ij"], smp["ij"]], axis=1), np.int32)
    n_kappa = n_kappa_all[smp["pairs"]]
    counts = np.zeros(case.n)
    for (i, j), k in zip(smp["ij"], n_kappa):
        counts[[i, j]] += 2 * k
    for sampling, _ in case.setups:
        m, m_half = case.metric(sampling, vs), case.metric(sampling, half)
        tol = T.tolerance(sampling, len(idx) if listed else case.N)
        for loss, floor, scale in STATEMENT[case.label]:
            delta = float(VR.case_delta(case.label, scale))
            want_h, want_r = VM.case_map(case.label, loss, floor, scale)
            s = VM.case_scale(case.label, loss, floor, scale)
            if listed:
                _, _, _, hits, rej = m.evaluate_variance_robust_map_pairs(idx, LOSS_CODES[loss], delta, floor)
            else:
                _, _, _, hits, rej = m.evaluate_variance_robust_map(LOSS_CODES[loss], delta, floor)
            assert np.all(np.isfinite(hits)) and np.all(np.isfinite(rej)) and np.all(hits >= 0) and np.all(rej >= 0)
            a, b = M.compare(hits, want_h, s, tol), M.compare(rej, want_r, s, tol)
            where = "case %s %-10s %-13s floor %-5g %-6s" % (case.label, sampling, loss, floor, scale)
            line = "%s (delta %.6g): HITS %.3g, REJ %.3g of the bar %.0e" % (where, delta, a, b, tol)
            if tol == T.TOL_THROUGHPUT and case.label not in ("c", "f"):
                h64, r64 = VM.case_map(case.label, loss, floor, scale, "float64")
                line += "; against float64 positions HITS %.3g, REJ %.3g" % (M.compare(hits, h64, s, tol), M.compare(rej, r64, s, tol))
            print(line)
            eh = _sums(hits, counts, where)
            if not max(a, b, eh) <= 1.0:
                failures.append(line + "; sum HITS %.3g" % eh)
        # V == 0.5: sum REJ from the rows
        loss = STATEMENT[case.label][0][0]
        delta = float(R.case_delta(case.label, "p90"))
        if listed:
            _, _, _, hits, rej, rows = m_half.evaluate_variance_robust_map_pairs(idx, LOSS_CODES[loss], delta, 1.0, want_pairs=True)
        else:
            _, _, _, hits, rej, rows = m_half.evaluate_variance_robust_map(LOSS_CODES[loss], delta, 1.0, want_pairs=True)
        where = "case %s %-10s %-13s" % (case.label, sampling, loss)
        eh, er = _sums(hits, counts, where), _refused(rej, rows, smp["ij"], n_kappa, where)
        if not max(eh, er) <= 1.0:
            failures.append("%s: V == 0.5: sum HITS %.3g, sum REJ %.3g of their bars" % (where, eh, er))
        m.close()
        m_half.close()
    assert not failures, "\n".join(failures)


# ---- 3: reproducible, subsets ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", ["polynomial", "per_sample", "reference"])
def test_reproducible_and_subsets(gpu_ctx, oracle_mod, sampling):
    """Two calls: identical plane bytes.  The list reversed: identical.  The list cut in two calls: the fixed-point sums add up to
    those of the whole list exactly, and every float plane is float32(q 2^-32) of its sums; a pair listed twice deposits twice, a pair
    without samples (P0 == P1) nothing.  views = one view, the last view, an unordered list, every view reversed: the all-views planes
    bit for bit, the rows unchanged."""
    import epipolarconsistency_amd as E
    c = _Case(gpu_ctx, "d")
    try:
        m = c.metric(sampling, c.variance_dtrs(c.variances))
        delta, floor = float(VR.case_delta("d", "p90")), 1.5
        first = m.evaluate_variance_robust_map(E.LOSS_HUBER, delta, floor, want_pairs=True)
        again = m.evaluate_variance_robust_map(E.LOSS_HUBER, delta, floor, want_pairs=True)
        assert all(np.array_equal(_u32(first[k]), _u32(again[k])) for k in (3, 4, 5)) and _same_scalars(first, again)
        idx = _all_pairs_list(c.n)
        # a fixed mode for the three lists: "reference" for every length, or a throughput path (which does not depend on the length)
        fwd = m.evaluate_variance_robust_map_pairs(idx, E.LOSS_HUBER, delta, floor, want_pairs=True)
        q_fwd = m.robust_map_fixed()
        for k in (0, 1):
            assert np.array_equal(_u32(fwd[3 + k]), _u32((q_fwd[k].astype(np.float64) * 2.0 ** -32).astype(np.float32)))
        assert _same_planes(fwd, first), sampling
        rev = m.evaluate_variance_robust_map_pairs(idx[::-1].copy(), E.LOSS_HUBER, delta, floor, want_pairs=True)
        assert _same_planes(rev, fwd) and np.array_equal(_u32(rev[5]), _u32(fwd[5][::-1]))
        cut = 11
        m.evaluate_variance_robust_map_pairs(idx[:cut], E.LOSS_HUBER, delta, floor)
        q_a = m.robust_map_fixed()
        m.evaluate_variance_robust_map_pairs(idx[cut:], E.LOSS_HUBER, delta, floor)
        q_b = m.robust_map_fixed()
        for k in (0, 1):
            assert np.array_equal(q_a[k] + q_b[k], q_fwd[k]), (sampling, k)
        twice = m.evaluate_variance_robust_map_pairs(np.concatenate([idx, idx[:cut]]), E.LOSS_HUBER, delta, floor)
        q_twice = m.robust_map_fixed()
        assert all(np.array_equal(q_twice[k], q_fwd[k] + q_a[k]) for k in (0, 1)) and twice[3].sum() > fwd[3].sum()
        dead = m.evaluate_variance_robust_map_pairs(np.concatenate([idx, [[2, 2, 2, 3]]]).astype(np.int32), E.LOSS_HUBER, delta, floor, want_pairs=True)
        assert np.array_equal(dead[5][-1], [0.0, 1.0, 1.0, 0.0])        # a pair without samples: its row, and no deposit
        assert _same_fixed(m.robust_map_fixed(), q_fwd)
        for views in ([2], [c.n - 1], [5, 0, c.n - 1, 3], list(range(c.n))[::-1]):
            part = m.evaluate_variance_robust_map(E.LOSS_HUBER, delta, floor, views=views, want_pairs=True)
            assert part[3].shape[0] == len(views) and _same_scalars(part, first) and np.array_equal(_u32(part[5]), _u32(first[5]))
            for k, v in enumerate(views):
                assert np.array_equal(_u32(part[3][k]), _u32(first[3][v])) and np.array_equal(_u32(part[4][k]), _u32(first[4][v])), (views, v)
            lpart = m.evaluate_variance_robust_map_pairs(idx, E.LOSS_HUBER, delta, floor, views=views)
            assert _same_planes(lpart, part)
        m.close()
    finally:
        c.close()


# ---- 4: the map as the next pass's variance fields -----------------------------------------------------------------------------------------
def test_map_variances(gpu_ctx, oracle_mod):
    """A field with zeros, values between 0 and floor / 2 and bins below min_hits, against numpy bit for bit; max_factor 1 and a
    delta = inf map return V's bits; the three kinds of map refuse each other's calls."""
    import epipolarconsistency_amd as E
    c = _Case(gpu_ctx, "d")
    try:
        floor = 1.5
        rng = np.random.default_rng(11)
        fields = [np.array(f, np.float32) for f in c.variances]
        for f in fields:                                                  # blocks of zeros and of values below floor / 2 in every view
            f[:16, :24] = 0.0
            f[16:32, 24:48] = rng.uniform(0.0, 0.5 * floor, (16, 24)).astype(np.float32)
        fields[2][:] = 0.0                                                # a clean view: zeros everywhere
        vs = c.variance_dtrs(fields)
        m = c.metric("polynomial", vs)
        delta = float(VR.case_delta("d", "p90"))
        _, _, _, hits, rej = m.evaluate_variance_robust_map(E.LOSS_TRUNCATED, delta, floor)
        mu = M.map_weights(hits, rej, 1.0, 1.0)
        assert (hits < 1.0).any() and (hits >= 4.0).any() and ((mu > 0.0) & (mu < 1.0)).any()
        assert (mu * np.float32(1.5) <= 1.0).any() and (mu * np.float32(1.5) > 1.0).any()      # the cap at max_factor 1.5 is reached, and not everywhere
        assert any(((f == 0.0) & (mu[v] < 1.0)).any() for v, f in enumerate(fields))           # a zero where the loss rejected
        assert any(((f > 0.0) & (f < 0.5 * floor) & (mu[v] < 1.0)).any() for v, f in enumerate(fields))
        for min_hits, gain, max_factor in ((0.0, 1.0, 1e4), (1.0, 1.0, 1e4), (4.0, 2.5, 8.0), (1.0, 0.5, 1.5)):
            new = m.variance_robust_map_variances(floor, min_hits, gain, max_factor)
            assert len(new) == c.n and new[0].getFilter() == E.FILTER_NONE
            for v, w in enumerate(new):
                got, want = w.readback(), VM.map_variances(fields[v], hits[v], rej[v], floor, min_hits, gain, max_factor)
                assert np.array_equal(_u32(got), _u32(want)), (min_hits, gain, max_factor, v, int((_u32(got) != _u32(want)).sum()))
                for slip in VM.RULE_SLIPS:
                    assert not np.array_equal(_u32(got), _u32(VM.map_variances(fields[v], hits[v], rej[v], floor, min_hits, gain, max_factor, slip))), (v, slip)
            assert any((w.readback() > f).any() for w, f in zip(new, fields))
            _close(new)
        same = m.variance_robust_map_variances(floor, 1.0, 1.0, 1.0)     # max_factor 1: V
        assert all(np.array_equal(_u32(w.readback()), _u32(f)) for w, f in zip(same, fields))
        _close(same)
        part = m.evaluate_variance_robust_map(E.LOSS_TRUNCATED, delta, floor, views=[4, 1])
        new = m.variance_robust_map_variances(floor)
        assert len(new) == 2 and np.array_equal(_u32(part[3][0]), _u32(hits[4]))
        for k, v in enumerate((4, 1)):                                    # the field follows the mapped view, not the slot
            assert np.array_equal(_u32(new[k].readback()), _u32(VM.map_variances(fields[v], part[3][k], part[4][k], floor)))
        _close(new)
        m.evaluate_variance_robust_map(E.LOSS_TRUNCATED, INF, floor)
        same = m.variance_robust_map_variances(floor, 1.0, 3.0)          # nothing rejected: V
        assert all(np.array_equal(_u32(w.readback()), _u32(f)) for w, f in zip(same, fields))
        _close(same)
        m.evaluate_variance_robust_map(E.LOSS_TRUNCATED, delta, floor)
        second = m.variance_robust_map_variances(floor)
        m2 = c.metric("polynomial", second)                               # the second half of a new 2 n metric
        value, mean_weight = m2.evaluate_variance(floor)
        before = m.evaluate_variance(floor)
        assert 0.0 < mean_weight < before[1] and value > 0.0             # less weight than under the old variances
        m2.close()
        _close(second)
        # this kind's map is refused by the two *_map_weights calls ...
        for call in (m.robust_map_weights, m.weighted_robust_map_weights):
            with pytest.raises(E.EccError) as e:
                call()
            assert e.value.code == 1
        _close(m.variance_robust_map_variances(floor))                   # ... and is still held
        # ... and the other two kinds' maps by this call
        m.evaluate_robust_map(E.LOSS_TRUNCATED, delta)                    # the n-metric's map, held by the same metric
        with pytest.raises(E.EccError) as e:
            m.variance_robust_map_variances(floor)
        assert e.value.code == 1 and "no variance robust map held" in str(e.value)
        m.close()
        mw = c.metric("polynomial", c.constant(0.5))                      # 0.5 read as a line weight
        mw.evaluate_weighted_robust_map(E.LOSS_TRUNCATED, delta)
        with pytest.raises(E.EccError) as e:
            mw.variance_robust_map_variances(floor)
        assert e.value.code == 1
        _close(mw.weighted_robust_map_weights())
        mw.evaluate_variance_robust_map(E.LOSS_TRUNCATED, delta, 1.0)
        _close(mw.variance_robust_map_variances(1.0))
        mw.refreshRadonIntermediates(0, 1)                                # drops the held map
        with pytest.raises(E.EccError):
            mw.variance_robust_map_variances(1.0)
        mw.close()
    finally:
        c.close()


# ---- 5: the reason the calls exist ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _demo_statement():
    """The statement's figures of DESIGN.md 4.31 from the oracle's intermediates, computed once for the three sampling modes:
    key -> (delta, per-view shares of pass 1, ratios after passes 0, 1, 2)."""
    import oracle
    from conftest import make_small_scan
    Ps, imgs = make_small_scan()
    noisy, both, var = VR.demo_images(imgs)
    B = V.DEMO_BINS
    clean_d = [oracle.radon(im, B, B) for im in imgs]
    noisy_d = [d if k != V.DEMO_VIEW else oracle.radon(noisy[k], B, B) for k, d in enumerate(clean_d)]
    both_d = [d if k != VR.DEMO_BLOCK_VIEW else oracle.radon(both[k], B, B) for k, d in enumerate(noisy_d)]
    fields0 = [np.asarray(oracle.radon(v, B, B, filter=2), np.float32) for v in var]
    floor = V.demo_floor(fields0)
    K = {key: oracle.evaluate_all(Ps, d, 128, 128, want_K01=True)["K01s"] for key, d in (("clean", clean_d), ("noisy", noisy_d), ("both", both_d))}
    out = {}
    for key, bad in (("both", both_d), ("noisy", noisy_d)):
        fields, delta, shares = fields0, None, []
        ratios = [VM.demo_ratio(Ps, clean_d, bad, fields, floor, 128, 128, K["clean"], K[key])]
        for _ in range(2):
            delta, hits, rej, fields = VM.demo_pass(Ps, bad, fields, floor, 128, 128, K[key], delta)
            shares.append(VM.rejected_share(hits, rej))
            ratios.append(VM.demo_ratio(Ps, clean_d, bad, fields, floor, 128, 128, K["clean"], K[key]))
        out[key] = (delta, shares[0], ratios)
    return out


@pytest.mark.parametrize("sampling", ["polynomial", "per_sample", "auto"])
def test_the_feedback_makes_the_variance_form_robust(gpu_ctx, oracle_mod, sampling):
    """DESIGN.md 4.30's fixture on the device: 8 views of the spheres at 128^2 -> 96^2 bins, noise of 5 % on the left half of view 3
    with V known, the opaque block pasted unflagged into view 5; truncated loss, delta = variance_robust_scale(rows at delta = inf,
    2.0) of the corrupted scan, held; floor = variance_floor of V_3; min_hits 1, gain 1, max_factor 1e4.
        the map:       view 5 has the largest and view 3 the smallest sum REJ / sum HITS;
        the feedback:  corrupted / clean of evaluate_variance under the returned variances, the same fields applied to both scans:
                       pass 1 <= 1/4 of pass 0, pass 2 <= 1/4 of pass 1;
        noise only:    <= 1.05 after two passes.
    The device's shares and ratios are printed beside the statement's (DESIGN.md 4.31 has a run's).  refine_variances(passes=2)
    returns pass 2's fields bit for bit."""
    import epipolarconsistency_amd as E
    from conftest import make_small_scan
    Ps, imgs = make_small_scan()
    noisy, both, var = VR.demo_images(imgs)
    B = V.DEMO_BINS
    dev = {key: E.RadonIntermediate.compute_batch(gpu_ctx, np.asarray(x, np.float32), B, B) for key, x in (("clean", imgs), ("noisy", noisy), ("both", both))}
    var_d = E.variance_intermediates(gpu_ctx, var, B, B)
    TR = E.LOSS_TRUNCATED
    made = []

    def metric(dtrs):
        return E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling(sampling)

    def ratio(key, fields):
        bad, clean = metric(dev[key] + fields), metric(dev["clean"] + fields)
        out = bad.evaluate_variance(floor)[0] / clean.evaluate_variance(floor)[0]
        bad.close()
        clean.close()
        return out
    try:
        floor = E.variance_floor(var_d[V.DEMO_VIEW].readback(), V.DEMO_FLOOR_FRACTION)
        statement = _demo_statement()
        got = {}
        for key in ("both", "noisy"):
            fields, delta, shares, ratios, passes = var_d, None, [], [ratio(key, var_d)], []
            for _ in range(2):
                m = metric(dev[key] + fields)
                if delta is None:
                    delta = E.variance_robust_scale(m.evaluate_variance_robust(TR, INF, floor, want_pairs=True)[3], VR.DEMO_K)
                _, mean_weight, mass, hits, rej = m.evaluate_variance_robust_map(TR, delta, floor)
                fields = m.variance_robust_map_variances(floor, VM.DEMO_MIN_HITS, VM.DEMO_GAIN, VM.DEMO_MAX_FACTOR)
                m.close()
                made += fields
                shares.append(VM.rejected_share(hits, rej))
                ratios.append(ratio(key, fields))
                passes.append((fields, mean_weight, mass))
            got[key] = (delta, shares, ratios, passes)
            s_delta, s_share, s_ratios = statement[key]
            print("%-5s %-10s delta %.6g (statement %.6g); sum REJ / sum HITS per view, pass 1: %s (statement %s; worst relative difference "
                  "%.3g); corrupted / clean of evaluate_variance: %s (statement %s; relative differences %s)" % (
                      key, sampling, delta, s_delta, " ".join("%.4f" % v for v in shares[0]), " ".join("%.4f" % v for v in s_share),
                      float(np.max(np.abs(shares[0] - s_share) / np.where(s_share > 0, s_share, 1.0))),
                      " -> ".join("%.5g" % v for v in ratios), " -> ".join("%.5g" % v for v in s_ratios),
                      " ".join("%.2g" % (abs(a - b) / b) for a, b in zip(ratios, s_ratios))))
        delta, shares, ratios, passes = got["both"]
        refined, records = E.refine_variances(gpu_ctx, Ps, dev["both"], var_d, floor, passes=2, sampling=sampling)
        made += refined
        same = [np.array_equal(_u32(a.readback()), _u32(b.readback())) for a, b in zip(refined, passes[1][0])]
        assert len(same) == len(Ps) and all(same), same
        assert len(records) == 2 and records[0]["delta"] == records[1]["delta"] == delta
        for rec, (_, mean_weight, mass), share in zip(records, passes, shares):
            assert _u64(rec["mean_weight"])[()] == _u64(mean_weight)[()] and _u64(rec["inlier_mass"])[()] == _u64(mass)[()]
            assert np.allclose(rec["rejected_share"], share, rtol=1e-12)
        assert all(np.all(b.readback() >= a.readback()) for a, b in zip(passes[0][0], passes[1][0]))
        assert int(np.argmax(shares[0])) == VR.DEMO_BLOCK_VIEW and int(np.argmin(shares[0])) == V.DEMO_VIEW, shares[0]
        assert ratios[0] >= 100.0 and ratios[1] <= 0.25 * ratios[0] and ratios[2] <= 0.25 * ratios[1], ratios
        assert got["noisy"][2][2] <= 1.05, got["noisy"][2]
    finally:
        _close([d for ds in dev.values() for d in ds] + var_d + made)


# ---- 6: errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors(gpu_ctx, oracle_mod):
    """In the stated order: evaluate_variance_robust[_pairs]' own first, in their order, then the views list;
    variance_robust_map_variances' own.  A refused argument does not reach the device: nothing is written and no map is held."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib
    L = _lib.lib()
    c = _Case(gpu_ctx, "d")
    try:
        vs = c.variance_dtrs(c.variances)
        m = c.metric("auto", vs)
        delta, floor = float(VR.case_delta("d", "p90")), 1.5
        handles = (C.c_void_p * c.n)()
        assert L.ecc_metric_variance_robust_map_variances(m._h, floor, 1.0, 1.0, 1e4, handles) == 1 and b"no variance robust map held" in L.ecc_last_error()
        with pytest.raises(E.EccError):
            m.variance_robust_map_variances(floor)
        bins = c.n_t * c.n_alpha
        value, weight, mass = C.c_double(-1.0), C.c_double(-1.0), C.c_double(-1.0)
        terms, hits, rej = np.full((c.N, 4), -1.0, np.float32), np.full(c.n * bins, -1.0, np.float32), np.full(c.n * bins, -1.0, np.float32)
        out = (C.c_void_p(hits.ctypes.data), C.c_void_p(rej.ctypes.data), C.byref(value), C.byref(weight), C.byref(mass), C.c_void_p(terms.ctypes.data))
        idx = _all_pairs_list(c.n)
        pidx = C.c_void_p(idx.ctypes.data)

        def both(h, loss, d, fl, views, k, outs=out, lst=pidx, count=len(idx)):
            v = None if views is None else C.c_void_p(np.ascontiguousarray(views, np.int32).ctypes.data)
            return (L.ecc_metric_evaluate_variance_robust_map(h, loss, d, fl, v, k, *outs),
                    L.ecc_metric_evaluate_variance_robust_map_pairs(h, lst, count, loss, d, fl, v, k, *outs))
        for views, k in (([0, 1, 1], 3), ([3, 3], 2), ([0, c.n], 2), ([-1], 1), ([0], -1), (None, 2)):   # (c.n: a variance intermediate is no view)
            assert both(m._h, 0, delta, floor, views, k) == (1, 1), (views, k)
        L.ecc_metric_evaluate_variance_robust_map(m._h, 0, delta, floor, C.c_void_p(np.array([3, 3], np.int32).ctypes.data), 2, *out)
        assert b"listed twice" in L.ecc_last_error()
        assert both(m._h, 7, delta, floor, [3, 3], 2) == (1, 1) and b"loss" in L.ecc_last_error()          # the loss comes before the list
        assert both(m._h, 0, -1.0, floor, [0, c.n], 2) == (1, 1) and b"delta" in L.ecc_last_error()
        for bad_floor in (0.0, -1.0, float("nan"), INF):
            assert both(m._h, 0, delta, bad_floor, [3, 3], 2) == (1, 1) and b"floor" in L.ecc_last_error()   # the floor before the list
        assert both(m._h, 0, -1.0, 0.0, [3, 3], 2) == (1, 1) and b"delta" in L.ecc_last_error()           # delta before the floor
        no_value = (out[0], out[1], None, out[3], out[4], out[5])
        assert both(m._h, 0, delta, floor, None, 0, outs=no_value) == (1, 1) and b"value is null" in L.ecc_last_error()
        assert both(m._h, 7, -1.0, 0.0, [3, 3], 2, outs=no_value) == (1, 1) and b"value is null" in L.ecc_last_error()   # value < loss < delta
        assert L.ecc_metric_evaluate_variance_robust_map_pairs(m._h, pidx, -1, 7, delta, floor, None, 0, *no_value) == 1
        assert L.ecc_last_error() == b"negative list length"                                       # the list's own checks first
        assert L.ecc_metric_evaluate_variance_robust_map_pairs(m._h, None, 2, 7, delta, floor, None, 0, *no_value) == 1
        assert L.ecc_last_error() == b"index list is null"
        bad = np.concatenate([idx[:3], [[0, 1, c.n, 1]]]).astype(np.int32)                          # a data index that is a variance's
        assert L.ecc_metric_evaluate_variance_robust_map_pairs(m._h, C.c_void_p(bad.ctypes.data), 4, 0, delta, floor,
                                                               C.c_void_p(np.array([3, 3], np.int32).ctypes.data), 2, *out) == 1
        assert b"invalid indices" in L.ecc_last_error()                                             # a bad tuple before the views list
        m.useCorrelation(True)
        assert both(m._h, 0, delta, floor, [3, 3], 2) == (5, 5)                                     # ECC_ERR_UNSUPPORTED, before the list
        assert both(m._h, 0, delta, 0.0, [3, 3], 2) == (1, 1) and b"floor" in L.ecc_last_error()    # the floor before use_corr
        assert L.ecc_metric_evaluate_variance_robust_map_pairs(m._h, C.c_void_p(bad.ctypes.data), 4, 0, delta, floor, None, 0, *out) == 5   # use_corr before a bad tuple
        m.useCorrelation(False)
        plain = c.metric("auto", [])                                                                # n intermediates: no variances
        assert both(plain._h, 0, delta, 0.0, [3, 3], 2) == (1, 1) and b"2 * n_views" in L.ecc_last_error()   # the shape before the floor
        plain.close()
        assert value.value == -1.0 and weight.value == -1.0 and mass.value == -1.0
        assert np.all(terms == -1.0) and np.all(hits == -1.0) and np.all(rej == -1.0)
        assert L.ecc_metric_variance_robust_map_variances(m._h, floor, 1.0, 1.0, 1e4, handles) == 1   # still no map: every call above failed
        got = m.evaluate_variance_robust_map(E.LOSS_HUBER, delta, floor, want_pairs=True)
        want = m.evaluate_variance_robust(E.LOSS_HUBER, delta, floor, want_pairs=True)
        assert _same_scalars(got, want) and np.array_equal(_u32(got[5]), _u32(want[3]))
        for args, word in (((0.0, 1.0, 1.0, 1e4), b"floor"), ((-1.0, 1.0, 1.0, 1e4), b"floor"), ((float("nan"), 1.0, 1.0, 1e4), b"floor"),
                           ((INF, 1.0, 1.0, 1e4), b"floor"), ((floor, -1.0, 1.0, 1e4), b"min_hits"), ((floor, float("nan"), 1.0, 1e4), b"min_hits"),
                           ((floor, 1.0, -0.5, 1e4), b"gain"), ((floor, 1.0, INF, 1e4), b"gain"), ((floor, 1.0, 1.0, 0.5), b"max_factor"),
                           ((floor, 1.0, 1.0, INF), b"max_factor"), ((floor, 1.0, 1.0, float("nan")), b"max_factor"),
                           ((0.0, -1.0, -1.0, 0.5), b"floor"), ((floor, -1.0, -1.0, 0.5), b"min_hits"), ((floor, 1.0, -1.0, 0.5), b"gain")):
            assert L.ecc_metric_variance_robust_map_variances(m._h, *args, handles) == 1 and word in L.ecc_last_error(), args
        assert L.ecc_metric_variance_robust_map_variances(m._h, floor, 1.0, 1.0, 1e4, None) == 1
        assert all(h is None for h in handles)
        _close(m.variance_robust_map_variances(floor))                                              # the map is still held
        empty = m.evaluate_variance_robust_map_pairs(np.zeros((0, 4), np.int32), E.LOSS_HUBER, delta, floor)   # an empty list: zeros, no map held
        assert not empty[3].any() and not empty[4].any()
        with pytest.raises(E.EccError):
            m.variance_robust_map_variances(floor)
        m.close()
    finally:
        c.close()
