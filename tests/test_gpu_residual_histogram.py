"""ecc_metric_evaluate_residual_histogram[_pairs] and ecc_metric_evaluate_variance_residual_histogram[_pairs] on the GPU
(csrc/ecc_residual_histogram.hip, csrc/residual_histogram_kernel.hip): the per-view counts of the per-sample residual.  The cases
are the small loop-class cases of weighted_terms.CASES (residual_histogram_terms.LABELS: a polynomial, b per-sample, c row-quad
copies, d reference with four waves per pair, e reference with one, i plain data, j a user kappa step) with the data of channel 0
and, for the variance form, the variance fields of tests/variance_terms.py at floor 1.5.  Per case two widths per table size (the
overflow bin holds a tenth, and half a percent, of the samples in the statement) and 64 and 256 bins.

  exact        counts are integers, so these are equalities: the same call twice; row sums whatever the width and the table size, an
               even total; width 2 w against width w bin by bin; the list of all pairs against the all-pairs call and two disjoint
               lists against their union under an explicitly set sampling mode; V == 0.5 against the raw form; V, floor x 4 and
               width x 1/2; a one-pair list against evaluate_robust_pairs' r column;
  statement    the bracket of residual_histogram_terms on cumulative counts, per view row and per bin edge, at that module's tau
               (tests/test_residual_histogram_terms_oracle.py shows that this comparison rejects the slips it is there for); the
               smallest tau that would have passed is printed per table (DESIGN.md 4.34 records a run);
  edge cases, errors."""
import ctypes as C

import numpy as np
import pytest

import channel_terms as T
import residual_histogram_terms as H
from test_gpu_variance import _Case

pytestmark = pytest.mark.gpu

INF = float("inf")
EXPLICIT = {"auto": "reference"}   # case d selects its kernel through "auto" (28 pairs); the list checks set the mode it resolves to


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


def _raw_metric(case, sampling):
    return case.metric(sampling, [])


def _widths(label, kind, n_bins):
    return [float(H.case_width(label, kind, n_bins, share)) for share in H.OVERFLOW]


def _check_shape(counts, n, n_bins):
    assert counts.shape == (n, n_bins) and counts.dtype == np.uint64


@pytest.mark.parametrize("case", H.LABELS, indirect=True)
def test_counts_are_exact(case):
    """The integer identities of the raw form, in every sampling setup of the case: (1) the same call twice gives the same bits;
    (2) a view's row sum is the same at every width and table size, every row sum is even (+-kappa samples come in twos) and the
    sum of all cells, twice the samples, a multiple of 4; (3) width 2 w against width w at the same n_bins = B:
    coarse[k] == fine[2 k] + fine[2 k + 1] for k < B / 2 - 1 and the coarse bins from B / 2 - 1 up sum to fine[B - 2] + fine[B - 1]
    (inv_width halves exactly); (4) under an explicitly set sampling mode the list of all pairs equals the all-pairs call and two
    disjoint lists add up to their union; (7) a one-pair list at a width that leaves the overflow bin empty:
    sum counts[k] (k w)^2 <= r N <= sum counts[k] ((k + 1) w)^2 with r from evaluate_robust_pairs at delta = inf and N the row
    sum, loosened by the float32 rounding of r."""
    idx = _all_pairs_list(case.n)
    for sampling, _ in case.setups:
        m = _raw_metric(case, sampling)
        sums = None
        for B in H.N_BINS:
            for w in _widths(case.label, "raw", B):
                fine = m.evaluate_residual_histogram(w, B)
                _check_shape(fine, case.n, B)
                assert np.array_equal(fine, m.evaluate_residual_histogram(w, B)), (sampling, B, w)                      # (1)
                if sums is None:
                    sums = fine.sum(axis=1)
                    assert np.all(sums > 0) and np.all(sums % 2 == 0)
                assert np.array_equal(fine.sum(axis=1), sums), (sampling, B, w)                                        # (2)
                coarse = m.evaluate_residual_histogram(2.0 * w, B)                                                     # (3)
                half = B // 2
                assert np.array_equal(coarse[:, :half - 1], fine[:, 0:B - 2:2] + fine[:, 1:B - 2:2]), (sampling, B, w)
                assert np.array_equal(coarse[:, half - 1:].sum(axis=1), fine[:, B - 2] + fine[:, B - 1]), (sampling, B, w)
                assert np.array_equal(coarse.sum(axis=1), sums)
        # the largest table, 16 KiB of counters per workgroup, at the 64-bin table's width: the same bins below the smaller table's
        # overflow bin, which holds the rest
        B, big = H.N_BINS[0], 1024
        w = _widths(case.label, "raw", B)[0]
        small, large = m.evaluate_residual_histogram(w, B), m.evaluate_residual_histogram(w, big)
        _check_shape(large, case.n, big)
        assert np.array_equal(large[:, :B - 1], small[:, :B - 1]) and np.array_equal(large[:, B - 1:].sum(axis=1), small[:, B - 1]), sampling
        m.close()
        # (4) an explicitly set mode: a list's own length must not choose another one
        mode = EXPLICIT.get(sampling, sampling)
        m = _raw_metric(case, mode)
        B = H.N_BINS[0]
        w = _widths(case.label, "raw", B)[0]
        whole = m.evaluate_residual_histogram(w, B)
        assert np.array_equal(whole.sum(axis=1), sums), (mode, "row sums do not depend on the mode")
        assert np.array_equal(m.evaluate_residual_histogram_pairs(idx, w, B), whole), mode
        cut = len(idx) // 3
        first, second = m.evaluate_residual_histogram_pairs(idx[:cut], w, B), m.evaluate_residual_histogram_pairs(idx[cut:][::-1], w, B)
        assert np.array_equal(first + second, whole), mode
        # (7) one pair, tied to a column that is held to the statement already
        wide = float(np.float32(1.05 * H.case_scale(case.label, "raw") / (B - 1)))
        for q in (0, len(idx) // 2, len(idx) - 1):
            one = m.evaluate_residual_histogram_pairs(idx[q:q + 1], wide, B)
            i, j = idx[q, 2], idx[q, 3]
            assert np.array_equal(one[i], one[j]) and one.sum() == 2 * one[i].sum() and one[i, -1] == 0, (mode, q)
            _, _, rows = m.evaluate_robust_pairs(idx[q:q + 1], 1, INF, want_pairs=True)
            r, N, k = float(rows[0, 2]), float(one[i].sum()), np.arange(B, dtype=np.float64)
            cnt = one[i].astype(np.float64)
            lower, upper = float(cnt @ (k * wide) ** 2), float(cnt @ ((k + 1.0) * wide) ** 2)
            eps = 2.0 ** -24   # r is one float32 rounding of raw / count
            assert lower <= r * N * (1.0 + eps) and r * N * (1.0 - eps) <= upper, (mode, q, lower, r * N, upper)
        assert int(whole.sum()) % 4 == 0   # twice an even number of samples (the count itself: test_counts_against_the_statement)
        m.close()


@pytest.mark.parametrize("case", H.LABELS, indirect=True)
def test_counts_against_the_statement(case):
    """Both forms against the float64 statement over the float32 positions, per sampling setup, table size and width: every row sum
    equals the statement's sample count of that view, and per view row and bin edge the cumulative count lies in the statement's
    bracket at tau = residual_histogram_terms.tau_of (1.1e-7 of the case's largest value under the reference arithmetic, 2e-4 on the
    throughput paths: twice what a run measured).  The statement alone has at most 2 % of a row's samples within tau of any edge (asserted here as well), so
    the bracket cannot hide a wrong bin.  Printed per table: the smallest tau that would have passed."""
    vs = case.variance_dtrs(case.variances)
    failures = []
    for sampling, _ in case.setups:
        reference = T.tolerance(sampling, case.N) == T.TOL_REFERENCE
        for kind in H.KINDS:
            m = _raw_metric(case, sampling) if kind == "raw" else case.metric(sampling, vs)
            tau = H.tau_of(case.label, kind, reference)
            for B in H.N_BINS:
                for w in _widths(case.label, kind, B):
                    got = m.evaluate_residual_histogram(w, B) if kind == "raw" else m.evaluate_variance_residual_histogram(H.FLOOR, w, B)
                    _check_shape(got, case.n, B)
                    share = H.band_share(case.label, kind, w, B, tau)
                    cells, rows = H.bracket(got, case.label, kind, w, tau)
                    need = H.needed_tau(got, case.label, kind, w)
                    line = "case %s %-10s %-8s B %3d width %.6g: needs tau %.3g = %.3g of the largest value %.3g; tau %.3g, band share %.4f, " \
                           "%d cells outside, %d row sums differ" % (case.label, sampling, kind, B, w, need, need / H.case_scale(case.label, kind),
                                                                      H.case_scale(case.label, kind), tau, share, cells, rows)
                    print(line)
                    if cells or rows or not share <= H.MAX_BAND_SHARE:
                        failures.append(line)
            m.close()
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case", H.LABELS, indirect=True)
def test_variance_form_identities(case):
    """(5) V == 0.5f and floor <= 1: s == sc == 1.0f, sqrtf(1.0f) == 1.0f and a / 1.0f == a -- the counts are the bits of the raw
    form on the n-metric over the same data, at floor 0.25 and 1.0.  (6) the case's fields and the floor x 4 with the width x 1/2
    (all exact in float32): sqrtf(4 sc) == 2 sqrtf(sc), z halves exactly and inv_width doubles exactly -- the counts keep their bits.
    Also the list form of all pairs against the all-pairs call, and repeatability."""
    half = case.constant(0.5)
    vs = case.variance_dtrs(case.variances)
    vs4 = case.variance_dtrs([np.float32(4.0) * f for f in case.variances])
    idx = _all_pairs_list(case.n)
    for sampling, _ in case.setups:
        B = H.N_BINS[1]
        m_raw, m_half = _raw_metric(case, sampling), case.metric(sampling, half)
        for w in _widths(case.label, "raw", B):
            want = m_raw.evaluate_residual_histogram(w, B)
            for floor in (0.25, 1.0):
                assert np.array_equal(m_half.evaluate_variance_residual_histogram(floor, w, B), want), (sampling, w, floor)   # (5)
        m_raw.close()
        m_half.close()
        m, m4 = case.metric(sampling, vs), case.metric(sampling, vs4)
        for B in H.N_BINS:
            for w in _widths(case.label, "variance", B):
                got = m.evaluate_variance_residual_histogram(H.FLOOR, w, B)
                assert np.array_equal(got, m.evaluate_variance_residual_histogram(H.FLOOR, w, B)), (sampling, B, w)
                assert np.array_equal(m4.evaluate_variance_residual_histogram(4.0 * H.FLOOR, 0.5 * w, B), got), (sampling, B, w)  # (6)
        mode = EXPLICIT.get(sampling, sampling)
        if mode == sampling:
            assert np.array_equal(m.evaluate_variance_residual_histogram_pairs(idx, H.FLOOR, w, B), got), sampling
        m.close()
        m4.close()


def test_edge_cases_and_errors(gpu_ctx, oracle_mod):
    """An empty list is ECC_OK with all zeros written; NaN data lands in the overflow bin and nowhere else; the argument errors of
    a live metric come before any write, in the header's order."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib
    c = _Case(gpu_ctx, "d")
    try:
        L = _lib.lib()
        m = _raw_metric(c, "reference")
        B = 64
        w = float(H.case_width("d", "raw", B, "tenth"))
        empty = m.evaluate_residual_histogram_pairs(np.zeros((0, 4), np.int32), w, B)
        assert empty.shape == (c.n, B) and not empty.any()
        buf = np.full((c.n, B), 7, np.uint64)
        ptr = C.c_void_p(buf.ctypes.data)
        idx = _all_pairs_list(c.n)
        bad = idx.copy()
        bad[3, 2] = c.n   # a data index that names no row
        calls = [(L.ecc_metric_evaluate_residual_histogram(m._h, 0.0, B, ptr), 1), (L.ecc_metric_evaluate_residual_histogram(m._h, INF, B, ptr), 1),
                 (L.ecc_metric_evaluate_residual_histogram(m._h, float("nan"), B, ptr), 1), (L.ecc_metric_evaluate_residual_histogram(m._h, 1e-40, B, ptr), 1),
                 (L.ecc_metric_evaluate_residual_histogram(m._h, w, 32, ptr), 1), (L.ecc_metric_evaluate_residual_histogram(m._h, w, 96, ptr), 1),
                 (L.ecc_metric_evaluate_residual_histogram(m._h, w, 1088, ptr), 1), (L.ecc_metric_evaluate_residual_histogram(m._h, w, B, None), 1),
                 (L.ecc_metric_evaluate_residual_histogram_pairs(m._h, C.c_void_p(idx.ctypes.data), -1, w, B, ptr), 1),
                 (L.ecc_metric_evaluate_residual_histogram_pairs(m._h, None, 2, w, B, ptr), 1),
                 (L.ecc_metric_evaluate_residual_histogram_pairs(m._h, C.c_void_p(bad.ctypes.data), len(bad), w, B, ptr), 1),
                 (L.ecc_metric_evaluate_variance_residual_histogram(m._h, 1.5, w, B, ptr), 1),      # n_dtrs != 2 n_views
                 (L.ecc_metric_evaluate_variance_residual_histogram_pairs(m._h, C.c_void_p(idx.ctypes.data), len(idx), 1.5, w, B, ptr), 1)]
        assert [code for code, _ in calls] == [want for _, want in calls], calls
        m.useCorrelation(True)
        assert L.ecc_metric_evaluate_residual_histogram(m._h, w, B, ptr) == 5                       # ECC_ERR_UNSUPPORTED
        assert L.ecc_metric_evaluate_residual_histogram(m._h, 0.0, B, ptr) == 1                     # the width comes first
        assert np.all(buf == 7)
        m.close()
        vs = c.variance_dtrs(c.variances)
        m = c.metric("reference", vs)
        for floor in (0.0, -1.0, INF, float("nan")):
            assert L.ecc_metric_evaluate_variance_residual_histogram(m._h, floor, w, B, ptr) == 1
        assert L.ecc_metric_evaluate_variance_residual_histogram_pairs(m._h, C.c_void_p(bad.ctypes.data), len(bad), 1.5, w, B, ptr) == 1
        assert np.all(buf == 7)
        m.close()
        # NaN in one view's data: every sample of its pairs has d = NaN -> the overflow bin of both rows; the other pairs stay
        host = [h.copy() for h in c.host]
        host[2][:] = np.nan
        data = [E.RadonIntermediate.from_host(gpu_ctx, h, c.n_u, c.n_v) for h in host]
        mn = E.MetricRadonIntermediate(gpu_ctx, c.Ps, data).setSampling("reference")
        mn.setObjectRadius(c.radius)
        mn.setEpipolarPlaneStep(c.dkappa)
        clean = _raw_metric(c, "reference")
        got, want = mn.evaluate_residual_histogram(w, B), clean.evaluate_residual_histogram(w, B)
        with_2 = clean.evaluate_residual_histogram_pairs(np.array([t for t in idx if 2 in t[2:]], np.int32), w, B)
        assert got[2, -1] == want[2].sum() and not got[2, :-1].any()
        assert np.array_equal(got.sum(axis=1), want.sum(axis=1))
        others = [v for v in range(c.n) if v != 2]
        assert np.array_equal(got[others, :-1], (want - with_2)[others, :-1])
        mn.close()
        clean.close()
        for d in data:
            d.close()
    finally:
        c.close()


@pytest.mark.parametrize("case", ["d", "j"], indirect=True)
def test_sample_robust_scale_against_the_statement(case):
    """sample_robust_scale, raw and with a floor, against k x the statement's quantile of all samples.  The histogram's quantile is
    exact to within one bin of the last width used, and a width w is only kept when the quantile lies below (n_bins - 1) w, while
    w / 2 was left because it did not: w <= 2 Q / (n_bins - 1).  So the bar is max(first width, 2 Q / (n_bins - 1)) + tau, k
    times.  The default first width (4 x robust_scale over the bins) and a first width 1000 times too small, which takes the
    doubling path to the same bar; q outside [0, 1] is refused; NaN data with q = 1 stays in the overflow bin and ends in
    RuntimeError after the 32 doublings."""
    E, B, k = case.E, 64, 1.4826
    sampling = case.setups[0][0]
    reference = T.tolerance(sampling, case.N) == T.TOL_REFERENCE
    vs = case.variance_dtrs(case.variances)
    for kind, m, floor in (("raw", _raw_metric(case, sampling), None), ("variance", case.metric(sampling, vs), H.FLOOR)):
        a = H.all_values(case.label, kind)
        tau = H.tau_of(case.label, kind, reference)
        if floor is None:
            first = 4.0 * E.robust_scale(m.evaluate_robust(1, INF, want_pairs=True)[-1]) / B
        else:
            first = 4.0 * E.variance_robust_scale(m.evaluate_variance_robust(1, INF, floor, want_pairs=True)[-1]) / B
        for q in (0.5, 0.9, 0.999):
            Q = float(np.quantile(a, q))
            bar = k * (max(first, 2.0 * Q / (B - 1)) + tau)
            got = E.sample_robust_scale(m, q=q, k=k, n_bins=B, floor=floor)
            doubled = E.sample_robust_scale(m, q=q, k=k, n_bins=B, floor=floor, first_width=1e-3 * Q / (B - 1))
            print("case %s %s q %.3f: statement %.6g, default %.6g, from a small first width %.6g, bar %.3g" % (case.label, kind, q, k * Q, got, doubled, bar))
            assert abs(got - k * Q) <= bar, (kind, q, got, k * Q, bar)
            assert abs(doubled - k * Q) <= k * (2.0 * Q / (B - 1) + tau), (kind, q, doubled, k * Q)
        for q in (-0.1, 1.5, float("nan")):
            with pytest.raises(ValueError):
                E.sample_robust_scale(m, q=q, floor=floor)
        with pytest.raises(ValueError):
            E.sample_robust_scale(m, floor=floor, first_width=0.0)
        m.close()
    host = [h.copy() for h in case.host]
    host[1][:] = np.nan
    kw = {} if case.derivative else dict(filter=E.FILTER_NONE)
    data = [E.RadonIntermediate.from_host(case.ctx, h, case.n_u, case.n_v, **kw) for h in host]
    mn = E.MetricRadonIntermediate(case.ctx, case.Ps, data).setSampling(sampling)
    mn.setObjectRadius(case.radius)
    mn.setEpipolarPlaneStep(case.dkappa)
    try:
        with pytest.raises(RuntimeError, match="overflow bin"):
            E.sample_robust_scale(mn, q=1.0, n_bins=B, first_width=1.0)
        clean_share = 1.0 - 2.0 / case.n   # the pairs without view 1: their quantiles are still reachable
        assert np.isfinite(E.sample_robust_scale(mn, q=0.5 * clean_share, n_bins=B, first_width=1.0))
    finally:
        mn.close()
        for d in data:
            d.close()
