"""ecc_metric_evaluate_variance on the GPU (csrc/ecc_variance.hip, csrc/variance_kernel.hip): the metric with inverse-variance sample
weights.  The cases are channel_terms.CASES with the data of channel 0 and the variance fields of tests/variance_terms.py -- the
geometries, grids and settings that select each kernel and loop (labels a .. j); each case asserts from the records
of a single-channel metric that it reached its loop class, as tests/test_gpu_channel_terms.py does.

  half_is_evaluate   V == 0.5f (s == 1, omega == 1), floor 0.25 and 1.0: value, the c column, the u column and the mean weight have the
                     bits of evaluate() / 1.0;
  floor_only         V == 0, floor 4 (omega == 1/4): the c column is a quarter of evaluate(cost) bit for bit, u == 0.25, value has
                     evaluate()'s bits;
  scale_invariance   all V and the floor x 4: the same value bits, both columns x 1/4 exactly;
  oracle             c and u of every pair against variance_terms at both floors (tests/test_variance_terms_oracle.py shows that this
                     comparison rejects the slips it is there for), value and mean weight to 1e-5;
  demonstration      the reason the call exists: noise in half of one view multiplies evaluate() and leaves the variance form's value;
  repeatability, errors."""
import numpy as np
import pytest

import channel_terms as T
import variance_terms as V
from test_gpu_channel_terms import _reached, _records

pytestmark = pytest.mark.gpu


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


class _Case:
    """The data of a case on the device, and metrics over them with the variance fields asked for."""

    def __init__(self, gpu_ctx, label):
        import epipolarconsistency_amd as E
        self.E, self.ctx, self.label = E, gpu_ctx, label
        self.name, self.n, self.n_alpha, self.n_t, self.radius, self.dkappa, self.derivative, self.setups = V.settings(label)
        self.Ps, self.n_u, self.n_v, self.host, self.variances, self.K01s = V.case_inputs(label)
        self.N = self.n * (self.n - 1) // 2
        gpu_ctx.setQuadCopies(self.setups[0][1])
        kw = {} if self.derivative else dict(filter=E.FILTER_NONE)
        self.data = [E.RadonIntermediate.from_host(gpu_ctx, h, self.n_u, self.n_v, **kw) for h in self.host]
        self.made = []

    def variance_dtrs(self, fields):
        vs = [self.E.RadonIntermediate.from_host(self.ctx, f, self.n_u, self.n_v, filter=self.E.FILTER_NONE) for f in fields]
        self.made += vs
        return vs

    def constant(self, value):
        """One intermediate of the constant `value`, for every view."""
        return self.variance_dtrs([np.full((self.n_t, self.n_alpha), value, np.float32)]) * self.n

    def metric(self, sampling, vs):
        m = self.E.MetricRadonIntermediate(self.ctx, self.Ps, self.data + vs).setSampling(sampling)
        m.setObjectRadius(self.radius)
        m.setEpipolarPlaneStep(self.dkappa)
        return m

    def reached(self, sampling, t):
        rec = _records(self.ctx, self.Ps, self.data, self.radius, self.dkappa)
        _reached(self.label, sampling, rec, t, self.N)
        return rec

    def close(self):
        self.ctx.setQuadCopies("auto")
        _close(self.data + self.made)


@pytest.fixture
def case(gpu_ctx, oracle_mod, request):
    c = _Case(gpu_ctx, request.param)
    try:
        yield c
    finally:
        c.close()


LABELS = sorted(V.CASES)


def _plain(m, n):
    """evaluate() and the pair order of evaluate(cost) on the same metric."""
    plain = m.evaluate()
    cost = np.full((n, n), -2.0, np.float32)
    with_cost = m.evaluate(cost)
    return plain, with_cost, _pair_order(cost)


@pytest.mark.parametrize("case", LABELS, indirect=True)
def test_half_is_evaluate(case):
    """V == 0.5f: s = 0.5f + 0.5f == 1.0f, omega == 1.0f / 1.0f == 1.0f under floor 0.25 and floor 1.0 alike (1.0f * d is d): value
    has the bits of evaluate() on the same metric, pairs[:, 0] those of evaluate(cost), pairs[:, 1] == 1.0 and the mean weight == 1.0 --
    in every case and sampling mode of the table."""
    half = case.constant(0.5)
    for sampling, _ in case.setups:
        m = case.metric(sampling, half)
        out = [m.evaluate_variance(floor, want_pairs=True) for floor in (0.25, 1.0)]
        plain, with_cost, vals = _plain(m, case.n)
        m.close()
        for value, mean_weight, pairs in out:
            assert pairs.shape == (case.N, 2) and pairs.dtype == np.float32
            assert np.array_equal(_u32(pairs[:, 0]), _u32(vals)), (sampling, np.max(np.abs(pairs[:, 0] - vals)))
            assert _u64(value)[()] == _u64(plain)[()] == _u64(with_cost)[()], (sampling, value, plain)
            assert np.all(pairs[:, 1] == 1.0) and mean_weight == 1.0, (sampling, mean_weight)
        assert (vals > 0).sum() >= 0.8 * case.N


@pytest.mark.parametrize("case", LABELS, indirect=True)
def test_floor_only(case):
    """V == 0 and floor 4: every sample's omega is 1.0f / 4.0f == 0.25f, a power of two, so every product with it is exact: pairs[:, 0]
    == 0.25f * evaluate(cost) bit for bit, pairs[:, 1] == 0.25, the mean weight 0.25, and value -- sum c / sum u, both sums scaled by
    the same power of two -- has the bits of evaluate()."""
    zero = case.constant(0.0)
    for sampling, _ in case.setups:
        m = case.metric(sampling, zero)
        value, mean_weight, pairs = m.evaluate_variance(4.0, want_pairs=True)
        plain, _, vals = _plain(m, case.n)
        m.close()
        assert np.array_equal(_u32(pairs[:, 0]), _u32(np.float32(0.25) * vals)), (sampling, np.max(np.abs(pairs[:, 0] - 0.25 * vals)))
        assert np.all(pairs[:, 1] == 0.25) and mean_weight == 0.25, (sampling, mean_weight)
        assert _u64(value)[()] == _u64(plain)[()], (sampling, value, plain)
        assert (vals > 0).sum() >= 0.8 * case.N


@pytest.mark.parametrize("case", LABELS, indirect=True)
def test_scale_invariance(case):
    """The case's fields and each of its floors, then all of them x 4 (exact in float32): every s is 4 x as large, exactly, every omega
    a quarter, exactly -- both columns x 0.25 bit for bit, and the same value bits.  Only relative variances matter."""
    vs = case.variance_dtrs(case.variances)
    vs4 = case.variance_dtrs([np.float32(4.0) * f for f in case.variances])
    for sampling, _ in case.setups:
        m, m4 = case.metric(sampling, vs), case.metric(sampling, vs4)
        for floor in V.FLOORS:
            value, mean_weight, pairs = m.evaluate_variance(floor, want_pairs=True)
            value4, mean_weight4, pairs4 = m4.evaluate_variance(4.0 * floor, want_pairs=True)
            assert np.array_equal(_u32(pairs4), _u32(np.float32(0.25) * pairs)), (sampling, floor, np.max(np.abs(pairs4 - 0.25 * pairs)))
            assert _u64(value4)[()] == _u64(value)[()], (sampling, floor, value, value4)
            assert _u64(mean_weight4)[()] == _u64(0.25 * mean_weight)[()], (sampling, floor, mean_weight, mean_weight4)
            assert np.all(pairs[:, 1] > 0) and len(set(pairs[:, 1].tolist())) > case.N // 2   # the fields are seen
        m.close()
        m4.close()


@pytest.mark.parametrize("case", LABELS, indirect=True)
def test_pair_terms_against_the_direct_statement(case):
    """c and u of every pair (case e: the statement's sample of the pairs) against the float64 statement at both floors: 1e-6 of the
    scale under the reference arithmetic, 1e-3 on the throughput paths, the scale s omega_max for c and omega_max for u; value and
    mean weight to 1e-5 relative.  The worst ratios of a GPU run are recorded in DESIGN.md 4.28."""
    vs = case.variance_dtrs(case.variances)
    failures = []
    for sampling, _ in case.setups:
        t0 = V.case_terms(case.label, V.FLOORS[0])
        rec = case.reached(sampling, t0)
        assert np.max(np.abs(rec["kmax"] - case.K01s[:, 15])) <= 1e-3   # the records describe the statement's ranges, in its pair order
        tol = T.tolerance(sampling, case.N)
        m = case.metric(sampling, vs)
        for floor in V.FLOORS:
            t = V.case_terms(case.label, floor)
            rows = t["pairs"]
            want, scales = V.columns(t)
            value, mean_weight, pairs = m.evaluate_variance(floor, want_pairs=True)
            assert np.all(np.isfinite(pairs)) and np.isfinite(value)
            ratio = T.compare(pairs[rows], want, scales, tol)
            line = "case %s %s floor %g: c %.3g of the bar %.0e, u %.3g" % (case.label, sampling, floor, ratio[0], tol, ratio[1])
            if tol == T.TOL_THROUGHPUT:   # reported: the same against the float64-position statement
                c64, _ = V.columns(V.case_terms(case.label, floor, "float64"))
                r64 = T.compare(pairs[rows], c64, scales, tol)
                line += "; against float64 positions c %.3g, u %.3g" % (r64[0], r64[1])
            if "value" in t:
                ev = abs(value - t["value"]) / (T.TOL_MEAN * t["value"])
                eu = abs(mean_weight - t["mean_weight"]) / (T.TOL_MEAN * t["mean_weight"])
                line += "; value %.3g of the bar 1e-05, mean weight %.3g" % (ev, eu)
                ratio = np.append(ratio, [ev, eu])
            print(line)
            if not ratio.max() <= 1.0:
                failures.append(line)
        m.close()
    assert not failures, "\n".join(failures)


# ---- demonstration: the reason the feature exists --------------------------------------------------------------------------------
def test_noise_in_half_of_one_view(gpu_ctx, oracle_mod):
    """8 views of the spheres at 128^2 -> 96^2 bins; a second copy with Gaussian noise of 5 % of the view's maximum on the left half
    of view 3; V = variance_intermediates of the pixel variances, floor = variance_floor of V_3.  On the device, from the device's own
    Radon intermediates: evaluate() grows at least 2-fold, and the ratio of the variance form's values is the float64 statement's
    ratio, computed from the same intermediates, to 1e-5 relative."""
    import epipolarconsistency_amd as E
    from conftest import make_small_scan
    Ps, imgs = make_small_scan()
    noisy, var = V.demo_images(imgs)
    B, n = V.DEMO_BINS, len(Ps)
    clean_d = E.RadonIntermediate.compute_batch(gpu_ctx, np.asarray(imgs, np.float32), B, B)
    noisy_d = E.RadonIntermediate.compute_batch(gpu_ctx, noisy, B, B)
    var_d = E.variance_intermediates(gpu_ctx, var, B, B)
    try:
        assert len(var_d) == n and all(v.getFilter() == E.FILTER_NONE for v in var_d)
        fields = [v.readback().copy() for v in var_d]
        floor = E.variance_floor(fields[V.DEMO_VIEW], V.DEMO_FLOOR_FRACTION)
        assert floor == V.demo_floor(fields) and floor > 0
        assert all(not f.any() for k, f in enumerate(fields) if k != V.DEMO_VIEW) and (fields[V.DEMO_VIEW] > 0).mean() > 0.2
        out, host = {}, {}
        for key, data in (("clean", clean_d), ("noisy", noisy_d)):
            m = E.MetricRadonIntermediate(gpu_ctx, Ps, data + var_d).setSampling("auto")   # 28 pairs: the reference arithmetic
            out[key] = (m.evaluate(), m.evaluate_variance(floor)[0])
            m.close()
            host[key] = [d.readback().copy() for d in data]
        K = [oracle_mod.evaluate_all(Ps, host[key], 128, 128, want_K01=True)["K01s"] for key in ("clean", "noisy")]
        p0, p1, v0, v1 = V.demo_ratios(Ps, host["clean"], host["noisy"], fields, floor, 128, 128, K[0], K[1])
        plain_ratio, variance_ratio = out["noisy"][0] / out["clean"][0], out["noisy"][1] / out["clean"][1]
        print("device: evaluate() %.1f -> %.1f, a factor of %.3f; variance form %.1f -> %.1f, a factor of %.5f; statement: %.3f and %.5f (floor %.4g)"
              % (out["clean"][0], out["noisy"][0], plain_ratio, out["clean"][1], out["noisy"][1], variance_ratio, p1 / p0, v1 / v0, floor))
        assert plain_ratio >= 2.0, out
        assert abs(variance_ratio - v1 / v0) <= 1e-5 * (v1 / v0), (variance_ratio, v1 / v0)
        assert abs(v1 / v0 - 1.0) <= 0.05
    finally:
        _close(clean_d + noisy_d + var_d)


# ---- repeatability, errors -------------------------------------------------------------------------------------------------------
def test_repeatable_and_nothing_else_moved(gpu_ctx, oracle_mod):
    """Two calls give identical bits; evaluate() and a pose batch around the call are unchanged; without the pair terms the same two
    numbers."""
    c = _Case(gpu_ctx, "i")
    try:
        n = c.n
        m = c.metric("polynomial", c.variance_dtrs(c.variances))
        P0 = c.E.pack_projection_matrices(c.Ps)

        def observe():
            cost = np.zeros((n, n), np.float32)
            return np.concatenate([[m.evaluate(), m.evaluate(cost)], np.ravel(m.evaluate_pose_deltas([n // 2, 1], np.stack([P0[1], P0[2]])))]), cost
        before, cost_b = observe()
        first = m.evaluate_variance(V.FLOORS[1], want_pairs=True)
        second = m.evaluate_variance(V.FLOORS[1], want_pairs=True)
        after, cost_a = observe()
        assert np.array_equal(_u64(before), _u64(after)) and np.array_equal(_u32(cost_b), _u32(cost_a))
        assert _u64(first[0])[()] == _u64(second[0])[()] and _u64(first[1])[()] == _u64(second[1])[()]
        assert np.array_equal(_u32(first[2]), _u32(second[2]))
        assert m.evaluate_variance(V.FLOORS[1]) == first[:2]
        other = m.evaluate_variance(V.FLOORS[0], want_pairs=True)
        assert other[0] != first[0] and other[1] > first[1]    # the floor is seen
        m.close()
    finally:
        c.close()


def test_errors(gpu_ctx, oracle_mod):
    import epipolarconsistency_amd as E
    c = _Case(gpu_ctx, "d")
    try:
        vs = c.variance_dtrs(c.variances)
        m = c.metric("auto", vs)
        want = m.evaluate_variance(1.5, want_pairs=True)
        for floor in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(E.EccError) as e:
                m.evaluate_variance(floor)
            assert e.value.code == 1, (floor, e.value)   # ECC_ERR_INVALID_ARGUMENT
        m.useCorrelation(True)
        with pytest.raises(E.EccError) as e:
            m.evaluate_variance(1.5)
        assert e.value.code == 5, e.value   # ECC_ERR_UNSUPPORTED
        with pytest.raises(E.EccError) as e:
            m.evaluate_variance(0.0)
        assert e.value.code == 1, e.value   # the floor is checked before use_corr
        m.useCorrelation(False)
        again = m.evaluate_variance(1.5, want_pairs=True)
        assert _u64(again[0])[()] == _u64(want[0])[()] and np.array_equal(_u32(again[2]), _u32(want[2]))
        m.close()
        for dtrs in (c.data, c.data + vs[:-1], c.data + vs + vs[:1]):   # n, 2 n - 1, 2 n + 1 intermediates
            bad = E.MetricRadonIntermediate(gpu_ctx, c.Ps, dtrs)
            with pytest.raises(E.EccError) as e:
                bad.evaluate_variance(1.5)
            assert e.value.code == 1, (len(dtrs), e.value)
            bad.close()
        one = E.MetricRadonIntermediate(gpu_ctx, c.Ps[:1], [c.data[0], vs[0]])   # fewer than two views
        with pytest.raises(E.EccError) as e:
            one.evaluate_variance(1.5)
        assert e.value.code == 1
        one.close()
        none = E.MetricRadonIntermediate(gpu_ctx, None, c.data + vs)   # no matrices set
        with pytest.raises(E.EccError) as e:
            none.evaluate_variance(1.5)
        assert e.value.code == 1
        none.close()
    finally:
        c.close()
