"""ecc_metric_set_form_incremental on the GPU (csrc/ecc_form_call.h: form_base_kept; csrc/form_base_scatter_kernel.hip; DESIGN.md
4.32): the base columns of the five *_pose_deltas calls of the form families kept between calls.  Two metrics run over the same data,
one with the mode on and one with it off; every comparison is on BITS (_u64 of the values and of the second and third results), and
ecc_metric_last_form_base_pairs says which path a call took: n (n - 1) / 2 on a miss, 0 on a hit, c (n - 1) - c (c - 1) / 2 when c
views were refreshed.  The shapes are the smallest that reach each path:

  case a of tests/variance_terms.py   16 views, 768 x 768 bins, polynomial sampling, the limit is 4 changed views: all five forms; a walk
                                      of six optimiser steps
  40 views of small images, AUTO      780 pairs -> polynomial; eight changed views, 0 and 39 among them: 320 grid entries, more than
                                      one workgroup of the copy kernel
  16 views of small images            the drops: slab contents + refresh_dtrs, dkappa, floor, delta, another form, the switch itself;
                                      pose batching off; the all-pairs call in between
  case d                              8 views, AUTO -> the reference arithmetic: nothing is ever kept
  case a, automatic radius            view 0 changed so that the radius moves: a miss"""
import numpy as np
import pytest

import variance_terms as V
from test_gpu_pose_batch import _perturb, _poses, _scan
from test_gpu_variance import _Case, _u64

pytestmark = pytest.mark.gpu
INF = float("inf")
CODE = 1            # ECC_LOSS_TRUNCATED
FLOOR = V.FLOORS[1]   # active on part of the samples of variance_terms' fields


class _Forms:
    """The five calls over one data set: name -> (needs the second half of a 2 n metric, method, arguments behind the lists)."""

    def __init__(self, E, ctx, Ps, data, second, sampling, radius=0.0, dkappa=0.0):
        self.E, self.ctx, self.Ps, self.n = E, ctx, Ps, len(Ps)
        self.data, self.second, self.sampling, self.radius, self.dkappa = data, second, sampling, radius, dkappa
        self.metrics, self._deltas = [], {}

    def delta(self, which):
        """robust_scale / variance_robust_scale of the rows at the scan's matrices, k = 0.5, as the float32 the calls take"""
        if which not in self._deltas:
            m = self.metric(which == "vr")
            rows = m.evaluate_variance_robust(0, INF, FLOOR, want_pairs=True)[3] if which == "vr" else m.evaluate_robust(0, INF, want_pairs=True)[2]
            scale = self.E.variance_robust_scale if which == "vr" else self.E.robust_scale
            self._deltas[which] = float(np.float32(scale(rows, 0.5)))
            assert self._deltas[which] > 0
        return self._deltas[which]

    def form(self, name):
        return {"weighted": lambda: (True, "evaluate_weighted_pose_deltas", ()),
                "robust": lambda: (False, "evaluate_robust_pose_deltas", (CODE, self.delta("r"))),
                "weighted_robust": lambda: (True, "evaluate_weighted_robust_pose_deltas", (CODE, self.delta("r"))),
                "variance": lambda: (True, "evaluate_variance_pose_deltas", (FLOOR,)),
                "variance_robust": lambda: (True, "evaluate_variance_robust_pose_deltas", (CODE, self.delta("vr"), FLOOR))}[name]()

    def metric(self, two_n):
        m = self.E.MetricRadonIntermediate(self.ctx, self.Ps, self.data + (self.second if two_n else [])).setSampling(self.sampling)
        m.setObjectRadius(self.radius)
        m.setEpipolarPlaneStep(self.dkappa)
        self.metrics.append(m)
        return m

    def pair(self, form):
        """(mode on, mode off) for the form"""
        two_n = self.form(form)[0]
        return self.metric(two_n).setFormIncremental(True), self.metric(two_n)

    def call(self, m, form, views, rows, args=None):
        _, name, own = self.form(form)
        return getattr(m, name)(views, rows, *(own if args is None else args))

    def close(self):
        for m in self.metrics:
            m.close()
        self.metrics = []


def _bits_equal(got, want):
    return len(got) == len(want) and all(np.array_equal(_u64(g), _u64(w)) for g, w in zip(got, want))


def _lists(n):
    """K = 6 poses that move one or two views, as test_gpu_variance_batches.py::test_pose_deltas builds them"""
    return [[n // 2], [1, n - 1], [0], [], [2, 3], [n - 1]]


def _move(P, views, tag):
    P = P.copy()
    for v in views:
        P[v] = _perturb(P[v], tag, v)
    return P


def _step(f, form, on, off, P, expect, lists=None, args=None, off_expect=None):
    """Both metrics at the matrices P, the K poses around P on both: the same bits; the mode-on call evaluated `expect` base pairs,
    the mode-off call all of them (off_expect: what it reports instead).  Returns the results."""
    n = len(P)
    lists = _lists(n) if lists is None else lists
    _, views, rows = _poses(P, n, len(lists), lambda k: lists[k])
    for m in (on, off):
        m.setProjectionMatrices(P)
    got, want = f.call(on, form, views, rows, args), f.call(off, form, views, rows, args)
    assert _bits_equal(got, want), (form, expect, [np.asarray(g) - np.asarray(w) for g, w in zip(got, want)])
    assert on.last_form_base_pairs() == expect, (form, on.last_form_base_pairs(), expect)
    assert off.last_form_base_pairs() == (n * (n - 1) // 2 if off_expect is None else off_expect)
    return got


@pytest.fixture(scope="module")
def case_a(gpu_ctx, oracle_mod):
    c = _Case(gpu_ctx, "a")
    assert ("polynomial", "off") in c.setups and c.n == 16 and c.radius == 0.0
    f = _Forms(c.E, gpu_ctx, c.Ps, c.data, c.variance_dtrs(c.variances), "polynomial", c.radius, c.dkappa)
    f.P0 = c.E.pack_projection_matrices(c.Ps)
    try:
        yield f
    finally:
        f.close()
        c.close()


@pytest.mark.parametrize("form", ["weighted", "robust", "weighted_robust", "variance", "variance_robust"])
def test_every_path_on_sixteen_views(case_a, form):
    """120 base pairs at the first call, 0 at a repeated one, 15 with one changed view, 54 with four, 120 with five (the limit is
    min(32, 16 / 4) = 4), 29 with views 0 and 15 changed under a fixed object radius; the K = 6 poses of every call -- one of them
    moves view 0 and goes the sequential way under the automatic radius -- have the bits of the mode-off call."""
    f, n = case_a, case_a.n
    on, off = f.pair(form)
    try:
        P = f.P0
        first = _step(f, form, on, off, P, 120)
        if len(f.form(form)[2]) >= 2:   # the loss is active: an inlier mass strictly inside (0, 1)
            assert np.all((first[-1] > 0) & (first[-1] < 1)), first[-1]
        assert len(set(np.asarray(first[0]).tolist())) >= 5   # the poses differ (the empty one is the base)
        assert _bits_equal(_step(f, form, on, off, P, 0), first)
        P = _move(P, [7], 11)
        moved = _step(f, form, on, off, P, 15)
        assert not np.array_equal(_u64(moved[0]), _u64(first[0]))
        _step(f, form, on, off, P, 0)
        P = _move(P, [2, 5, 9, 14], 12)
        _step(f, form, on, off, P, 54)
        P = _move(P, [1, 4, 6, 10, 13], 13)
        _step(f, form, on, off, P, 120)
        _step(f, form, on, off, P, 0)
        P = _move(P, [3, 4], 14)   # adjacent views: their common pair once, from the column of view 3
        _step(f, form, on, off, P, 29)
        radius = on.getObjectRadius()
        for m in (on, off):
            m.setObjectRadius(radius)   # (ecc_metric_set_params: drops what is kept)
        _step(f, form, on, off, P, 120)
        P = _move(P, [0, n - 1], 15)
        _step(f, form, on, off, P, 29)
        _step(f, form, on, off, P, 0)
        assert _bits_equal(_step(f, form, on, off, f.P0, 120), _step(f, form, on, off, f.P0, 0))   # all sixteen views back
    finally:
        on.close()
        off.close()


def test_a_walk_of_six_optimiser_steps(case_a):
    """Set one view, then 12 probes of it (the robust form): 15 base pairs at every step after the first, the same bits throughout."""
    f = case_a
    on, off = f.pair("robust")
    try:
        P = f.P0
        for s, v in enumerate([5, 9, 2, 14, 7, 11]):
            P = _move(P, [v], 20 + s)
            _step(f, "robust", on, off, P, 120 if s == 0 else 15, lists=[[v]] * 12)
            assert on.last_batched_poses() == 12
    finally:
        on.close()
        off.close()


def test_the_automatic_radius_moves_with_view_0(case_a):
    """View 0 changed so that the automatic object radius moves: every pair's record changes with it -- a miss; the same view changed
    back: a miss again."""
    f, E = case_a, case_a.E
    on, off = f.pair("variance")
    try:
        _step(f, "variance", on, off, f.P0, 120)
        r0 = on.getObjectRadius()
        P = f.P0.copy()
        P[0] = (P[0].reshape(4, 3).T @ E.geometry.rigid_transform(tz=25.0, tx=3.0)).T.reshape(12)
        for m in (on, off):
            m.setProjectionMatrices(P)
        assert np.float32(on.getObjectRadius()) != np.float32(r0)
        _step(f, "variance", on, off, P, 120)
        _step(f, "variance", on, off, P, 0)
        _step(f, "variance", on, off, f.P0, 120)
    finally:
        on.close()
        off.close()


def test_forty_views_eight_changed(gpu_ctx):
    """40 views, AUTO sampling (780 pairs: polynomial), a fixed object radius; views 0, 3, 4, 11, 20, 21, 38 and 39 change: 320 grid
    entries -- two workgroups of the copy kernel --, 8 * 39 - 28 = 284 base pairs, the same bits."""
    import epipolarconsistency_amd as E
    n = 40
    Ps, base, dtrs = _scan(gpu_ctx, n)
    probe = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs)
    radius = probe.getObjectRadius()
    probe.close()
    f = _Forms(E, gpu_ctx, Ps, dtrs, [], "auto", radius)
    try:
        on, off = f.pair("robust")
        P = E.pack_projection_matrices(Ps)
        first = _step(f, "robust", on, off, P, 780)
        assert np.all((first[1] > 0) & (first[1] < 1))
        P = _move(P, [0, 3, 4, 11, 20, 21, 38, 39], 3)
        _step(f, "robust", on, off, P, 284)
        _step(f, "robust", on, off, P, 0)
        P = _move(P, list(range(10, 20)), 4)   # ten views: the limit
        _step(f, "robust", on, off, P, 10 * 39 - 45)
        P = _move(P, list(range(20, 31)), 5)   # eleven: a miss
        _step(f, "robust", on, off, P, 780)
    finally:
        f.close()
        for d in base:
            d.close()


def test_reference_arithmetic_keeps_nothing(gpu_ctx, oracle_mod):
    """Case d: 8 views, AUTO -> the reference arithmetic, which reads the callers' slabs: 28 base pairs at every call, the same bits."""
    c = _Case(gpu_ctx, "d")
    assert ("auto", "auto") in c.setups and c.n == 8
    f = _Forms(c.E, gpu_ctx, c.Ps, c.data, c.variance_dtrs(c.variances), "auto", c.radius, c.dkappa)
    try:
        P = c.E.pack_projection_matrices(c.Ps)
        for form in ("variance", "variance_robust"):
            on, off = f.pair(form)
            _step(f, form, on, off, P, 28)
            _step(f, form, on, off, P, 28)
            _step(f, form, on, off, _move(P, [5], 2), 28)
    finally:
        f.close()
        c.close()


def test_drops(gpu_ctx):
    """16 views of small images, polynomial sampling, the second half of the 2 n metric in slabs this test owns.  What drops the kept
    columns: changed slab contents + refresh_dtrs (and the values differ from before), another dkappa, another floor, another delta,
    another form, the switch itself.  What does not: the all-pairs call of the form in between.  Pose batching off: no base columns."""
    import torch
    import epipolarconsistency_amd as E
    n, S, B = 16, 128, 48
    Ps, base, dtrs = _scan(gpu_ctx, n)
    dev = torch.device("cuda", gpu_ctx.device)
    rng = np.random.default_rng(17)
    slabs = torch.zeros((n, E.slab_floats(B, B)), dtype=torch.float32, device=dev)   # owned here: rescaled in place below
    imgs = torch.from_numpy(rng.uniform(0.5, 2.0, (n, S, S)).astype(np.float32) / S).to(dev)
    second = E.RadonIntermediate.compute_into(gpu_ctx, imgs, slabs, B, B, filter=E.FILTER_NONE)   # positive fields: line integrals
    gpu_ctx.synchronize()
    f = _Forms(E, gpu_ctx, Ps, dtrs, second, "polynomial")
    try:
        on, off = f.pair("variance")
        P = E.pack_projection_matrices(Ps)

        def step(expect, form="variance", args=None):
            return _step(f, form, on, off, P, expect, args=args)
        before = step(120)
        assert on.device_bytes()["other"] - off.device_bytes()["other"] == 2 * 120 * 4   # the kept buffer, under other_bytes
        step(0)
        on.evaluate_variance(FLOOR, want_pairs=True)   # the all-pairs call has scratch of its own
        assert _bits_equal(step(0), before)
        # the contents of the variance slabs change, then refresh_dtrs on both
        slabs[n // 2:].mul_(1.75)
        torch.cuda.synchronize(dev)
        for m in (on, off):
            m.refreshRadonIntermediates()
        after = step(120)
        assert not np.array_equal(_u64(after[0]), _u64(before[0]))
        step(0)
        for m in (on, off):
            m.refreshRadonIntermediates(3, 1)   # any range
        assert _bits_equal(step(120), after)
        for m in (on, off):
            m.setEpipolarPlaneStep(0.01)
        step(120)
        step(0)
        step(120, args=(V.FLOORS[0],))   # another floor
        step(0, args=(V.FLOORS[0],))
        step(120)
        step(120, "variance_robust")      # another form
        step(0, "variance_robust")
        step(120, "variance_robust", (CODE, 2.0 * f.delta("vr"), FLOOR))   # another delta
        step(120, "variance_robust", (0, 2.0 * f.delta("vr"), FLOOR))       # another loss
        step(120)
        step(0)
        for m in (on, off):
            m.setSampling("per_sample")
        step(120)
        step(0)
        on.setFormIncremental(False)
        step(120)
        step(120)
        on.setFormIncremental(True)
        step(120)
        step(0)
        on.setFormIncremental(True)   # any call of the switch drops
        step(120)
        for m in (on, off):
            m.setPoseBatching(False)
        _step(f, "variance", on, off, P, 0, off_expect=0)   # no base columns at all
        assert on.last_batched_poses() == 0
        for m in (on, off):
            m.setPoseBatching(True)
        step(0)                        # ... and the kept ones are still those of the matrices
    finally:
        f.close()
        for d in base:
            d.close()
        for d in second:
            d.close()
