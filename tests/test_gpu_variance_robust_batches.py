"""ecc_metric_evaluate_variance_robust_pairs, _pose_deltas and _transforms on the GPU (csrc/ecc_variance_robust.hip): inverse-variance
weights and the robust loss of the studentised residual for pose optimisers and the registration of two scans, at the smallest shapes
that reach each path -- case d of tests/variance_terms.py (8 views, 96 x 64 bins, "auto": the reference arithmetic, four waves per
pair) and case a (16 views, 768 x 768 bins, the polynomial loops).  The contract of the batches is BITS: every value, mean weight,
inlier mass and pair row equals the sequential call for that list, pose or transform on a second metric, with batching on and off; the
index list is also held to the float64 statement."""
import ctypes as C

import numpy as np
import pytest

import channel_terms as T
import variance_robust_terms as VR
from test_gpu_pose_batch import _poses
from test_gpu_transforms import _composed, _cross_list, _transforms
from test_gpu_variance import _Case, _u32, _u64

pytestmark = pytest.mark.gpu

SHAPES = [("d", "auto"), ("a", "polynomial")]
LOSS, FLOOR, SCALE = "truncated", VR.FLOORS[1], "p90"   # one of the six combinations: the floor active on part of the samples
CODE = 1                                                  # ECC_LOSS_TRUNCATED


@pytest.fixture
def shape(gpu_ctx, oracle_mod, request):
    label, sampling = request.param
    c = _Case(gpu_ctx, label)
    assert (sampling, "off" if label == "a" else "auto") in c.setups
    c.sampling = sampling
    c.vs = c.variance_dtrs(c.variances)
    c.args = (CODE, float(VR.case_delta(label, SCALE)), FLOOR)
    c.metrics = []

    def metric(batching=True):
        m = c.metric(sampling, c.vs).setPoseBatching(batching)
        c.metrics.append(m)
        return m
    c.make = metric
    try:
        yield c
    finally:
        for m in c.metrics:
            m.close()
        c.close()


def _pair_index(i, j, n):
    return i * n - i * (i + 1) // 2 + (j - i - 1)


def _same(got, want):
    """The three float64 results (scalars or K-vectors) bit for bit, and the pair rows where both have them."""
    return all(np.array_equal(_u64(g), _u64(w)) for g, w in zip(got[:3], want[:3])) and \
        (len(got) < 4 or len(want) < 4 or np.array_equal(_u32(got[3]), _u32(want[3])))


@pytest.mark.parametrize("shape", SHAPES, indirect=True)
def test_index_list(shape):
    """One view's n - 1 tuples (i, j, i, j) and a permuted duplicate of them: the rows have the bits of the matching rows of the
    all-pairs call under the same resolved mode, and value, mean weight and inlier mass equal the float64 statement's sums over the
    list to 1e-5; for the other two losses the rows' bits as well."""
    n, v = shape.n, shape.n // 3
    m = shape.make()
    own = [(min(v, j), max(v, j)) for j in range(n) if j != v]
    order = np.random.default_rng(3).permutation(n - 1)
    tuples = own + [own[k] for k in order]
    idx = np.array([(i, j, i, j) for i, j in tuples], np.int32)
    rows = np.array([_pair_index(i, j, n) for i, j in tuples])
    full = m.evaluate_variance_robust(*shape.args, want_pairs=True)[3]
    value, mean_weight, inlier_mass, pairs = m.evaluate_variance_robust_pairs(idx, *shape.args, want_pairs=True)
    assert pairs.shape == (2 * (n - 1), 4) and np.array_equal(_u32(pairs), _u32(full[rows]))
    t = VR.case_terms(shape.label, LOSS, FLOOR, SCALE)
    assert len(t["pairs"]) == shape.N   # every pair is stated
    want = VR.results(t["c"][rows], t["u"][rows], t["k"][rows], len(rows))
    for got, key in ((value, "value"), (mean_weight, "mean_weight"), (inlier_mass, "inlier_mass")):
        assert abs(got - want[key]) <= T.TOL_MEAN * want[key], (key, got, want[key])
    assert inlier_mass < 1.0
    assert m.evaluate_variance_robust_pairs(idx, *shape.args) == (value, mean_weight, inlier_mass)
    assert m.evaluate_variance_robust_pairs(np.zeros((0, 4), np.int32), *shape.args) == (0.0, 0.0, 0.0)   # an empty list: nothing written
    for code in (0, 2):
        args = (code,) + shape.args[1:]
        assert np.array_equal(_u32(m.evaluate_variance_robust_pairs(idx, *args, want_pairs=True)[3]),
                              _u32(m.evaluate_variance_robust(*args, want_pairs=True)[3][rows])), code


@pytest.mark.parametrize("shape", SHAPES, indirect=True)
def test_pose_deltas(shape):
    """K = 6 poses that move one or two views or none, one of them view 0 under the automatic object radius (the sequential route
    inside the call): every value, mean weight and inlier mass has the bits of setProjectionMatrices + evaluate_variance_robust for that
    pose; the batch ran; the same bits with batching off; the set matrices are unchanged afterwards."""
    n = shape.n
    assert shape.radius == 0.0
    P0 = shape.E.pack_projection_matrices(shape.Ps)
    lists = [[n // 2], [1, n - 1], [0], [], [2, 3], [n - 1]]
    K = len(lists)
    poses, views, rows = _poses(P0, n, K, lambda k: lists[k])
    a, b = shape.make(), shape.make(batching=False)
    out = [b.setProjectionMatrices(P).evaluate_variance_robust(*shape.args) for P in poses]
    want = tuple(np.array([o[q] for o in out]) for q in range(3))
    base = b.setProjectionMatrices(P0).evaluate_variance_robust(*shape.args, want_pairs=True)
    got = a.evaluate_variance_robust_pose_deltas(views, rows, *shape.args)
    assert len(got) == 3 and _same(got, want), [g - w for g, w in zip(got, want)]
    assert K - 1 <= a.last_batched_poses() <= K    # the pose that moves view 0 changes the automatic radius: not batched
    assert len(set(want[0].tolist())) >= K - 1 and all(_u64(want[q][3])[()] == _u64(base[q])[()] for q in range(3))   # the empty pose is the base
    assert np.all(want[2] < 1.0) and len(set(want[2].tolist())) >= K - 1
    assert _same(a.evaluate_variance_robust(*shape.args, want_pairs=True), base)    # the set matrices are still the base
    a.setPoseBatching(False)
    assert _same(a.evaluate_variance_robust_pose_deltas(views, rows, *shape.args), want) and a.last_batched_poses() == 0
    assert _same(a.evaluate_variance_robust(*shape.args, want_pairs=True), base)
    # the packed form, without the mean weights and inlier masses: the C call with nulls
    from epipolarconsistency_amd import _lib
    a.setPoseBatching(True)
    off = np.array([0, 1, 2], np.int32)
    mv = np.array([n // 2, n - 1], np.int32)
    Pm = np.ascontiguousarray(np.stack([rows[0][0], rows[5][0]]))
    alone = np.zeros(2)
    assert _lib.lib().ecc_metric_evaluate_variance_robust_pose_deltas(a._h, 2, C.c_void_p(off.ctypes.data), C.c_void_p(mv.ctypes.data),
                                                                      C.c_void_p(Pm.ctypes.data), *shape.args, C.c_void_p(alone.ctypes.data),
                                                                      None, None) == 0
    assert np.array_equal(_u64(alone), _u64(want[0][[0, 5]]))
    packed = a.evaluate_variance_robust_pose_deltas_packed(off, mv, Pm, *shape.args)
    assert all(np.array_equal(_u64(packed[q]), _u64(want[q][[0, 5]])) for q in range(3))


@pytest.mark.parametrize("shape", SHAPES, indirect=True)
def test_transforms(shape):
    """n_source = 3 of 8 views, 5 of 16; five transforms, the identity among them: values, mean weights, inlier masses and pair rows
    have the bits of setProjectionMatrices(composed matrices) + evaluate_variance_robust_pairs(the cross list) per transform; all five
    went through the batch; the same bits with batching off; the metric is left as it was found."""
    n = shape.n
    ns = 3 if n == 8 else 5
    nt = n - ns
    Ts = _transforms(5)
    assert len(Ts) == 5 and np.array_equal(Ts[0], np.eye(4))
    a, b = shape.make(), shape.make()
    idx = _cross_list(ns, nt)
    values, means, masses, pairs = np.zeros(5), np.zeros(5), np.zeros(5), np.zeros((5, nt, ns, 4), np.float32)
    for k, Tk in enumerate(Ts):
        values[k], means[k], masses[k], rows = b.setProjectionMatrices(_composed(shape.Ps, ns, Tk)).evaluate_variance_robust_pairs(
            idx, *shape.args, want_pairs=True)
        pairs[k] = rows.reshape(nt, ns, 4)
    b.setProjectionMatrices(shape.Ps)
    want = (values, means, masses, pairs)
    base = a.evaluate_variance_robust(*shape.args, want_pairs=True)
    got = a.evaluate_variance_robust_transforms(ns, Ts, *shape.args, want_pairs=True)
    assert got[3].shape == (5, nt, ns, 4) and got[3].dtype == np.float32
    assert _same(got, want), (got[0] - want[0], got[1] - want[1], got[2] - want[2], np.abs(got[3] - want[3]).max())
    assert a.last_batched_transforms() == 5
    assert len(set(values[:4].tolist())) == 4 and np.all(means > 0) and np.all(masses < 1.0) and np.all(pairs[..., 1] > 0)
    assert np.all(pairs[..., 2] <= pairs[..., 1])
    assert _same(a.evaluate_variance_robust_transforms(ns, Ts, *shape.args), want[:3])      # the results alone
    assert _same(a.evaluate_variance_robust(*shape.args, want_pairs=True), base)            # the metric as it was found
    a.setPoseBatching(False)
    assert _same(a.evaluate_variance_robust_transforms(ns, Ts, *shape.args, want_pairs=True), want) and a.last_batched_transforms() == 0
    assert _same(a.evaluate_variance_robust(*shape.args, want_pairs=True), base)
    import epipolarconsistency_amd as E
    for bad_ns in (0, n):
        with pytest.raises(E.EccError) as e:
            a.evaluate_variance_robust_transforms(bad_ns, Ts, *shape.args)
        assert e.value.code == 1
    with pytest.raises(E.EccError) as e:
        a.evaluate_variance_robust_transforms(0, Ts, CODE, shape.args[1], 0.0)   # the floor before n_source
    assert "floor" in str(e.value)
