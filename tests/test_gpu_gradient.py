"""ecc_metric_evaluate_gradient (csrc/ecc_gradient.hip): the metric and the 2 p central-difference probes over p pose parameters of
ONE view in one call.  By default the probes go through the pose batch ("path 1"); with ecc_debug_set_gradient_launch their records
and sampling are ONE launch (csrc/small_poses_kernel.hip, "path 2") in front of the pose batch's segmented sum -- opt-in because it
measured no faster, switched on here wherever path 2 is asserted.

The contract (include/ecc_hip.h): every probe has THE BITS of ecc_metric_evaluate_pose_deltas for "the current matrices with the
view replaced by that probe", hence of setProjectionMatrices + evaluate on those matrices; the value has the bits of evaluate();
grad[p] = (probes[2p] - probes[2p + 1]) / (2.0 * h[p]) in binary64; the metric is left as evaluate_pose_deltas leaves it; what
path 2 declines goes through the pose batch (path 1) or sequentially (path 0) inside the same call with the same bits -- and
last_gradient_path() says which, which every case below ASSERTS: a run in which everything fell back would prove nothing."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEPS = np.array([0.5, 0.5, 0.5, np.deg2rad(0.1), np.deg2rad(0.1), np.deg2rad(0.1)])  # mm, mm, mm, rad, rad, rad
NAMES = ("tx", "ty", "tz", "rx", "ry", "rz")


def _scan(gpu_ctx, n, S=128, B=48, seed=5):
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import synthetic
    rng = np.random.default_rng(seed)
    Ps = synthetic.short_scan(n, S, S, 0.308 * 1024 / S)
    base = [E.RadonIntermediate.from_host(gpu_ctx, rng.standard_normal((B, B)).astype(np.float32), S, S) for _ in range(7)]
    return Ps, base, [base[v % 7] for v in range(n)]


def _rigid_probes(P34, steps=STEPS):
    """(12, 12) column-major rows plus_0, minus_0, plus_1, ... of the six rigid parameters, composed as the library composes."""
    from epipolarconsistency_amd import geometry as G, pack_projection_matrices
    out = []
    for k in range(6):
        for sign in (1.0, -1.0):
            out.append(G.compose_transform(P34, G.rigid_transform(**{NAMES[k]: sign * steps[k]})))
    return pack_projection_matrices(out)


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _sequential(ref, P0, view, rows):
    """setProjectionMatrices + evaluate one by one on `ref`: the probes, then the base."""
    out = []
    for row in rows:
        P = P0.copy()
        P[view] = row
        out.append(ref.setProjectionMatrices(P).evaluate())
    return np.array(out), ref.setProjectionMatrices(P0.copy()).evaluate()


def _check_rigid(a, b, ref, P0, view, want_path, steps=STEPS):
    """One evaluate_gradient_rigid on `a` against evaluate_pose_deltas on `b` and the sequential calls on `ref`."""
    rows = _rigid_probes(P0[view].reshape(4, 3).T, steps)
    value, grad, probes = a.evaluate_gradient_rigid(view, steps, want_probes=True)
    assert a.last_gradient_path() == want_path, (a.last_gradient_path(), want_path)
    deltas = b.evaluate_pose_deltas([[view]] * 12, list(rows[:, None, :]))
    seq, base = _sequential(ref, P0, view, rows)
    assert np.array_equal(_bits(probes), _bits(deltas)), (probes - deltas)
    assert np.array_equal(_bits(probes), _bits(seq)), (probes - seq)
    assert _bits(value)[0] == _bits(base)[0], (value, base)
    assert np.array_equal(_bits(grad), _bits((probes[0::2] - probes[1::2]) / (2.0 * steps)))
    value2, grad2 = a.evaluate_gradient_rigid(view, steps)   # without the probes: the same numbers
    assert _bits(value2)[0] == _bits(value)[0] and np.array_equal(_bits(grad2), _bits(grad))
    assert a.last_gradient_path() == want_path
    return value, grad, probes


def _close(metrics, base):
    for m in metrics:
        m.close()
    for d in base:
        d.close()


@pytest.mark.parametrize("n,mode", [(8, "auto"), (8, "polynomial"), (64, "auto"), (64, "polynomial"), (258, "auto"), (344, "polynomial")])
def test_probes_value_and_gradient_have_the_sequential_bits(gpu_ctx, n, mode):
    """n = 8 under "auto": 28 pairs, the reference arithmetic; 64: 2 016 pairs, 768 entries, four waves per pair; 258: 33 153 pairs
    (the sixteen-slice sum and finish_poses_kernel), 3 096 entries, two waves per pair; 344: 4 128 entries, one wave per pair --
    the launch shape of 400 views.  A moved view in the middle and the last view."""
    import epipolarconsistency_amd as E
    Ps, base, dtrs = _scan(gpu_ctx, n, B=32 if n > 100 else 48)
    P0 = E.pack_projection_matrices(Ps)
    a = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling(mode)
    b = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling(mode)
    ref = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling(mode).setPoseBatching(False)
    _check_rigid(a, b, ref, P0, n // 2, 1)   # the default: the pose batch
    a.debugSetGradientLaunch(True)
    for view in (n // 2, n - 1):
        _check_rigid(a, b, ref, P0, view, 2)
    _close((a, b, ref), base)


@pytest.mark.parametrize("setup", ["per_sample", "reference", "polynomial", "auto", "dkappa", "radius", "radius_view0", "incremental",
                                   "no_record_reuse", "no_small_eval"])
def test_every_taken_state_has_the_bits_on_path_2(gpu_ctx, setup):
    """With the launch switched on: the sampling modes of tests/test_gpu_sampling_modes.py, a user dkappa, a fixed radius (view 0 too: it is a view like any
    other then), the pose-delta mode, record reuse and the one-launch evaluation switched off: all taken by the new launch."""
    import epipolarconsistency_amd as E
    n = 20
    Ps, base, dtrs = _scan(gpu_ctx, n)
    P0 = E.pack_projection_matrices(Ps)

    def make():
        m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs)
        if setup in ("per_sample", "reference", "polynomial", "auto"):
            m.setSampling(setup)
        elif setup == "dkappa":
            m.setEpipolarPlaneStep(0.004)
        elif setup in ("radius", "radius_view0"):
            m.setObjectRadius(70.0)
        elif setup == "incremental":
            m.setIncremental(True)
        elif setup == "no_record_reuse":
            m.setRecordReuse(False)
        elif setup == "no_small_eval":
            m.setSmallEval(False)
        return m
    a, b, ref = make().debugSetGradientLaunch(True), make(), make().setPoseBatching(False)
    for view in ((0, 7) if setup == "radius_view0" else (11, n - 1)):
        _check_rigid(a, b, ref, P0, view, 2)
    _close((a, b, ref), base)


def test_declined_states_go_the_existing_way_with_the_same_bits(gpu_ctx):
    """The default (launch off: path 1) and every condition include/ecc_hip.h lists as declined with the launch on: the same
    bits, and the path the header promises."""
    import epipolarconsistency_amd as E
    n = 70   # 2 415 pairs: above the 2 048 up to which the reference arithmetic groups its sums per workgroup
    Ps, base, dtrs = _scan(gpu_ctx, n)
    P0 = E.pack_projection_matrices(Ps)

    def trio(prepare):
        return prepare(E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs)), prepare(E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs)), \
            prepare(E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs)).setPoseBatching(False)
    made = []
    # use_corr; the reference arithmetic chosen explicitly on more than 2 048 pairs; the debug switch
    for prepare in (lambda m: m.useCorrelation(True), lambda m: m.setSampling("reference")):
        a, b, ref = trio(prepare)
        made += [a, b, ref]
        a.debugSetGradientLaunch(True)
        _check_rigid(a, b, ref, P0, 33, 1)
    a, b, ref = trio(lambda m: m)
    made += [a, b, ref]
    _check_rigid(a, b, ref, P0, 33, 1)   # the default
    a.debugSetGradientLaunch(True)
    _check_rigid(a, b, ref, P0, 33, 2)
    a.debugSetGradientLaunch(False)
    _check_rigid(a, b, ref, P0, 33, 1)
    a.debugSetGradientLaunch(True)
    _check_rigid(a, b, ref, P0, 34, 2)
    # pose batching off: every probe sequentially
    a.setPoseBatching(False)
    _check_rigid(a, b, ref, P0, 33, 0)
    a.setPoseBatching(True)
    # view 0 under the automatic radius: path 1 as soon as one probe changes the radius (the launches take it as a float)
    radius0 = np.float32(ref.setProjectionMatrices(P0.copy()).getObjectRadius())
    changed = False
    for row in _rigid_probes(P0[0].reshape(4, 3).T):
        P = P0.copy()
        P[0] = row
        changed = changed or np.float32(ref.setProjectionMatrices(P).getObjectRadius()) != radius0
    ref.setProjectionMatrices(P0.copy())
    assert changed   # (the translations move the source: the estimate follows)
    _check_rigid(a, b, ref, P0, 0, 1)
    # more probes than the launch holds: 40 parameters
    rng = np.random.default_rng(3)
    from epipolarconsistency_amd import geometry as G
    view, p = 21, 40
    h = rng.uniform(0.1, 0.9, p) * np.where(np.arange(p) % 7 == 3, -1.0, 1.0)   # (a negative step is a step)
    dirs = rng.standard_normal((p, 3))
    P34 = P0[view].reshape(4, 3).T
    plus = [G.compose_transform(P34, G.rigid_transform(*(h[k] * dirs[k]))) for k in range(p)]
    minus = [G.compose_transform(P34, G.rigid_transform(*(-h[k] * dirs[k]))) for k in range(p)]
    value, grad, probes = a.evaluate_gradient(view, plus, minus, h, want_probes=True)
    assert a.last_gradient_path() == 1
    rows = E.pack_projection_matrices([M for pm in zip(plus, minus) for M in pm])
    assert np.array_equal(_bits(probes), _bits(b.evaluate_pose_deltas([[view]] * (2 * p), list(rows[:, None, :]))))
    seq, base_value = _sequential(ref, P0, view, rows)
    assert np.array_equal(_bits(probes), _bits(seq)) and _bits(value)[0] == _bits(base_value)[0]
    assert np.array_equal(_bits(grad), _bits((probes[0::2] - probes[1::2]) / (2.0 * h)))
    # eight parameters are the most the launch holds
    value8, grad8, probes8 = a.evaluate_gradient(view, plus[:8], minus[:8], h[:8], want_probes=True)
    assert a.last_gradient_path() == 2
    assert np.array_equal(_bits(probes8), _bits(probes[:16])) and np.array_equal(_bits(grad8), _bits(grad[:8])) and value8 == value
    value9, grad9 = a.evaluate_gradient(view, plus[:9], minus[:9], h[:9])
    assert a.last_gradient_path() == 1 and np.array_equal(_bits(grad9), _bits(grad[:9])) and value9 == value
    _close(made, base)


def test_the_metric_is_left_as_found(gpu_ctx):
    """The current matrices stay; a following evaluate() and evaluate_pose_deltas have their old bits; gradient calls
    interleaved with setProjectionMatrices of another view (the kept base values are redone for that view's pairs only)."""
    import epipolarconsistency_amd as E
    n = 40
    Ps, base, dtrs = _scan(gpu_ctx, n)
    P0 = E.pack_projection_matrices(Ps)
    a = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).debugSetGradientLaunch(True)
    b = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs)
    ref = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setPoseBatching(False)
    before = a.evaluate()
    rows = _rigid_probes(P0[9].reshape(4, 3).T)
    deltas_before = a.evaluate_pose_deltas([[9]] * 12, list(rows[:, None, :]))
    value, grad, probes = _check_rigid(a, b, ref, P0, 9, 2)
    assert all(np.array_equal(p, q) for p, q in zip(a.getProjectionMatrices(), ref.getProjectionMatrices()))
    assert _bits(a.evaluate())[0] == _bits(before)[0] == _bits(value)[0]
    assert np.array_equal(_bits(a.evaluate_pose_deltas([[9]] * 12, list(rows[:, None, :]))), _bits(deltas_before))
    assert np.array_equal(_bits(probes), _bits(deltas_before))
    # an optimiser's loop: another view moves between the gradient calls, then the gradient's own view
    from epipolarconsistency_amd import geometry as G
    P = P0.copy()
    for it, (moved, view) in enumerate([(3, 9), (17, 9), (9, 9), (39, 20), (0, 20)]):
        P = P.copy()
        P[moved] = E.pack_projection_matrices([G.compose_transform(P[moved].reshape(4, 3).T,
                                                                   G.rigid_transform(tx=0.3 * (it + 1), rz=0.002))])[0]
        a.setProjectionMatrices(P)
        b.setProjectionMatrices(P.copy())
        _check_rigid(a, b, ref, P, view, 2)
    _close((a, b, ref), base)


def test_probes_and_value_against_the_oracle(gpu_ctx, oracle_mod, small_scan):
    """oracle.evaluate_all on the small golden scan, the library's default sampling mode (28 pairs: the CPU path's own arithmetic,
    the mode tests/test_gpu_fuzz.py holds problems of this size to 1e-5 in): every probe and the value within the project's parity
    target, 1e-5 relative.  Nothing is asserted about the DIFFERENCE against the oracle: it inherits cancellation, and the bit
    contract ties it to paths that are oracle-tested."""
    import epipolarconsistency_amd as E
    s = small_scan
    dtrs = [E.RadonIntermediate.from_host(gpu_ctx, d, s["n_u"], s["n_v"]) for d in s["dtrs"]]
    m = E.MetricRadonIntermediate(gpu_ctx, s["Ps"], dtrs).setSampling("auto").debugSetGradientLaunch(True)
    P0 = E.pack_projection_matrices(s["Ps"])
    for view in (4, 7):
        value, grad, probes = m.evaluate_gradient_rigid(view, STEPS, want_probes=True)
        assert m.last_gradient_path() == 2
        rows = _rigid_probes(P0[view].reshape(4, 3).T)
        want_value = oracle_mod.evaluate_all(s["Ps"], s["dtrs"], s["n_u"], s["n_v"])["mean"]
        print("value", value, want_value, abs(value - want_value) / want_value)
        assert abs(value - want_value) <= 1e-5 * want_value
        for k, row in enumerate(rows):
            Pk = [np.asarray(P, np.float64) for P in s["Ps"]]
            Pk[view] = row.reshape(4, 3).T
            want = oracle_mod.evaluate_all(Pk, s["dtrs"], s["n_u"], s["n_v"])["mean"]
            print("view", view, "probe", k, probes[k], want, abs(probes[k] - want) / want)
            assert abs(probes[k] - want) <= 1e-5 * want, (view, k, probes[k], want)
    _close((m,), dtrs)


def test_the_gradient_points_away_from_the_consistent_pose(gpu_ctx, small_scan):
    """Consistent synthetic data, the last view displaced along tx: at +2 mm the metric rises with tx, at -2 mm it falls (on the
    CPU oracle the metric of this scan and view is 6147 5928 5748 5611 5516 5466 5461 5503 5593 5732 5918 6155 6436 over
    tx = -3 ... 3 mm in steps of 0.5: monotone on both sides of its minimum over +-3 mm)."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import geometry as G
    s = small_scan
    dtrs = [E.RadonIntermediate.from_host(gpu_ctx, d, s["n_u"], s["n_v"]) for d in s["dtrs"]]
    view = 7
    m = E.MetricRadonIntermediate(gpu_ctx, s["Ps"], dtrs).setSampling("auto").debugSetGradientLaunch(True)
    for tx, sign in ((2.0, 1.0), (-2.0, -1.0)):
        Ps = [np.asarray(P, np.float64) for P in s["Ps"]]
        Ps[view] = G.compose_transform(Ps[view], G.rigid_transform(tx=tx))
        value, grad = m.setProjectionMatrices(Ps).evaluate_gradient_rigid(view, STEPS)
        assert m.last_gradient_path() == 2
        print("tx", tx, "value", value, "grad", grad)
        assert sign * grad[0] > 0.0, (tx, grad)
    _close((m,), dtrs)


def test_argument_errors(gpu_ctx):
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd._lib import EccError
    n = 6
    Ps, base, dtrs = _scan(gpu_ctx, n)
    P0 = E.pack_projection_matrices(Ps)
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs)
    rows = _rigid_probes(P0[2].reshape(4, 3).T)
    plus, minus = rows[0::2], rows[1::2]
    before = m.evaluate()
    for h in (np.array([0.5, 0.0, 0.5, 0.1, 0.1, 0.1]), np.array([0.5, 0.5, np.nan, 0.1, 0.1, 0.1]),
              np.array([0.5, 0.5, 0.5, np.inf, 0.1, 0.1])):
        with pytest.raises(EccError):
            m.evaluate_gradient(2, plus, minus, h)
    for view in (-1, n, n + 100):
        with pytest.raises(EccError):
            m.evaluate_gradient(view, plus, minus, STEPS)
        with pytest.raises(ValueError):
            m.evaluate_gradient_rigid(view, STEPS)
    with pytest.raises(ValueError):
        m.evaluate_gradient(2, plus[:5], minus, STEPS)
    assert m.evaluate() == before   # nothing was launched, nothing changed
    empty = E.MetricRadonIntermediate(gpu_ctx, None, dtrs)   # Radon intermediates, no matrices
    with pytest.raises(EccError):
        empty.evaluate_gradient(2, plus, minus, STEPS)
    with pytest.raises(ValueError):
        empty.evaluate_gradient_rigid(2, STEPS)
    _close((m, empty), base)
