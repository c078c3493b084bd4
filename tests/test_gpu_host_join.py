"""The host-side join of the two-stream record-reuse form (ecc_metric_set_host_join, default on; not in the reference).

evaluate() and evaluate_range() queue the all-pairs launch on the context's stream and the moved views' refit and list launch on the
metric's side stream as before, then wait ON THE HOST for the side stream's event and only then queue the sum behind the all-pairs
launch -- no cross-stream wait stands between the two kernels.  The asynchronous range call, the RCCL form and a group's metrics keep
the event on the device.  The launches, their order within each stream and their arguments are the same, so the contract tested here
is: every mean, partial sum and pair value is BIT-IDENTICAL (==) to the same calls on a metric with the switch off and record reuse
off, whatever is called between two steps.

24 views, 64 x 64 projections, 48 x 48 bins: 276 pairs (above the one-launch path's 192), setRecordReuse(always=True) so that the
two-stream form runs at that size (moved views' launch first, all-pairs launch beside it); one case of 184 views (16 836 pairs, above
ECC_REFIT_FIRST_MAX_PAIRS) for the other order, the all-pairs launch first, which is the benchmark's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, S, B = 24, 64, 48
N_PAIRS = N * (N - 1) // 2


def test_adapter_setter_is_well_formed():
    """CPU: the adapter's setHostJoin against the mock Eigen header, like test_eigen_branch_is_at_least_well_formed."""
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror", "-DECC_TEST_MOCK_EIGEN",
           "-I" + os.path.join(ROOT, "tests", "cpp", "mock_eigen"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "epipolarconsistency_amd", "cpp"), os.path.join(ROOT, "tests", "cpp", "test_adapter_host_join_syntax.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.fixture(scope="module")
def scan(gpu_ctx):
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import synthetic
    rng = np.random.default_rng(41)
    Ps = synthetic.short_scan(N, S, S, 0.308 * 1024 / S)
    imgs = rng.random((N, S, S), dtype=np.float32)
    dtrs = E.RadonIntermediate.compute_batch(gpu_ctx, imgs, B, B)
    yield dict(Ps=Ps, imgs=imgs, dtrs=dtrs)
    for d in dtrs:
        d.close()


def _moved(Ps, views, k=1.0):
    import epipolarconsistency_amd as E
    out = list(Ps)
    for v in views:
        out[v] = out[v] @ E.geometry.rigid_transform(tx=0.7 * k, ty=-0.3 * k, rz=0.01 * k, ry=0.004 * (v + 1))
    return out


def _pair(gpu_ctx, Ps, dtrs):
    """The metric under test (two-stream form at every size, host join on by default) and the reference (one stream, refits everything)."""
    import epipolarconsistency_amd as E
    on = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setRecordReuse(True, always=True)
    off = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setRecordReuse(False).setHostJoin(False)
    return on, off


def _step(on, off, Ps, n_pairs=N_PAIRS):
    """set -> evaluate on both, then the pair values: mean, partial sum and every value equal."""
    a = on.setProjectionMatrices(Ps).evaluate()
    b = off.setProjectionMatrices(Ps).evaluate()
    assert a == b
    assert on.last_evaluated_pairs() == n_pairs
    sa, va = on.evaluate_range(0, n_pairs, want_pairs=True)
    sb, vb = off.evaluate_range(0, n_pairs, want_pairs=True)
    assert sa == sb and np.array_equal(va, vb)
    return a


@pytest.mark.gpu
def test_twelve_steps(gpu_ctx, scan):
    on, off = _pair(gpu_ctx, scan["Ps"], scan["dtrs"])
    first = _step(on, off, scan["Ps"])
    Ps = list(scan["Ps"])
    seen = {first}
    # one view, two, none, the first view (the automatic object radius follows it: everything is refitted), ...
    moves = [[5], [2, 17], [], [0], [23], [11], [], [3, 4], [0], [12], [7]]
    for k, views in enumerate(moves):
        Ps = _moved(Ps, views, 0.5 + 0.1 * k)
        v = _step(on, off, Ps)
        if views:
            assert v not in seen
        seen.add(v)
    assert _step(on, off, scan["Ps"]) == first  # back to a previous set of matrices: the first value again, bit for bit
    # the stamps of the last synchronous evaluation: "step queued" lies between the first launch and the sum's
    st = np.zeros(9)
    from epipolarconsistency_amd import _lib
    _lib.check(_lib.lib().ecc_debug_step_stamps(on._h, C.c_void_p(st.ctypes.data)))
    assert st[2] <= st[3] <= st[8] <= st[6] <= st[7]
    on.close()
    off.close()


@pytest.mark.gpu
def test_other_calls_between_two_steps(gpu_ctx, scan):
    """What an optimiser's surroundings call between set -> evaluate steps, each followed by a step that takes the two-stream form."""
    import epipolarconsistency_amd as E
    s = scan
    on, off = _pair(gpu_ctx, s["Ps"], s["dtrs"])
    _step(on, off, s["Ps"])
    P1, P2, P3 = _moved(s["Ps"], [9], 0.4), _moved(s["Ps"], [9, 14], 0.6), _moved(s["Ps"], [20], 0.8)
    idx = np.array([[0, 5, 0, 5], [9, 14, 9, 14], [2, 23, 2, 23]], np.int32)
    for m in (on, off):  # set -> set -> evaluate
        m.setProjectionMatrices(P1)
    _step(on, off, P2)
    # set -> a sub-range (its own kept records), then the full range again
    for first, count in ((0, 23), (100, 77), (275, 1)):
        a = on.setProjectionMatrices(P3).evaluate_range(first, count, want_pairs=True)
        b = off.setProjectionMatrices(P3).evaluate_range(first, count, want_pairs=True)
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
        a = on.setProjectionMatrices(P1).evaluate_range(first, count, want_pairs=True)  # the refit of that range, host join
        b = off.setProjectionMatrices(P1).evaluate_range(first, count, want_pairs=True)
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
    _step(on, off, P2)
    # set -> index list
    oa, ob = np.zeros(3, np.float32), np.zeros(3, np.float32)
    assert on.setProjectionMatrices(P3).evaluate(idx, oa) == off.setProjectionMatrices(P3).evaluate(idx, ob) and np.array_equal(oa, ob)
    _step(on, off, P1)
    # set -> cost image (one stream: the list launch does not write it)
    ca, cb = np.full((N, N), 2.0, np.float32), np.full((N, N), 2.0, np.float32)
    assert on.setProjectionMatrices(P2).evaluate(ca) == off.setProjectionMatrices(P2).evaluate(cb) and np.array_equal(ca, cb)
    _step(on, off, P3)
    # set -> setSampling -> evaluate, and back
    for mode in ("per_sample", "polynomial"):
        for m in (on, off):
            m.setProjectionMatrices(P1).setSampling(mode)
        _step(on, off, P1)
        _step(on, off, P2)
    # set -> refresh of one Radon intermediate -> evaluate
    for m in (on, off):
        m.setProjectionMatrices(P3).refreshRadonIntermediates(9, 1)
    _step(on, off, P3)
    # set -> a pose batch -> evaluate
    poses = [E.pack_projection_matrices(P) for P in (P1, P2, P3)]
    for m in (on, off):
        m.setProjectionMatrices(P2)
    assert np.array_equal(on.evaluate_poses(poses), off.evaluate_poses(poses))
    _step(on, off, P1)
    # set -> close with nothing evaluated; a metric closed right after a host-joined step
    on.setProjectionMatrices(P2)
    on.close()
    off.close()
    gpu_ctx.synchronize()


@pytest.mark.gpu
def test_switch_off_in_the_middle(gpu_ctx, scan):
    on, off = _pair(gpu_ctx, scan["Ps"], scan["dtrs"])
    Ps = list(scan["Ps"])
    for k, views in enumerate([[], [6], [6, 7], [1], [22], [13]]):
        if k == 3:
            on.setHostJoin(False)
        if k == 5:
            on.setHostJoin(True)
        Ps = _moved(Ps, views, 0.3 + 0.2 * k)
        _step(on, off, Ps)
    on.close()
    off.close()


@pytest.mark.gpu
def test_asynchronous_range_and_group_keep_the_device_side_join(gpu_ctx, scan, monkeypatch):
    import torch
    import epipolarconsistency_amd as E
    s = scan
    on, off = _pair(gpu_ctx, s["Ps"], s["dtrs"])
    dev = torch.device("cuda", 0)
    sums = torch.zeros(8, dtype=torch.float64, device=dev)
    vals = [torch.zeros(N_PAIRS, dtype=torch.float32, device=dev) for _ in range(8)]
    want = []
    _step(on, off, s["Ps"])
    for k in range(8):  # asynchronous calls with a synchronous, host-joined step after every second one
        P1 = _moved(s["Ps"], [k + 2] if k % 3 else [k, k + 9], 0.1 * (k + 1))
        on.setProjectionMatrices(P1)
        on.evaluate_range_async(0, N_PAIRS, sums[k:k + 1], vals[k])
        want.append(off.setProjectionMatrices(P1).evaluate_range(0, N_PAIRS, want_pairs=True))
        if k & 1:
            _step(on, off, _moved(s["Ps"], [k], 0.35))
    gpu_ctx.synchronize()
    torch.cuda.synchronize()
    assert sums.cpu().tolist() == [w[0] for w in want]
    for k in range(8):
        assert np.array_equal(vals[k].cpu().numpy(), want[k][1])
    on.close()
    # a one-rank group with the two-stream form on its rank (ECC_RECORD_REUSE=2: for every size)
    monkeypatch.setenv("ECC_RECORD_REUSE", "2")
    g = E.Group([0])
    gd = g.compute_batch(s["imgs"], B, B)
    gm = E.GroupMetricRadonIntermediate(g, s["Ps"], gd)
    for views in ([], [3], [3, 8], [0], []):
        P1 = _moved(s["Ps"], views, 0.45)
        assert gm.setProjectionMatrices(P1).evaluate() == off.setProjectionMatrices(P1).evaluate(), views
    gm.close()
    off.close()
    g.close()


@pytest.mark.gpu
def test_all_pairs_launch_first(gpu_ctx):
    """184 views, 16 836 pairs: from ECC_REFIT_FIRST_MAX_PAIRS on the all-pairs launch goes out before the refit (the benchmark's order)."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import synthetic
    rng = np.random.default_rng(43)
    n = 184
    Ps = synthetic.short_scan(n, S, S, 0.308 * 1024 / S)
    base = [E.RadonIntermediate.from_host(gpu_ctx, rng.standard_normal((B, B)).astype(np.float32), S, S) for _ in range(4)]
    dtrs = [base[v % 4] for v in range(n)]
    on = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs)  # the library's defaults: the two-stream form from 8 192 pairs on
    off = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setRecordReuse(False).setHostJoin(False)
    n_pairs = n * (n - 1) // 2
    cur = list(Ps)
    for k, views in enumerate([[], [92], [92, 183], [], [0], [17]]):
        cur = _moved(cur, views, 0.4 + 0.1 * k)
        _step(on, off, cur, n_pairs)
    on.close()
    off.close()
    for d in base:
        d.close()

