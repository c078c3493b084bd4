"""ecc_metric_evaluate_transforms (csrc/ecc_transforms.hip): K rigid source-to-target transforms of two scans as ONE compose /
E1 / list launch, ONE record launch, ONE pair launch and ONE segmented float64 sum (the registration of two scans; ref:
tools/Registration/Registration3D3D.hxx:56-62, :91-110, which the reference evaluates one setProjectionMatrices +
evaluate(indices) at a time).

The contract: every mean and every pair value is BIT-IDENTICAL to ecc_metric_set_projections(composed matrices) +
ecc_metric_evaluate_pairs(the n_source x n_target cross list) -- whatever the list length (the one-launch path, the automatic
mode's threshold, whole float4s and tails, the sixteen-slice sum), the sampling mode, the object radius (under the automatic
one every transform has its OWN radius, served inside the batch), use_corr, a user dkappa, batches that split, and whatever the
metric did before; and the call leaves the metric as it found it.  The values are also held against the oracle directly."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the tolerances tests/test_gpu_parity.py::test_index_list_and_subset holds index lists to (its :160-161, :172-173)
REL_MEAN_LIST = 5e-5   # mean of a list, polynomial mode
REL_PAIR = 2e-4        # a single pair value, polynomial mode (tests/test_gpu_parity.py:16)
REL_AUTO = 1e-6        # mean and every pair in the default mode (few pairs: the CPU path's own arithmetic)


def _scan(gpu_ctx, n, S=128, B=48, seed=5):
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import synthetic
    rng = np.random.default_rng(seed)
    Ps = synthetic.short_scan(n, S, S, 0.308 * 1024 / S)
    base = [E.RadonIntermediate.from_host(gpu_ctx, rng.standard_normal((B, B)).astype(np.float32), S, S) for _ in range(7)]
    return Ps, base, [base[v % 7] for v in range(n)]


def _cross_list(ns, nt):
    """entry q = j * ns + i -> (i, ns + j, i, ns + j), source index fast"""
    j, i = np.divmod(np.arange(ns * nt), ns)
    return np.ascontiguousarray(np.stack([i, ns + j, i, ns + j], axis=1).astype(np.int32))


def _composed(Ps, ns, T):
    from epipolarconsistency_amd import geometry
    return [geometry.compose_transform(P, T) for P in Ps[:ns]] + list(Ps[ns:])


def _transforms(K):
    """The identity, pure rotations, translations that change the automatic radius (the source moves towards / away from
    the object), general rigid motions, and two equal transforms (the last repeats the one before it)."""
    from epipolarconsistency_amd import geometry
    Ts = [np.eye(4), geometry.rigid_transform(rz=0.02), geometry.rigid_transform(rx=-0.015, ry=0.01),
          geometry.rigid_transform(tx=25.0), geometry.rigid_transform(tx=-40.0, tz=30.0)]
    k = 0
    while len(Ts) < K - 1:
        k += 1
        Ts.append(geometry.rigid_transform(tx=0.9 * k, ty=-0.4 * (k % 5), tz=0.3 * (k % 3), rz=0.0015 * k, rx=0.0007 * (k % 4)))
    Ts = Ts[:max(K - 1, 1)]
    if K >= 2:
        Ts.append(Ts[-1].copy())
    return Ts


def _sequential(b, Ps, ns, nt, Ts):
    idx = _cross_list(ns, nt)
    means, pairs = np.zeros(len(Ts)), np.zeros((len(Ts), nt, ns), np.float32)
    for k, T in enumerate(Ts):
        out = np.zeros(ns * nt, np.float32)
        means[k] = b.setProjectionMatrices(_composed(Ps, ns, T)).evaluate(idx, out)
        pairs[k] = out.reshape(nt, ns)
    return means, pairs


def _configure(m, mode, radius=0.0, dkappa=0.0, corr=False):
    m.setSampling(mode)
    m.setObjectRadius(radius)
    m.setEpipolarPlaneStep(dkappa)
    m.useCorrelation(corr)
    return m


CASES = [
    # (n_source, n_target, mode, radius, dkappa, corr)
    (1, 1, "auto", 0.0, 0.0, False), (1, 1, "polynomial", 0.0, 0.0, False), (1, 1, "reference", 80.0, 0.0, False),
    (1, 7, "auto", 0.0, 0.0, False), (1, 7, "per_sample", 0.0, 0.0, True), (1, 7, "polynomial", 90.0, 0.006, False),
    (3, 2, "auto", 0.0, 0.0, False), (3, 2, "polynomial", 0.0, 0.0, False), (3, 2, "reference", 0.0, 0.0, False),
    (20, 20, "auto", 0.0, 0.0, False), (20, 20, "polynomial", 0.0, 0.0, False), (20, 20, "per_sample", 75.0, 0.0, False),
    (20, 20, "reference", 0.0, 0.0, False), (20, 20, "polynomial", 0.0, 0.0, True), (20, 20, "auto", 0.0, 0.006, False),
    (23, 22, "auto", 0.0, 0.0, False), (23, 22, "auto", 60.0, 0.0, False),     # 506 pairs: below ECC_SAMPLING_AUTO_REFERENCE_PAIRS
    (23, 23, "auto", 0.0, 0.0, False), (23, 23, "polynomial", 110.0, 0.0, False),  # 529: above it
    (64, 65, "auto", 0.0, 0.0, False), (64, 65, "per_sample", 0.0, 0.0, False),    # 4 160 values: whole float4s
    (67, 33, "auto", 0.0, 0.0, False), (67, 33, "polynomial", 0.0, 0.006, True),   # 2 211: a tail of 3
    (181, 182, "auto", 0.0, 0.0, False), (181, 182, "polynomial", 100.0, 0.0, False),  # 32 942 values: the sixteen-slice sum
]


@pytest.mark.parametrize("ns,nt,mode,radius,dkappa,corr", CASES)
def test_transforms_have_the_sequential_bits(gpu_ctx, ns, nt, mode, radius, dkappa, corr):
    import epipolarconsistency_amd as E
    n = ns + nt
    Ps, base, dtrs = _scan(gpu_ctx, n, B=32 if n > 100 else 48)
    K = 9 if n < 200 else 5
    Ts = _transforms(K)
    assert len(Ts) == K
    a = _configure(E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs), mode, radius, dkappa, corr)
    b = _configure(E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs), mode, radius, dkappa, corr)
    if radius == 0.0:
        # the automatic radius follows the COMPOSED view 0: the case tests the per-transform radius only if they differ
        radii = {np.float32(E.host_object_radius(_composed(Ps, ns, T)[0], 128, 128)) for T in Ts}
        assert len(radii) >= 2, radii
    want_m, want_p = _sequential(b, Ps, ns, nt, Ts)
    got_m, got_p = a.evaluate_transforms(ns, Ts, want_pairs=True)
    assert a.last_batched_transforms() == K
    assert got_p.shape == (K, nt, ns) and got_p.dtype == np.float32 and got_m.dtype == np.float64
    assert np.array_equal(got_p, want_p), (np.argwhere(got_p != want_p)[:5], np.abs(got_p - want_p).max())
    assert np.array_equal(got_m, want_m), (np.flatnonzero(got_m != want_m), (got_m - want_m)[got_m != want_m])
    assert got_m[-1] == got_m[-2] and np.array_equal(got_p[-1], got_p[-2])  # two equal transforms: equal bits
    # the means alone (no pair values requested), and again in another order from whatever state the call left
    assert np.array_equal(a.evaluate_transforms(ns, Ts), want_m)
    assert np.array_equal(a.evaluate_transforms(ns, Ts[::-1]), want_m[::-1]) and a.last_batched_transforms() == K
    a.close(); b.close()
    for d in base:
        d.close()


def test_batches_that_split(gpu_ctx):
    """181 x 182 = 32 942 entries per transform: ECC_POSE_BATCH_MAX_ENTRIES = 2^20 holds 31 of them, so 40 transforms go as
    two batches (31 + 9); same bits, all of them through the batch."""
    import epipolarconsistency_amd as E
    ns, nt, K = 181, 182, 40
    Ps, base, dtrs = _scan(gpu_ctx, ns + nt, B=32)
    Ts = _transforms(K)
    a = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling("auto")
    b = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling("auto")
    want_m, want_p = _sequential(b, Ps, ns, nt, Ts)
    got_m, got_p = a.evaluate_transforms(ns, Ts, want_pairs=True)
    assert a.last_batched_transforms() == K
    assert np.array_equal(got_p, want_p) and np.array_equal(got_m, want_m), np.flatnonzero(got_m != want_m)
    a.close(); b.close()
    for d in base:
        d.close()


def test_the_metric_is_left_as_found(gpu_ctx):
    """evaluate() before and after a batch bit-equal with record reuse on (the kept records are neither used for the batch nor
    overwritten by it), with the pose-delta mode on (last_evaluated_pairs after the batch what it is without it), and an
    evaluate_pose_deltas after a batch bit-equal to one before it (the pose batch's kept base values and scratch)."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import geometry
    ns, nt = 60, 52
    n = ns + nt   # 6 216 pairs: above ECC_RECORD_REUSE_MIN_PAIRS
    Ps, base, dtrs = _scan(gpu_ctx, n)
    Ts = _transforms(7)
    P0 = E.pack_projection_matrices(Ps)
    P1 = P0.copy()
    P1[5] = (P0[5].reshape(4, 3).T @ geometry.rigid_transform(tx=0.3, rz=0.001)).T.reshape(12)

    a = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setRecordReuse(True, always=True)
    ref = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setRecordReuse(True, always=True)
    seq = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs)
    want_m, _ = _sequential(seq, Ps, ns, nt, Ts)
    before = a.evaluate()
    assert before == ref.evaluate()
    assert np.array_equal(a.evaluate_transforms(ns, Ts), want_m) and a.last_batched_transforms() == len(Ts)
    assert a.evaluate() == before
    assert [np.array_equal(x, y) for x, y in zip(a.getProjectionMatrices(), Ps)] == [True] * n
    # one view moves: the reuse path refits its pairs from the kept records, as if the batch had not happened
    assert a.setProjectionMatrices(P1).evaluate() == ref.setProjectionMatrices(P1).evaluate()
    assert np.array_equal(a.evaluate_transforms(ns, Ts[:3]), _sequential(seq, [p.reshape(4, 3).T for p in P1], ns, nt, Ts[:3])[0])
    assert a.setProjectionMatrices(P0).evaluate() == before

    # the pose-delta mode
    c = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setIncremental(True)
    d = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setIncremental(True)
    assert c.evaluate() == d.evaluate() == before
    assert np.array_equal(c.evaluate_transforms(ns, Ts), want_m) and c.last_batched_transforms() == len(Ts)
    x, y = c.setProjectionMatrices(P1).evaluate(), d.setProjectionMatrices(P1).evaluate()
    assert x == y and c.last_evaluated_pairs() == d.last_evaluated_pairs() == n - 1
    x, y = c.setProjectionMatrices(P0).evaluate(), d.setProjectionMatrices(P0).evaluate()
    assert x == y == before and c.last_evaluated_pairs() == d.last_evaluated_pairs() == n - 1

    # the pose batch around a transform batch
    views = [[3], [7, 9], [n - 1]]
    rows = [np.stack([(P0[v].reshape(4, 3).T @ geometry.rigid_transform(tx=0.2 * (q + 1), ry=0.002)).T.reshape(12) for v in vk])
            for q, vk in enumerate(views)]
    e = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs)
    first = e.evaluate_pose_deltas(views, rows)
    assert e.last_batched_poses() == 3
    assert np.array_equal(e.evaluate_transforms(ns, Ts), want_m)
    again = e.evaluate_pose_deltas(views, rows)
    assert np.array_equal(first, again) and e.last_batched_poses() == 3
    assert e.evaluate() == before
    for m in (a, ref, seq, c, d, e):
        m.close()
    for dd in base:
        dd.close()


def test_fallbacks_and_arguments(gpu_ctx):
    """setPoseBatching(False): the sequential way inside the call, same bits, nothing batched, the base matrices current again.
    No transforms: nothing happens.  Arguments are checked like the neighbours'."""
    import epipolarconsistency_amd as E
    ns, nt = 9, 6
    Ps, base, dtrs = _scan(gpu_ctx, ns + nt)
    Ts = _transforms(6)
    a = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling("auto")
    b = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs).setSampling("auto")
    want_m, want_p = _sequential(b, Ps, ns, nt, Ts)
    before = a.evaluate()
    got_m, got_p = a.evaluate_transforms(ns, Ts, want_pairs=True)
    assert a.last_batched_transforms() == 6 and np.array_equal(got_m, want_m) and np.array_equal(got_p, want_p)
    a.setPoseBatching(False)
    got_m, got_p = a.evaluate_transforms(ns, Ts, want_pairs=True)
    assert a.last_batched_transforms() == 0 and np.array_equal(got_m, want_m) and np.array_equal(got_p, want_p)
    assert a.evaluate() == before
    a.setPoseBatching(True)
    assert a.evaluate_transforms(ns, np.zeros((0, 4, 4))).shape == (0,) and a.last_batched_transforms() == 0
    one = a.evaluate_transforms(ns, Ts[1])  # a single (4, 4) matrix
    assert one.shape == (1,) and one[0] == want_m[1] and a.last_batched_transforms() == 1
    for bad_ns in (0, -1, ns + nt, ns + nt + 3):
        with pytest.raises(E.EccError) as ei:
            a.evaluate_transforms(bad_ns, Ts)
        assert ei.value.code == 1 and "n_source" in str(ei.value)
    # fewer Radon intermediates than views: a registration needs one per view
    short = E.MetricRadonIntermediate(gpu_ctx, Ps, dtrs[:ns + nt - 1])
    with pytest.raises(E.EccError) as ei:
        short.evaluate_transforms(ns, Ts)
    assert ei.value.code == 1 and "Radon intermediate" in str(ei.value)
    for m in (a, b, short):
        m.close()
    for d in base:
        d.close()


def _rel(x, y):
    return abs(x - y) / abs(y)


def test_against_the_oracle_directly(gpu_ctx, oracle_mod, small_scan):
    """4 source + 4 target views of the small scan with ORACLE dtrs, five transforms: every mean and pair value of the batch
    against oracle.evaluate_pairs(composed Ps, ...) of that transform -- not through the sequential calls."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import geometry
    s = small_scan
    ns = nt = 4
    dtrs = [E.RadonIntermediate.from_host(gpu_ctx, d, s["n_u"], s["n_v"]) for d in s["dtrs"]]
    Ts = [np.eye(4), geometry.rigid_transform(tx=4.0, ty=-2.0), geometry.rigid_transform(rz=0.02, rx=-0.01),
          geometry.rigid_transform(tx=-6.0, tz=5.0, ry=0.015), geometry.rigid_transform(tx=1.0, ty=1.0, tz=1.0, rx=0.01, ry=0.01, rz=0.01)]
    idx = _cross_list(ns, nt)
    wants = [oracle_mod.evaluate_pairs(_composed(s["Ps"], ns, T), s["dtrs"], s["n_u"], s["n_v"], idx) for T in Ts]
    m = E.MetricRadonIntermediate(gpu_ctx, s["Ps"], dtrs).setSampling("polynomial")
    for mode, tol_mean, tol_pair in (("polynomial", REL_MEAN_LIST, REL_PAIR), ("auto", REL_AUTO, REL_AUTO)):
        m.setSampling(mode)
        means, pairs = m.evaluate_transforms(ns, Ts, want_pairs=True)
        assert m.last_batched_transforms() == len(Ts)
        for k, want in enumerate(wants):
            print(mode, k, "mean rel", _rel(means[k], want["mean"]), "pair rel max",
                  np.max(np.abs(pairs[k].reshape(-1) - want["pairs"]) / np.abs(want["pairs"])))
            assert _rel(means[k], want["mean"]) < tol_mean, (mode, k, means[k], want["mean"])
            np.testing.assert_allclose(pairs[k].reshape(-1), want["pairs"], rtol=tol_pair)
    m.close()
    for d in dtrs:
        d.close()


def test_a_registration_finds_the_true_transform(gpu_ctx, oracle_mod):
    """One registration that means something: the 8 views of make_small_scan(), T_true = rigid_transform(tx=6, ty=-3, rz=0.02);
    source = views 0, 2, 4, 6 with matrices P_i inv(T_true), target = views 1, 3, 5, 7 with P_j, images projected at the true P,
    ORACLE dtrs of 96 x 96 bins, the 16 cross pairs, 21 transforms rigid_transform(tx=6+d, ty=-3, rz=0.02), d = -10 .. 10 mm,
    in one call.  The object radius is FIXED at 60 mm: the oracle's minimum is then the interior point d = 0 (5224.96; next
    best 5231.02, i.e. 1.16e-3 above -- 23 times the 5e-5 a mean may be off, so the argmin cannot flip inside the tolerance).
    Under the automatic radius the radius, and with it the kappa range, changes from transform to transform, the values of a
    sweep are not strictly comparable, and the oracle's own minimum sits at d = -1 with the runner-up 1.5e-4 above it: a
    registration caller fixes the radius."""
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import geometry
    from conftest import make_small_scan
    Ps, imgs = make_small_scan()
    n_u = n_v = 128
    dtrs_h = [oracle_mod.radon(im, 96, 96) for im in imgs]
    T_true = geometry.rigid_transform(tx=6, ty=-3, rz=0.02)
    src, tgt = [0, 2, 4, 6], [1, 3, 5, 7]
    Ps_reg = [Ps[i] @ np.linalg.inv(T_true) for i in src] + [Ps[j] for j in tgt]
    dtrs_reg = [dtrs_h[v] for v in src + tgt]
    ns = nt = 4
    idx = _cross_list(ns, nt)
    ds = np.arange(-10, 11)
    Ts = [geometry.rigid_transform(tx=6 + float(d), ty=-3, rz=0.02) for d in ds]
    want = np.array([oracle_mod.evaluate_pairs(_composed(Ps_reg, ns, T), dtrs_reg, n_u, n_v, idx, object_radius_mm=60.0)["mean"]
                     for T in Ts])
    dev = [E.RadonIntermediate.from_host(gpu_ctx, d, n_u, n_v) for d in dtrs_reg]
    m = E.MetricRadonIntermediate(gpu_ctx, Ps_reg, dev).setSampling("polynomial")
    m.setObjectRadius(60.0)
    got = m.evaluate_transforms(ns, Ts)
    assert m.last_batched_transforms() == len(Ts)
    print("oracle", want, "batch", got, "rel", np.abs(got - want) / np.abs(want))
    assert 0 < int(np.argmin(want)) < len(ds) - 1  # an interior minimum
    assert int(np.argmin(got)) == int(np.argmin(want))
    assert np.all(np.abs(got - want) / np.abs(want) < REL_MEAN_LIST), np.abs(got - want) / np.abs(want)
    m.close()
    for d in dev:
        d.close()


@pytest.mark.timeout(600)
def test_randomised_sweep_of_the_transform_batch():
    """80 random registrations (scripts/fuzz_transforms.py): batched against sequential, bit-identical."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_transforms.py"), "80", "3"], capture_output=True, text=True,
                       timeout=500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "0 of 80 cases differ" in r.stdout
