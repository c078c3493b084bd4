"""The metric's DIFFERENCES between nearby poses against the float64-geometry oracle.

An optimiser (Gui/SingleImageMotion.h, the NLopt wrapper, config 5's 6-DoF sweep) moves one view and compares the metric at
nearby poses; a finite difference subtracts two sums that agree to parts in 1e4.  The value bars of the other parity tests
(mean 1e-5) allow a difference error ~1e3 times what the reference arithmetic itself makes.  Here every case evaluates the
6-DoF pose grid of one view (tests/pose_response.py: h in {1, 0.1, 0.01, 0.001} mm and {1e-3 .. 1e-6} rad, both signs, and the
base pose: 49 poses) with ONE evaluate_pose_deltas call per sampling mode, and measures the central difference S(+h) - S(-h)
and the second difference S(+h) - 2 S(0) + S(-h) of S = mean * n_pairs against the oracle with every sample coordinate exact
(tests/pose_response.py "x": variant 1's float64 geometry, and the texel position and weights in float64 too): e_gpu for the library, e0 for the normative oracle (variant 0).

  A  config-2 shape: short scan, 64 views of 512^2, 768 x 768 bins, view 31 moved
  B  the angulated orbit (tests/geometry_catalog.py), 130 views, 512 x 790 bins, view 65
  C  scattered poses, 48 views, 1000 x 767 bins, view 40: a 1-5 mm short-baseline repeat of view 0 (kappa_max = pi/2, refused)
  D  short scan, 32 views of 256^2, 192 x 192 bins (496 pairs: the default mode takes the reference arithmetic), view 15
  E  case A with view 0 moved (tx, rz): every pair changes (the object radius follows view 0); oracle: evaluate_all
  F  case A with a user dkappa of 0.004

Bars (per case and mode, over all its cells): p50(e_gpu) <= 1.25 p50(e0) and max(e_gpu) <= 2 max(e0); reference mode also
within 1e-6 S_moved of variant 0.
Why not variant 1 alone: it rounds the angle and distance to float32 and forms the texel position in float32 as the reference
does, so its differences share variant 0's rounding and e0 against it cancels.  Against variant 1 the polynomial path measured
p50 1.29x / max 2.37x e0 on B and max 8.8x on F (per-sample 7.3x); against exact sampling the same runs are p50 0.47x / max 1.09x
(B) and max 0.57x / 0.32x (F) -- variant 1 itself is 17.7 off the exact sums on F's tz 1 mm cells, the library 11.6 / 6.5, the
normative oracle 20.4.  Non-vacuity, per DoF: its largest step is above 10x the largest e0 of its own cells and the best-resolved
DoF is above 1e3x (measured: the DoFs below 1e3x are rz on A 74x, rz on D 250x, rx / rz on F 340x / 600x;
rz barely moves a short scan); the smallest step of some DoF reaches the noise floor.  Same samples: the kappa sample
count of every moved pair at every pose is the oracle's (kappa_max measured bit-equal on all of them).  Class boundaries (B, C):
poses 1e-7 mm apart on either side of a change of a moved pair's degree, clamp class or fit acceptance meet the per-pair bar of
tests/test_gpu_geometry_parity.py and bar 1.  Negative control: a coarse economisation fails bar 1."""
import numpy as np
import pytest

import geometry_catalog as G
import pose_response as R

pytestmark = pytest.mark.gpu

Q50, QMAX = 1.25, 2.0
T_BAD = 3e-4  # economisation bound (bins) that fails the difference bar (test_negative_control_...)

CASES = {
    "A": dict(geom="short", n=64, size=512, pixel=0.616, bins=(768, 768), v=31, dkappa=0.0,
              modes=("polynomial", "per_sample", "reference", "auto")),
    "B": dict(geom="angulated", n=130, bins=(512, 790), v=65, dkappa=0.0, modes=("polynomial", "per_sample", "reference")),
    "C": dict(geom="scattered", n=48, bins=(1000, 767), v=40, dkappa=0.0, modes=("polynomial", "per_sample", "reference")),
    "D": dict(geom="short", n=32, size=256, pixel=1.232, bins=(192, 192), v=15, dkappa=0.0, modes=("auto",)),
    "E": dict(geom="short", n=64, size=512, pixel=0.616, bins=(768, 768), v=0, dkappa=0.0, dofs=("tx", "rz"),
              modes=("polynomial", "per_sample", "reference")),
    "F": dict(geom="short", n=64, size=512, pixel=0.616, bins=(768, 768), v=31, dkappa=0.004,
              modes=("polynomial", "per_sample", "reference")),
}

_data = {}    # (geom, n, bins) -> scan on the device
_oracle = {}  # case -> the oracle's response on its pose grid
_bars = {}    # case -> e0 of its cells


@pytest.fixture(scope="module", autouse=True)
def _release_scans():
    """The cached device scans live as long as this module's tests."""
    yield
    for d in _data.values():
        for dtr in d["dtrs"]:
            dtr.close()
    _data.clear()
    _oracle.clear()


def _scan(gpu_ctx, c):
    key = (c["geom"], c["n"], c["bins"])
    if key not in _data:
        from epipolarconsistency_amd import synthetic
        if c["geom"] == "short":
            Ps = synthetic.short_scan(c["n"], c["size"], c["size"], c["pixel"])
            n_u = n_v = c["size"]
            phantom = synthetic.sphere_phantom(seed=1234, extent_mm=30.0, rmin=8.0, rmax=25.0)
        else:
            Ps, n_u, n_v = G.make(c["geom"], c["n"])
            phantom = G.phantom()
        slabs, dtrs, host = R.device_case(gpu_ctx, Ps, n_u, n_v, c["bins"][0], c["bins"][1], phantom)
        _data[key] = dict(Ps=[np.asarray(P, np.float64) for P in Ps], n_u=n_u, n_v=n_v, slabs=slabs, dtrs=dtrs, host=host)
    return _data[key]


def _response(gpu_ctx, oracle_mod, name):
    """The scan, the case's pose grid and the oracle's response on it (cached)."""
    c = CASES[name]
    d = _scan(gpu_ctx, c)
    labels, mats = R.pose_grid(d["Ps"][c["v"]], c.get("dofs", R.DOFS))
    if name not in _oracle:
        f = R.all_pairs_response if c["v"] == 0 else R.moved_pair_response
        _oracle[name] = f(oracle_mod, d["Ps"], d["host"], d["n_u"], d["n_v"], c["v"], mats, dkappa=c["dkappa"])
    return c, d, labels, mats, _oracle[name]


def _metric(gpu_ctx, c, d, mode):
    import epipolarconsistency_amd as E
    return E.MetricRadonIntermediate(gpu_ctx, d["Ps"], d["dtrs"]).setSampling(mode).setEpipolarPlaneStep(c["dkappa"])


def _gpu_sums(m, c, d, mats):
    n = len(d["Ps"])
    means = m.evaluate_pose_deltas([[c["v"]]] * len(mats), [[P] for P in mats])
    return means, means * (n * (n - 1) // 2)


def _errors(labels, S, orc, ref="x"):
    """e per cell (D and D2 of every (dof, h)) of the sums S against orc[ref] (exact sampling), as a flat array in cell order."""
    got, want = R.cells(labels, S), R.cells(labels, orc[ref]["sums"])
    return np.array([abs(g - w) for key in want for g, w in zip(got[key], want[key])])


def _table(labels, orc, S_gpu):
    c0, c64, cg = R.cells(labels, orc[0]["sums"]), R.cells(labels, orc["x"]["sums"]), R.cells(labels, S_gpu)
    for (dof, h), (D, D2) in c64.items():
        print("    %s %-6g D_x %+.4e e0 %.2e e_gpu %.2e | D2_x %+.3e e0 %.2e e_gpu %.2e"
              % (dof, h, D, abs(c0[(dof, h)][0] - D), abs(cg[(dof, h)][0] - D), D2, abs(c0[(dof, h)][1] - D2),
                 abs(cg[(dof, h)][1] - D2)))


def _bar(e_gpu, e0):
    return bool(np.percentile(e_gpu, 50) <= Q50 * np.percentile(e0, 50) and e_gpu.max() <= QMAX * e0.max())


def _attribute(m, c, d, labels, mats, orc, e_gpu):
    """Per-pair attribution of the worst cell: the moved pairs by index list at +h and -h, the worst pairs' change against
    variant 1 with their class (degree, clamp-free, refused) and kappa sample count on each side."""
    keys = list(R.cells(labels, orc["x"]["sums"]).keys())
    dof, h = keys[int(np.argmax(e_gpu)) // 2]
    at = {lab: k for k, lab in enumerate(labels)}
    pq = orc["pairs"]
    n = len(d["Ps"])
    idx = np.ascontiguousarray(np.stack([pq[:, 1], pq[:, 2], pq[:, 1], pq[:, 2]], 1).astype(np.int32))
    side = {}
    for s in (1, -1):
        k = at[(dof, h, s)]
        P = list(d["Ps"])
        P[c["v"]] = mats[k]
        m.setProjectionMatrices(P)
        out = np.empty(len(idx), np.float32)
        m.evaluate(idx, out)
        recs = m.debug_polynomials(0, n * (n - 1) // 2)
        K01 = m.debug_K01(0, n * (n - 1) // 2)[pq[:, 0]]
        side[s] = (out.astype(np.float64), [recs[q] for q in pq[:, 0]],
                   R.kappa_samples(K01, c["dkappa"], d["n_u"], d["n_v"], c["bins"][1]), k)
    m.setProjectionMatrices(d["Ps"])
    kp, km = side[1][3], side[-1][3]
    dg = side[1][0] - side[-1][0]
    d64 = orc["x"]["values"][kp].astype(np.float64) - orc["x"]["values"][km]
    d0 = orc[0]["values"][kp].astype(np.float64) - orc[0]["values"][km]
    worst = np.argsort(-np.abs(dg - d64))[:6]
    print("    attribution %s %g: sum of pair changes %.3e (exact %.3e)" % (dof, h, dg.sum(), d64.sum()))
    for r in worst:
        cls = ["deg %d %s" % (rec[r]["degree"], "free" if rec[r]["clamp_free"] else "clamped") if rec[r]["poly_ok"] else "refused"
               for rec in (side[1][1], side[-1][1])]
        print("      pair (%d, %d): change err %.2e (oracle %.2e), +h %s %d samples, -h %s %d samples"
              % (pq[r, 1], pq[r, 2], abs(dg[r] - d64[r]), abs(d0[r] - d64[r]), cls[0], side[1][2][r], cls[1], side[-1][2][r]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_pose_differences_against_the_oracle(gpu_ctx, oracle_mod, name):
    """Bars 1-3 of the module docstring on one case, every mode of the case."""
    c, d, labels, mats, orc = _response(gpu_ctx, oracle_mod, name)
    n = len(d["Ps"])
    n_pairs = n * (n - 1) // 2
    e0 = _errors(labels, orc[0]["sums"], orc)
    e01 = _errors(labels, orc[0]["sums"], orc, ref=1)
    _bars[name] = e0
    S_moved = abs(orc[0]["sums"][0])
    print("\ncase %s: %d views, bins %s, view %d moved, %d poses, S_moved %.4e; e0 p50 %.2e max %.2e"
          % (name, n, c["bins"], c["v"], len(mats), S_moved, np.percentile(e0, 50), e0.max()))
    fails = []
    # 1. the difference bar, every mode
    for mode in c["modes"]:
        m = _metric(gpu_ctx, c, d, mode)
        means, S = _gpu_sums(m, c, d, mats)
        for k in (1, len(mats) // 2, len(mats) - 1):  # the batch is bit-identical to one pose at a time
            Pk = list(d["Ps"])
            Pk[c["v"]] = mats[k]
            assert m.setProjectionMatrices(Pk).evaluate() == means[k], (mode, labels[k])
        m.setProjectionMatrices(d["Ps"])
        e_gpu = _errors(labels, S, orc)
        e_gpu1 = _errors(labels, S, orc, ref=1)
        ok = _bar(e_gpu, e0)
        print("  %-10s e_gpu p50 %.2e max %.2e | e0 p50 %.2e max %.2e | p50 %.2fx max %.2fx | bar %s"
              " | against variant 1: p50 %.2fx max %.2fx"
              % (mode, np.percentile(e_gpu, 50), e_gpu.max(), np.percentile(e0, 50), e0.max(),
                 np.percentile(e_gpu, 50) / np.percentile(e0, 50), e_gpu.max() / e0.max(), ok,
                 np.percentile(e_gpu1, 50) / np.percentile(e01, 50), e_gpu1.max() / e01.max()))
        _table(labels, orc, S)
        if mode == "reference":  # the CPU path's arithmetic: variant 0 itself, up to the sum's order
            e_ref = _errors(labels, S, orc, ref=0)
            print("    reference vs variant 0: max %.2e (%.1e of S_moved)" % (e_ref.max(), e_ref.max() / S_moved))
            if not e_ref.max() <= 1e-6 * S_moved:
                fails.append(("reference vs variant 0", e_ref.max(), S_moved))
        if not ok:
            _attribute(m, c, d, labels, mats, orc, e_gpu)
            fails.append(("bar 1", mode, np.percentile(e_gpu, 50), e_gpu.max(), np.percentile(e0, 50), e0.max()))
        m.close()
    # 2. non-vacuity: the largest steps are resolved, the smallest reach the noise floor
    c64 = R.cells(labels, orc["x"]["sums"])
    dofs = c.get("dofs", R.DOFS)
    keys = list(c64.keys())
    e0_dof = {dof: max(max(e0[2 * k], e0[2 * k + 1]) for k, key in enumerate(keys) if key[0] == dof) for dof in dofs}
    big = {dof: abs(c64[(dof, R.steps(dof)[0])][0]) / e0_dof[dof] for dof in dofs}
    small = {dof: abs(c64[(dof, R.steps(dof)[-1])][0]) / e0.max() for dof in dofs}
    print("  non-vacuity: |D_x| at the largest step / the DoF's max(e0) %s; at the smallest step / max(e0) %s"
          % (" ".join("%s %.1e" % kv for kv in big.items()), " ".join("%s %.1e" % kv for kv in small.items())))
    if not (min(big.values()) >= 10 and max(big.values()) >= 1e3):
        fails.append(("largest steps not resolved", big))
    if not min(small.values()) <= 10:
        fails.append(("smallest steps above the noise floor", small))
    # 3. same samples: the GPU's K01 at every pose, the loop rule in float32
    m = _metric(gpu_ctx, c, d, "polynomial")
    pq = orc["pairs"][:, 0]
    eq_kmax = total = n_bad = 0
    for k, P in enumerate(mats):
        Pk = list(d["Ps"])
        Pk[c["v"]] = P
        K01 = m.setProjectionMatrices(Pk).debug_K01(0, n_pairs)[pq]
        want = orc[0]["K01s"][k]
        got_n = R.kappa_samples(K01, c["dkappa"], d["n_u"], d["n_v"], c["bins"][1])
        want_n = R.kappa_samples(want, c["dkappa"], d["n_u"], d["n_v"], c["bins"][1])
        bad = np.nonzero(got_n != want_n)[0]
        if len(bad):
            n_bad += len(bad)
            fails.append(("sample count", labels[k], [(int(orc["pairs"][b, 1]), int(orc["pairs"][b, 2]), int(got_n[b]),
                                                       int(want_n[b]), float(K01[b, 15]), float(want[b, 15])) for b in bad[:5]]))
        eq_kmax += int((K01[:, 15] == want[:, 15]).sum())
        total += len(pq)
    print("  same samples: %d pair-poses, %d sample counts differ; kappa_max bit-equal on %d (%.2f %%)"
          % (total, n_bad, eq_kmax, 100.0 * eq_kmax / total))
    m.close()
    assert not fails, fails


# ---- class boundaries ----------------------------------------------------------------------------------------------------
SCAN_MM, SCAN_STEPS, RESOLUTION_MM = 20.0, 200, 1e-7
KINDS = ("degree", "clamp", "refused")


def _classes(m, Ps, v, tz, pq, n_pairs):
    import epipolarconsistency_amd as E
    P = list(Ps)
    P[v] = Ps[v] @ E.geometry.rigid_transform(tz=tz)
    recs = m.setProjectionMatrices(P).debug_polynomials(0, n_pairs)
    return [(recs[q]["poly_ok"], recs[q]["degree"], recs[q]["clamp_free"]) for q in pq]


def _kind(a, b):
    if a[0] != b[0]:
        return "refused"
    if a[1] != b[1]:
        return "degree"
    if a[2] != b[2]:
        return "clamp"
    return None


def _boundaries(m, Ps, v, pq, n_pairs, per_kind=2):
    """tz scan of view v over +-SCAN_MM, then bisection to RESOLUTION_MM: up to per_kind (tz_a, tz_b, moved-pair row, kind) per
    kind where one moved pair changes its degree, its clamp class or the acceptance of its fit."""
    grid = np.linspace(-SCAN_MM, SCAN_MM, SCAN_STEPS + 1)
    cls = [_classes(m, Ps, v, tz, pq, n_pairs) for tz in grid]
    found = {k: [] for k in KINDS}
    for g in range(SCAN_STEPS):
        for r in range(len(pq)):
            kind = _kind(cls[g][r], cls[g + 1][r])
            if kind is None or len(found[kind]) >= per_kind:
                continue
            a, b, ca = grid[g], grid[g + 1], cls[g][r]
            while b - a > RESOLUTION_MM:
                mid = 0.5 * (a + b)
                cm = _classes(m, Ps, v, mid, pq, n_pairs)[r]
                if _kind(ca, cm) is None:
                    a, ca = mid, cm
                else:
                    b = mid
            cb = _classes(m, Ps, v, b, pq, n_pairs)[r]
            found[_kind(ca, cb)].append((a, b, r, ca, cb))
    return found


def test_class_boundaries(gpu_ctx, oracle_mod):
    """Cases B and C, polynomial mode: at poses RESOLUTION_MM apart on either side of a change of one moved pair's class, that
    pair's change (index list) against variant 1's meets the per-pair bar of tests/test_gpu_geometry_parity.py (2x the normative
    oracle's largest relative error over the case's moved pairs), and the change of the mean meets bar 1's max (2 max(e0) of the
    case's grid).  Both against exact sampling, as bar 1.  Each of the three kinds of switch is found."""
    import epipolarconsistency_amd as E
    seen = {k: 0 for k in KINDS}
    for name in ("B", "C"):
        c, d, labels, mats, orc = _response(gpu_ctx, oracle_mod, name)
        e0_max = _bars[name].max() if name in _bars else _errors(labels, orc[0]["sums"], orc).max()
        Ps, v = d["Ps"], c["v"]
        n = len(Ps)
        n_pairs = n * (n - 1) // 2
        pq = orc["pairs"]
        p0, p64 = orc[0]["values"].astype(np.float64), orc["x"]["values"].astype(np.float64)
        scale_all = 1e-3 * np.abs(p64).max()
        noise = (np.abs(p0 - p64) / np.maximum(np.abs(p64), scale_all)).max()
        m = _metric(gpu_ctx, c, d, "polynomial")
        found = _boundaries(m, Ps, v, pq[:, 0], n_pairs)
        print("\ncase %s: per-pair bar 2 x %.2e, mean bar 2 x %.2e" % (name, noise, e0_max))
        for kind in KINDS:
            for a, b, r, ca, cb in found[kind]:
                seen[kind] += 1
                moved = [Ps[v] @ E.geometry.rigid_transform(tz=tz) for tz in (a, b)]
                sub = R.moved_pair_response(oracle_mod, Ps, d["host"], d["n_u"], d["n_v"], v, moved)
                i, j = int(pq[r, 1]), int(pq[r, 2])
                idx = np.array([[i, j, i, j]], np.int32)
                vals = []
                for P in moved:
                    Pk = list(Ps)
                    Pk[v] = P
                    out = np.empty(1, np.float32)
                    m.setProjectionMatrices(Pk).evaluate(idx, out)
                    vals.append(float(out[0]))
                m.setProjectionMatrices(Ps)
                d_gpu = vals[1] - vals[0]
                d64 = float(sub["x"]["values"][1, r]) - float(sub["x"]["values"][0, r])
                d0 = float(sub[0]["values"][1, r]) - float(sub[0]["values"][0, r])
                scale = max(abs(float(sub["x"]["values"][0, r])), scale_all)
                e_pair, e0_pair = abs(d_gpu - d64) / scale, abs(d0 - d64) / scale
                _, S = _gpu_sums(m, c, d, moved)
                D_gpu, D64, D0 = S[1] - S[0], sub["x"]["sums"][1] - sub["x"]["sums"][0], sub[0]["sums"][1] - sub[0]["sums"][0]
                print("  %-7s pair (%d, %d) at tz %+.7f mm: %s -> %s | pair change %+.3e, err %.2e (oracle %.2e) | mean change "
                      "err %.2e (oracle %.2e)" % (kind, i, j, a, ca, cb, d64, e_pair, e0_pair, abs(D_gpu - D64), abs(D0 - D64)))
                assert e_pair <= 2 * noise, (name, kind, i, j, a, e_pair, noise)
                assert abs(D_gpu - D64) <= QMAX * e0_max, (name, kind, i, j, a, D_gpu, D64, e0_max)
        m.close()
    print("boundaries found:", seen)
    for kind in KINDS:
        assert seen[kind] > 0, (kind, seen)


def test_negative_control_coarse_economisation_fails_the_difference_bar(gpu_ctx, oracle_mod):
    """The difference bar catches a worse polynomial path: with the economisation bound raised from 2e-8 bins to T_BAD = 3e-4 it
    fails on at least one of A, B and C; at the default it passes on all three.  Measured (max e_gpu / max e0): 3e-4 fails A (3.2x)
    and B (8.6x), 1e-3 all three (17x, 6.3x, 15x); 1e-4 stays inside the bar (B 1.96x), so the sharper check of the fit at 1e-4 is
    the per-pair bar of tests/test_gpu_geometry_parity.py."""
    verdict = {}
    for name in ("A", "B", "C"):
        c, d, labels, mats, orc = _response(gpu_ctx, oracle_mod, name)
        e0 = _errors(labels, orc[0]["sums"], orc)
        m = _metric(gpu_ctx, c, d, "polynomial")
        for tol in (None, 3e-5, 1e-4, 3e-4, 1e-3):
            if tol is not None:
                m.debugSetPolyTolerance(tol)
            e_gpu = _errors(labels, _gpu_sums(m, c, d, mats)[1], orc)
            verdict[(name, tol)] = _bar(e_gpu, e0)
            print("  %s tol %-7s e_gpu p50 %.2e max %.2e (e0 %.2e %.2e): p50 %.2fx max %.2fx, bar %s"
                  % (name, "default" if tol is None else "%.0e" % tol, np.percentile(e_gpu, 50), e_gpu.max(),
                     np.percentile(e0, 50), e0.max(), np.percentile(e_gpu, 50) / np.percentile(e0, 50), e_gpu.max() / e0.max(),
                     verdict[(name, tol)]))
        m.close()
    assert all(verdict[(name, None)] for name in ("A", "B", "C")), verdict
    assert not all(verdict[(name, T_BAD)] for name in ("A", "B", "C")), verdict
