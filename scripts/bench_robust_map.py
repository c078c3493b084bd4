#!/usr/bin/env python3
"""The time of ecc_metric_evaluate_robust_map beside the calls it extends (GPU box):
    python scripts/bench_robust_map.py [--legs ermol] [--views 400] [--bins 768] [--loss 0] [--root DIR] [--commit REVISION]
--views views (400) of a 1024^2 detector, --bins^2 Radon bins (768), POLYNOMIAL sampling, wall clock per call:
(e) evaluate();
(r) evaluate_robust(loss, delta), delta = robust_scale(its rows at delta = inf, 0.5);
(m) the map with every view mapped, planes left on the device (hits = rejected = NULL) -- and once with the planes copied to the host;
(o) the map with ONE view mapped (view n / 2), planes copied;
(l) the map's index-list form over the n - 1 pairs of that view, that view mapped, planes copied.
--root: the checkout whose package and library are timed (default: this one), so that the same script times an earlier commit in
the same job; a library without the map call runs (e) and (r) only.  Before it is timed, (m) is checked against (r) bit for bit.
Every shape is warmed up twice; a figure is the median of --windows windows of at least --min-seconds each, with min and max beside
it.  One JSON line per leg.  The map legs also report the plane memory on the device and the bytes their atomics add: 32 bytes of
HITS per footprint (four 8-byte cells), sum HITS footprints in all, and at most as many again for REJ (a sample with w == 1 skips
them)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="ermol")
ap.add_argument("--views", type=int, default=400)
ap.add_argument("--bins", type=int, default=768)
ap.add_argument("--loss", type=int, default=0)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--min-seconds", type=float, default=0.5)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--commit", default="")
args = ap.parse_args()

sys.path.insert(0, os.path.abspath(args.root))
import epipolarconsistency_amd as E  # noqa: E402
from epipolarconsistency_amd import _lib, synthetic  # noqa: E402
from epipolarconsistency_amd._lib import check  # noqa: E402

ctx = E.Context(0)
rng = np.random.default_rng(7)
S, B, n, LOSS, INF = 1024, args.bins, args.views, args.loss, float("inf")
pool = [E.RadonIntermediate.from_host(ctx, rng.standard_normal((B, B)).astype(np.float32), S, S) for _ in range(11)]
Ps = synthetic.short_scan(n, S, S, 0.308)
m = E.MetricRadonIntermediate(ctx, Ps, [pool[v % len(pool)] for v in range(n)]).setSampling("polynomial")
has_map = hasattr(m, "evaluate_robust_map")
rec = dict(views=n, pairs=n * (n - 1) // 2, bins=B, loss=LOSS, commit=args.commit, root=os.path.abspath(args.root))


def windows(fn):
    """median, min, max of the windows' ms per call; calls per window"""
    fn()  # warm-up of this shape
    fn()
    t0 = time.perf_counter()
    fn()
    reps = max(1, int(np.ceil(args.min_seconds / max(time.perf_counter() - t0, 1e-6))))
    ms = []
    for _ in range(args.windows):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()    # (every call here returns with its results on the host: the clock stops behind the device)
        ms.append(1e3 * (time.perf_counter() - t0) / reps)
    return dict(ms_per_call=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)), calls_per_window=reps)


def report(leg, w, **more):
    print(json.dumps(dict(rec, leg=leg, **w, **more)), flush=True)


delta = float(np.float32(E.robust_scale(m.evaluate_robust(LOSS, INF, want_pairs=True)[2], 0.5)))
if "e" in args.legs:
    report("e_evaluate", windows(m.evaluate), value=m.evaluate())
if "r" in args.legs:
    value, mass = m.evaluate_robust(LOSS, delta)
    report("r_evaluate_robust", windows(lambda: m.evaluate_robust(LOSS, delta)), value=value, inlier_mass=mass, delta=delta)
if has_map:
    L = _lib.lib()
    value, mass = C.c_double(0.0), C.c_double(0.0)
    padded = E.slab_floats(B, B)

    def map_call(views, planes, idx=None):
        v = None if views is None else C.c_void_p(views.ctypes.data)
        k = 0 if views is None else len(views)
        h, r = (None, None) if planes is None else (C.c_void_p(planes[0].ctypes.data), C.c_void_p(planes[1].ctypes.data))
        if idx is None:
            check(L.ecc_metric_evaluate_robust_map(m._h, LOSS, delta, v, k, h, r, C.byref(value), C.byref(mass), None))
        else:
            check(L.ecc_metric_evaluate_robust_map_pairs(m._h, C.c_void_p(idx.ctypes.data), len(idx), LOSS, delta, v, k, h, r, C.byref(value),
                                                           C.byref(mass), None))

    one = np.array([n // 2], np.int32)
    planes1 = (np.zeros((1, B, B), np.float32), np.zeros((1, B, B), np.float32))
    if "m" in args.legs:
        want = m.evaluate_robust(LOSS, delta)
        map_call(None, None)
        assert np.float64(want[0]).tobytes() == np.float64(value.value).tobytes() and want[1] == mass.value, "the map call is not evaluate_robust"
        w = windows(lambda: map_call(None, None))
        planes = (np.zeros((n, B, B), np.float32), np.zeros((n, B, B), np.float32))
        t0 = time.perf_counter()
        map_call(None, planes)
        with_copies = 1e3 * (time.perf_counter() - t0)
        footprints = float(planes[0].astype(np.float64).sum())
        report("m_map_all_views", w, ms_with_planes_copied=with_copies, plane_bytes_device=int(n * (16 * padded + 8 * B * B)),
               hits_footprints=footprints, hits_atomic_bytes=32.0 * footprints, rej_atomic_bytes_at_most=32.0 * footprints,
               rej_over_hits=float(planes[1].astype(np.float64).sum()) / footprints)
        del planes
    if "o" in args.legs:
        w = windows(lambda: map_call(one, planes1))
        footprints = float(planes1[0].astype(np.float64).sum())
        report("o_map_one_view", w, plane_bytes_device=int(16 * padded + 8 * B * B), hits_footprints=footprints,
               hits_atomic_bytes=32.0 * footprints)
    if "l" in args.legs:
        v = n // 2
        idx = np.array([[min(u, v), max(u, v)] * 2 for u in range(n) if u != v], np.int32)
        w = windows(lambda: map_call(one, planes1, idx))
        report("l_map_list_one_view", w, listed_pairs=len(idx), hits_footprints=float(planes1[0].astype(np.float64).sum()))
m.close()
