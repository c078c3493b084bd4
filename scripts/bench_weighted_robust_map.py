#!/usr/bin/env python3
"""The time of ecc_metric_evaluate_weighted_robust_map beside the calls it extends (GPU box):
    python scripts/bench_weighted_robust_map.py [--legs wrmol] [--views 400] [--bins 768] [--loss 0] [--root DIR] [--commit REVISION]
--views views (400) of a 1024^2 detector, --bins^2 Radon bins (768), POLYNOMIAL sampling, wall clock per call, on a 2 n metric
whose weights are uniform in [0, 1] with a tenth of the bins at 0, and on the n-metric over the same data:
(w) evaluate_weighted_robust(loss, delta), delta = weighted_robust_scale(its rows at delta = inf, 0.5);
(r) evaluate_robust_map(loss, delta) on the n-metric, every view mapped, planes left on the device;
(m) the weighted map with every view mapped, planes left on the device (hits = rejected = NULL) -- and once with the planes copied;
(o) the weighted map with ONE view mapped (view n / 2), planes copied;
(l) the weighted map's index-list form over the n - 1 pairs of that view, that view mapped, planes copied.
--root: the checkout whose package and library are timed (default: this one), so that the same script times an earlier commit in
the same job; a library without the weighted map runs (w) and (r) only.  Before it is timed, (m) is checked against (w) bit for bit.
Every shape is warmed up twice; a figure is the median of --windows windows of at least --min-seconds each, with min and max beside
it.  One JSON line per leg."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="wrmol")
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


def weight_field():
    w = rng.uniform(0.0, 1.0, (B, B)).astype(np.float32)
    w[rng.uniform(0.0, 1.0, (B, B)) < 0.1] = 0.0
    return w


wpool = [E.RadonIntermediate.from_host(ctx, weight_field(), S, S, filter=E.FILTER_NONE) for _ in range(7)]
Ps = synthetic.short_scan(n, S, S, 0.308)
data = [pool[v % len(pool)] for v in range(n)]
m = E.MetricRadonIntermediate(ctx, Ps, data + [wpool[v % len(wpool)] for v in range(n)]).setSampling("polynomial")
m1 = E.MetricRadonIntermediate(ctx, Ps, data).setSampling("polynomial")
has_map = hasattr(m, "evaluate_weighted_robust_map")
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


L = _lib.lib()
delta = float(np.float32(E.weighted_robust_scale(m.evaluate_weighted_robust(LOSS, INF, want_pairs=True)[3], 0.5)))
if "w" in args.legs:
    value, cover, mass = m.evaluate_weighted_robust(LOSS, delta)
    report("w_evaluate_weighted_robust", windows(lambda: m.evaluate_weighted_robust(LOSS, delta)), value=value, coverage=cover, inlier_mass=mass,
           delta=delta)
if "r" in args.legs and hasattr(m1, "evaluate_robust_map"):
    value, mass = C.c_double(0.0), C.c_double(0.0)
    w = windows(lambda: check(L.ecc_metric_evaluate_robust_map(m1._h, LOSS, delta, None, 0, None, None, C.byref(value), C.byref(mass), None)))
    report("r_robust_map_all_views_n_metric", w, value=value.value, inlier_mass=mass.value, delta=delta)
if has_map:
    value, cover, mass = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
    padded = E.slab_floats(B, B)

    def map_call(views, planes, idx=None):
        v = None if views is None else C.c_void_p(views.ctypes.data)
        k = 0 if views is None else len(views)
        h, r = (None, None) if planes is None else (C.c_void_p(planes[0].ctypes.data), C.c_void_p(planes[1].ctypes.data))
        if idx is None:
            check(L.ecc_metric_evaluate_weighted_robust_map(m._h, LOSS, delta, v, k, h, r, C.byref(value), C.byref(cover), C.byref(mass), None))
        else:
            check(L.ecc_metric_evaluate_weighted_robust_map_pairs(m._h, C.c_void_p(idx.ctypes.data), len(idx), LOSS, delta, v, k, h, r,
                                                                  C.byref(value), C.byref(cover), C.byref(mass), None))

    one = np.array([n // 2], np.int32)
    planes1 = (np.zeros((1, B, B), np.float32), np.zeros((1, B, B), np.float32))
    if "m" in args.legs:
        want = m.evaluate_weighted_robust(LOSS, delta)
        map_call(None, None)
        got = (value.value, cover.value, mass.value)
        assert np.asarray(want, np.float64).tobytes() == np.asarray(got, np.float64).tobytes(), "the map call is not evaluate_weighted_robust"
        w = windows(lambda: map_call(None, None))
        planes = (np.zeros((n, B, B), np.float32), np.zeros((n, B, B), np.float32))
        t0 = time.perf_counter()
        map_call(None, planes)
        with_copies = 1e3 * (time.perf_counter() - t0)
        hits_mass = float(planes[0].astype(np.float64).sum())
        report("m_weighted_map_all_views", w, ms_with_planes_copied=with_copies, plane_bytes_device=int(n * (16 * padded + 8 * B * B)),
               hits_mass=hits_mass, rej_over_hits=float(planes[1].astype(np.float64).sum()) / hits_mass, coverage=cover.value)
        del planes
    if "o" in args.legs:
        w = windows(lambda: map_call(one, planes1))
        report("o_weighted_map_one_view", w, plane_bytes_device=int(16 * padded + 8 * B * B), hits_mass=float(planes1[0].astype(np.float64).sum()))
    if "l" in args.legs:
        v = n // 2
        idx = np.array([[min(u, v), max(u, v)] * 2 for u in range(n) if u != v], np.int32)
        w = windows(lambda: map_call(one, planes1, idx))
        report("l_weighted_map_list_one_view", w, listed_pairs=len(idx), hits_mass=float(planes1[0].astype(np.float64).sum()))
m.close()
m1.close()
