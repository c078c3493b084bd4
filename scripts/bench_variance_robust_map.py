#!/usr/bin/env python3
"""The time of ecc_metric_evaluate_variance_robust_map beside the calls it extends (GPU box):
    python scripts/bench_variance_robust_map.py [--lib PATH] [--legs vwmol] [--views 400] [--bins 768] [--loss 0] [--tag NAME]
--views views (400) of a 1024^2 detector, --bins^2 Radon bins (768), POLYNOMIAL sampling, Huber's loss, wall clock per call, on a 2 n
metric: the data, then one positive field per view (0.25 * 16^U(0, 1) per bin), which evaluate_weighted_robust_map reads as line
weights and evaluate_variance_robust_map as variances -- the same 8 gathers per kappa step and the same deposits either way.
delta = 0.5 x the form's own scale of its delta = inf rows.
(v) evaluate_variance_robust(loss, delta, floor), the call the map extends;
(w) evaluate_weighted_robust_map on the same metric: every view mapped with the planes left on the device (hits = rejected = NULL),
    one view mapped (view n / 2) with its planes copied, and the index-list form over the n - 1 pairs of that view;
(m) the variance map with every view mapped, planes left on the device -- and once with the planes copied;
(o) the variance map with ONE view mapped (view n / 2), planes copied;
(l) the variance map's index-list form over the n - 1 pairs of that view, that view mapped, planes copied.
(v) and (w) exist on the parent revision too: --lib PATH loads another build of the library, where they alone run.  Run the builds
alternately inside one job (parent, this, parent, this; --tag parent_run1, this_run1, ...).  Before it is timed, (m) is checked
against (v) bit for bit.  There is no time gate: the map is a diagnostic and its atomics set its time.
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
ap.add_argument("--lib", default="")
ap.add_argument("--legs", default="vwmol")
ap.add_argument("--views", type=int, default=400)
ap.add_argument("--bins", type=int, default=768)
ap.add_argument("--loss", type=int, default=0)
ap.add_argument("--floor", type=float, default=1.5)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--min-seconds", type=float, default=0.5)
ap.add_argument("--tag", default="")
args = ap.parse_args()

if args.lib:
    os.environ["ECC_HIP_LIB"] = os.path.abspath(args.lib)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epipolarconsistency_amd import _lib  # noqa: E402
with open(_lib.LIB_PATH, "rb") as f:  # (looked up in the file: the package loads the library itself, after torch's runtime)
    HAVE_MAP = b"ecc_metric_evaluate_variance_robust_map" in f.read()
if not HAVE_MAP:  # the parent's build: legs (v) and (w) only
    for name in [k for k in _lib.SIGNATURES if "variance_robust_map" in k]:
        _lib.SIGNATURES.pop(name, None)
import epipolarconsistency_amd as E  # noqa: E402
from epipolarconsistency_amd import synthetic  # noqa: E402
from epipolarconsistency_amd._lib import check  # noqa: E402

ctx = E.Context(0)
rng = np.random.default_rng(7)
S, B, n, LOSS, FLOOR, INF = 1024, args.bins, args.views, args.loss, args.floor, float("inf")
pool = [E.RadonIntermediate.from_host(ctx, rng.standard_normal((B, B)).astype(np.float32), S, S) for _ in range(11)]
vpool = [E.RadonIntermediate.from_host(ctx, (0.25 * 16.0 ** rng.random((B, B))).astype(np.float32), S, S, filter=E.FILTER_NONE) for _ in range(7)]
Ps = synthetic.short_scan(n, S, S, 0.308)
m = E.MetricRadonIntermediate(ctx, Ps, [pool[v % len(pool)] for v in range(n)] + [vpool[(v + 3) % len(vpool)] for v in range(n)]).setSampling("polynomial")
rec = dict(views=n, pairs=n * (n - 1) // 2, bins=B, loss=LOSS, floor=FLOOR, lib=args.tag or (args.lib or "this"))


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
one = np.array([n // 2], np.int32)
planes1 = (np.zeros((1, B, B), np.float32), np.zeros((1, B, B), np.float32))
idx = np.array([[min(u, n // 2), max(u, n // 2)] * 2 for u in range(n) if u != n // 2], np.int32)
value, second, mass = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
padded = E.slab_floats(B, B)


def map_call(fn, lead, extra, views, planes):
    v = None if views is None else C.c_void_p(views.ctypes.data)
    k = 0 if views is None else len(views)
    h, r = (None, None) if planes is None else (C.c_void_p(planes[0].ctypes.data), C.c_void_p(planes[1].ctypes.data))
    check(fn(m._h, *lead, *extra, v, k, h, r, C.byref(value), C.byref(second), C.byref(mass), None))


delta = float(np.float32(E.variance_robust_scale(m.evaluate_variance_robust(LOSS, INF, FLOOR, want_pairs=True)[3], 0.5)))
if "v" in args.legs:
    got = m.evaluate_variance_robust(LOSS, delta, FLOOR)
    report("v_evaluate_variance_robust", windows(lambda: m.evaluate_variance_robust(LOSS, delta, FLOOR)), value=got[0], mean_weight=got[1],
           inlier_mass=got[2], delta=delta)
if "w" in args.legs:
    raw_delta = float(np.float32(E.weighted_robust_scale(m.evaluate_weighted_robust(LOSS, INF, want_pairs=True)[3], 0.5)))
    f, g, lead = L.ecc_metric_evaluate_weighted_robust_map, L.ecc_metric_evaluate_weighted_robust_map_pairs, (C.c_void_p(idx.ctypes.data), len(idx))
    report("w_weighted_map_all_views", windows(lambda: map_call(f, (), (LOSS, raw_delta), None, None)), delta=raw_delta)
    report("w_weighted_map_one_view", windows(lambda: map_call(f, (), (LOSS, raw_delta), one, planes1)), delta=raw_delta)
    report("w_weighted_map_list_one_view", windows(lambda: map_call(g, lead, (LOSS, raw_delta), one, planes1)), listed_pairs=len(idx), delta=raw_delta)
if HAVE_MAP:
    f, g, lead = L.ecc_metric_evaluate_variance_robust_map, L.ecc_metric_evaluate_variance_robust_map_pairs, (C.c_void_p(idx.ctypes.data), len(idx))
    extra = (LOSS, delta, FLOOR)
    if "m" in args.legs:
        want = m.evaluate_variance_robust(LOSS, delta, FLOOR)
        map_call(f, (), extra, None, None)
        got = (value.value, second.value, mass.value)
        assert np.asarray(want, np.float64).tobytes() == np.asarray(got, np.float64).tobytes(), "the map call is not evaluate_variance_robust"
        w = windows(lambda: map_call(f, (), extra, None, None))
        planes = (np.zeros((n, B, B), np.float32), np.zeros((n, B, B), np.float32))
        t0 = time.perf_counter()
        map_call(f, (), extra, None, planes)
        with_copies = 1e3 * (time.perf_counter() - t0)
        hits_mass = float(planes[0].astype(np.float64).sum())
        report("m_variance_map_all_views", w, ms_with_planes_copied=with_copies, plane_bytes_device=int(n * (16 * padded + 8 * B * B)),
               hits_mass=hits_mass, rej_over_hits=float(planes[1].astype(np.float64).sum()) / hits_mass, delta=delta)
        del planes
    if "o" in args.legs:
        w = windows(lambda: map_call(f, (), extra, one, planes1))
        report("o_variance_map_one_view", w, plane_bytes_device=int(16 * padded + 8 * B * B), hits_mass=float(planes1[0].astype(np.float64).sum()))
    if "l" in args.legs:
        w = windows(lambda: map_call(g, lead, extra, one, planes1))
        report("l_variance_map_list_one_view", w, listed_pairs=len(idx), hits_mass=float(planes1[0].astype(np.float64).sum()))
m.close()
