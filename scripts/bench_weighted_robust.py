#!/usr/bin/env python3
"""The time of ecc_metric_evaluate_weighted_robust beside the three calls it is made of (GPU box):
    python scripts/bench_weighted_robust.py [--legs ewrc] [--views 400] [--bins 768] [--loss 0] [--root DIR] [--commit REVISION]
--views views (400) of a 1024^2 detector, --bins^2 Radon bins (768), POLYNOMIAL sampling, wall clock per call:
(e) evaluate() on the metric of n intermediates;
(w) evaluate_weighted() on the metric of 2 n intermediates: the same data, then line weights in 8 x 8 blocks that are 0, 1 or U(0, 1);
(r) evaluate_robust(loss, delta) on the n-metric, delta = robust_scale(its rows at delta = inf, 0.5);
(c) evaluate_weighted_robust(loss, delta) on the 2 n metric, delta = weighted_robust_scale(its rows at delta = inf, 0.5).
What (c) is measured against: t(w) + (t(r) - t(e)) -- the weighted kernel's eight gathers per kappa step plus what the loss
arithmetic adds to the plain kernel.  --root: the checkout whose package and library are timed (default: this one), so that the same
script times an earlier commit in the same job; a library without the combined call skips (c).  Before it is timed, (c) is checked
against (w) at delta = inf, bit for bit.  Every shape is warmed up twice; a figure is the median of --windows windows of at least
--min-seconds each, with min and max beside it.  One JSON line per leg."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="ewrc")
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
from epipolarconsistency_amd import synthetic  # noqa: E402

ctx = E.Context(0)
rng = np.random.default_rng(7)
S, B, n, LOSS, INF = 1024, args.bins, args.views, args.loss, float("inf")
pool = [E.RadonIntermediate.from_host(ctx, rng.standard_normal((B, B)).astype(np.float32), S, S) for _ in range(11)]


def weight_field():
    """8 x 8 blocks, each exactly 0.0, exactly 1.0 or U(0, 1) per bin (the fields of tests/weighted_terms.py)."""
    side = -(-B // 8)
    kind = np.repeat(np.repeat(rng.integers(0, 3, (8, 8)), side, axis=0), side, axis=1)[:B, :B]
    return np.where(kind == 2, rng.random((B, B)), kind).astype(np.float32)


wpool = [E.RadonIntermediate.from_host(ctx, weight_field(), S, S, filter=E.FILTER_NONE) for _ in range(11)]
Ps = synthetic.short_scan(n, S, S, 0.308)
data = [pool[v % len(pool)] for v in range(n)]
weights = [wpool[v % len(wpool)] for v in range(n)]
m1 = E.MetricRadonIntermediate(ctx, Ps, data).setSampling("polynomial")
m2 = E.MetricRadonIntermediate(ctx, Ps, data + weights).setSampling("polynomial")
combined = hasattr(m2, "evaluate_weighted_robust")
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


def same(x, y):
    return np.float64(x).tobytes() == np.float64(y).tobytes()


if "e" in args.legs:
    report("e_evaluate", windows(m1.evaluate), value=m1.evaluate())
if "w" in args.legs:
    value, coverage = m2.evaluate_weighted()
    report("w_evaluate_weighted", windows(m2.evaluate_weighted), value=value, coverage=coverage)
if "r" in args.legs:
    delta = float(np.float32(E.robust_scale(m1.evaluate_robust(LOSS, INF, want_pairs=True)[2], 0.5)))
    value, mass = m1.evaluate_robust(LOSS, delta)
    report("r_evaluate_robust", windows(lambda: m1.evaluate_robust(LOSS, delta)), value=value, inlier_mass=mass, delta=delta)
if "c" in args.legs and combined:
    at_inf = m2.evaluate_weighted_robust(LOSS, INF, want_pairs=True)
    value, coverage = m2.evaluate_weighted()
    assert same(at_inf[0], value) and same(at_inf[1], coverage) and at_inf[2] == 1.0, "delta = inf is not evaluate_weighted"
    delta = float(np.float32(E.weighted_robust_scale(at_inf[3], 0.5)))
    value, coverage, mass = m2.evaluate_weighted_robust(LOSS, delta)
    assert 0.0 < mass < 1.0
    report("c_evaluate_weighted_robust", windows(lambda: m2.evaluate_weighted_robust(LOSS, delta)), value=value, coverage=coverage,
           inlier_mass=mass, delta=delta)
m1.close()
m2.close()
