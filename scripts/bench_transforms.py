#!/usr/bin/env python3
"""Transforms per second of the batched registration (GPU box):
    python scripts/bench_transforms.py [--legs ab] [--sizes 20,50,100,200] [--K 600,12] [--bins 1024] [--modes auto]
(a) ecc_metric_evaluate_transforms (csrc/ecc_transforms.hip), K transforms per call;
(b) the sequential loop a caller without it runs: setProjectionMatrices(composed matrices) + evaluate(index list) per
    transform -- only calls that exist without the batch, so the same script measures the baseline on an older revision
    (--legs b; the composed matrices are made by numpy there and are not timed in either leg).
An "evaluation" here is ONE transform = n_source * n_target sampled pairs (not an all-pairs evaluation).  Every timed window
ends in a synchronous result; each shape is warmed up first; the figure is the median of --windows windows of at least
--min-seconds each, with the spread (min .. max) beside it.  One JSON line per (size, K, mode, leg)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import epipolarconsistency_amd as E  # noqa: E402
from epipolarconsistency_amd import geometry, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="ab")
ap.add_argument("--sizes", default="20,50,100,200")
ap.add_argument("--K", default="600,12")
ap.add_argument("--bins", type=int, default=1024)
ap.add_argument("--modes", default="auto")
ap.add_argument("--radius", type=float, default=0.0)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--min-seconds", type=float, default=0.3)
ap.add_argument("--once", action="store_true", help="one batched call per shape and nothing else (for a kernel trace)")
args = ap.parse_args()

ctx = E.Context(0)
rng = np.random.default_rng(7)
S = 1024
pool = [E.RadonIntermediate.from_host(ctx, rng.standard_normal((args.bins, args.bins)).astype(np.float32), S, S) for _ in range(8)]


def compose(P, T):
    return geometry.compose_transform(P, T) if hasattr(geometry, "compose_transform") else P @ T


def windows(fn, per_call):
    fn()  # warm-up of this shape
    fn()
    t0 = time.perf_counter()
    fn()
    reps = max(1, int(np.ceil(args.min_seconds / max(time.perf_counter() - t0, 1e-6))))
    rates = []
    for _ in range(args.windows):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        rates.append(per_call * reps / (time.perf_counter() - t0))
    return float(np.median(rates)), float(min(rates)), float(max(rates)), reps


for size in [int(x) for x in args.sizes.split(",")]:
    ns = nt = size
    n = ns + nt
    Ps = synthetic.short_scan(n, S, S, 0.308)
    dtrs = [pool[v % len(pool)] for v in range(n)]
    j, i = np.divmod(np.arange(ns * nt), ns)
    idx = np.ascontiguousarray(np.stack([i, ns + j, i, ns + j], axis=1).astype(np.int32))
    out = np.zeros(ns * nt, np.float32)
    for mode in args.modes.split(","):
        m = E.MetricRadonIntermediate(ctx, Ps, dtrs).setSampling(mode)
        m.setObjectRadius(args.radius)
        for K in [int(x) for x in args.K.split(",")]:
            Ts = np.stack([geometry.rigid_transform(tx=0.05 * k, ty=-0.02 * (k % 7), tz=0.01 * (k % 5), rz=1e-4 * k, rx=5e-5 * (k % 3))
                           for k in range(K)])
            if args.once:
                m.evaluate_transforms(ns, Ts)
                m.evaluate_transforms(ns, Ts)
                continue
            rec = dict(n_source=ns, n_target=nt, pairs_per_transform=ns * nt, K=K, mode=mode, bins=args.bins, radius=args.radius)
            if "a" in args.legs:
                med, lo, hi, reps = windows(lambda: m.evaluate_transforms(ns, Ts), K)
                assert m.last_batched_transforms() == K
                print(json.dumps(dict(rec, leg="a_batched", transforms_per_s=med, min=lo, max=hi, calls_per_window=reps,
                                      ns_per_pair=1e9 / (med * ns * nt))), flush=True)
            if "b" in args.legs:
                composed = [E.pack_projection_matrices([compose(P, T) for P in Ps[:ns]] + list(Ps[ns:])) for T in Ts]

                def loop():
                    for Pk in composed:
                        m.setProjectionMatrices(Pk).evaluate(idx, out)
                med, lo, hi, reps = windows(loop, K)
                m.setProjectionMatrices(Ps)
                print(json.dumps(dict(rec, leg="b_sequential", transforms_per_s=med, min=lo, max=hi, calls_per_window=reps,
                                      ns_per_pair=1e9 / (med * ns * nt))), flush=True)
        m.close()
