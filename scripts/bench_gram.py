#!/usr/bin/env python3
"""Milliseconds per ecc_metric_evaluate_gram against the evaluation it is built from (GPU box):
    python scripts/bench_gram.py [--lib PATH] [--legs abc] [--views 400] [--bins 768] [--channels 2,3,4]
(a) evaluate_gram(K) without the pair entries on a metric of K * views Radon intermediates (csrc/ecc_gram.hip, csrc/gram_kernel.hip);
(b) evaluate() -- no cost image, library defaults: the benchmark's step without its setProjectionMatrices -- on a single-channel
    metric.  It exists on older revisions too: --lib PATH loads another build of the library (one made from the parent revision),
    where only --legs b runs.  (b) on both revisions shows that the existing path was left alone; THE GATE for (a) is
    K (K + 1) / 2 x (b), the all-pairs evaluations the existing calls need for the same matrix, and (a) / (K x (b)) says what the
    shared position arithmetic buys;
(c) once, for the record: the loop the call replaces -- compute_into of all images + refreshRadonIntermediates + evaluate().
Every shape is warmed up; the figure is the median of --windows windows of at least --min-seconds each, with the spread
(min .. max) beside it.  Run the builds alternately inside one job (parent, this, parent, this).  One JSON line per leg.
--once K[,K...]: two calls of leg (a) per K and nothing else (for a kernel trace or a counter pass; K = 1 is pairs_kernel)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default="")
ap.add_argument("--legs", default="abc")
ap.add_argument("--views", type=int, default=400)
ap.add_argument("--bins", type=int, default=768)
ap.add_argument("--channels", default="2,3,4")
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--min-seconds", type=float, default=0.3)
ap.add_argument("--tag", default="")
ap.add_argument("--once", default="")
args = ap.parse_args()
if args.lib:
    os.environ["ECC_HIP_LIB"] = os.path.abspath(args.lib)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epipolarconsistency_amd import _lib  # noqa: E402
with open(_lib.LIB_PATH, "rb") as f:  # (looked up in the file: the package loads the library itself, after torch's runtime)
    HAVE_GRAM = b"ecc_metric_evaluate_gram" in f.read()
if not HAVE_GRAM:  # an older build: leg (b) only
    _lib.SIGNATURES.pop("ecc_metric_evaluate_gram", None)
import epipolarconsistency_amd as E  # noqa: E402
from epipolarconsistency_amd import synthetic  # noqa: E402

ctx = E.Context(0)
rng = np.random.default_rng(7)
S, n = 1024, args.views
pool = [E.RadonIntermediate.from_host(ctx, rng.standard_normal((args.bins, args.bins)).astype(np.float32), S, S) for _ in range(11)]
Ps = synthetic.short_scan(n, S, S, 0.308)
rec = dict(views=n, bins=args.bins, lib=args.tag or (args.lib or "this"))


def windows(fn):
    fn()  # warm-up of this shape
    fn()
    t0 = time.perf_counter()
    fn()
    reps = max(1, int(np.ceil(args.min_seconds / max(time.perf_counter() - t0, 1e-6))))
    ms = []
    for _ in range(args.windows):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        ms.append(1e3 * (time.perf_counter() - t0) / reps)
    return float(np.median(ms)), float(min(ms)), float(max(ms)), reps


def channel_metric(K):  # K * n intermediates, channel-major, neighbouring channels and views on different arrays
    return E.MetricRadonIntermediate(ctx, Ps, [pool[(3 * c + v) % len(pool)] for c in range(K) for v in range(n)])


if args.once:
    for K in [int(x) for x in args.once.split(",")]:
        m = channel_metric(K)
        m.evaluate_gram(K)
        m.evaluate_gram(K)
        m.close()
    sys.exit(0)

single = E.MetricRadonIntermediate(ctx, Ps, [pool[v % len(pool)] for v in range(n)])
if "b" in args.legs:
    med, lo, hi, reps = windows(single.evaluate)
    b_ms = med
    print(json.dumps(dict(rec, leg="b_evaluate", ms_per_call=med, min=lo, max=hi, calls_per_window=reps)), flush=True)
if "a" in args.legs and HAVE_GRAM:
    for K in [int(x) for x in args.channels.split(",")]:
        m = channel_metric(K)
        G = m.evaluate_gram(K)
        assert G[0, 0] == single.evaluate() and np.array_equal(G, G.T)   # channel 0 is the single-channel metric's scan
        med, lo, hi, reps = windows(lambda: m.evaluate_gram(K))
        out = dict(rec, leg="a_gram", channels=K, ms_per_call=med, min=lo, max=hi, calls_per_window=reps)
        if "b" in args.legs:
            out.update(over_b=med / b_ms, gate=K * (K + 1) / 2, over_K_b=med / (K * b_ms))
        print(json.dumps(out), flush=True)
        m.close()
if "c" in args.legs:
    import torch
    dev = torch.device("cuda", ctx.device)
    imgs = torch.rand((n, S, S), dtype=torch.float32, device=dev)
    slabs = torch.zeros((n, E.slab_floats(args.bins, args.bins)), dtype=torch.float32, device=dev)
    dtrs = E.RadonIntermediate.compute_into(ctx, imgs, slabs, args.bins, args.bins)
    ctx.synchronize()
    loop_metric = E.MetricRadonIntermediate(ctx, Ps, dtrs)

    def loop():
        E.RadonIntermediate.compute_into(ctx, imgs, slabs, args.bins, args.bins)
        loop_metric.refreshRadonIntermediates()
        return loop_metric.evaluate()
    loop()
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        loop()
        ms.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps(dict(rec, leg="c_recompute_refresh_evaluate", ms_per_call=float(np.median(ms)), min=min(ms), max=max(ms),
                          calls_per_window=1)), flush=True)
    loop_metric.close()
single.close()
