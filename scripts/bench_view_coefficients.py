#!/usr/bin/env python3
"""Milliseconds per ecc_metric_evaluate_view_coefficients against the calls it is expected to cost as much as (GPU box):
    python scripts/bench_view_coefficients.py [--lib PATH] [--legs ab] [--views 400] [--bins 768] [--channels 1,2,3,4]
(a) evaluate_view_coefficients(a) -- value and gradient, no pair terms -- on a metric of K * views Radon intermediates
    (csrc/ecc_view_coeff.hip, csrc/view_coeff_kernel.hip), a ~ U(0.5, 1.5);
(b) what it is gated against: evaluate_gram(K) on the same metric for K = 2 .. 4 -- the same 4 K gathers per kappa step -- and
    evaluate() (no cost image, library defaults) on a single-channel metric for K = 1.  (b) exists on the parent revision too:
    --lib PATH loads another build of the library, where only leg (b) runs.  THE GATE: (a) <= 1.15 x (b) of the parent's build;
    (b) on both builds shows that the existing paths were left alone.
Every shape is warmed up; the figure is the median of --windows windows of at least --min-seconds each, with the spread
(min .. max) beside it.  Run the builds alternately inside one job (parent, this, parent, this).  One JSON line per leg and K.
--once K[,K...]: two calls of leg (a) per K and nothing else (for a kernel trace or a counter pass)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default="")
ap.add_argument("--legs", default="ab")
ap.add_argument("--views", type=int, default=400)
ap.add_argument("--bins", type=int, default=768)
ap.add_argument("--channels", default="1,2,3,4")
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
    HAVE_CALL = b"ecc_metric_evaluate_view_coefficients" in f.read()
if not HAVE_CALL:  # the parent's build: leg (b) only
    _lib.SIGNATURES.pop("ecc_metric_evaluate_view_coefficients", None)
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


def channel_metric(K):  # K * n intermediates, channel-major, neighbouring channels and views on different arrays (scripts/bench_gram.py)
    return E.MetricRadonIntermediate(ctx, Ps, [pool[(3 * c + v) % len(pool)] for c in range(K) for v in range(n)]).setSampling("polynomial")


def coefficients(K):
    return np.random.default_rng(11).uniform(0.5, 1.5, (K, n)).astype(np.float32)


if args.once:
    for K in [int(x) for x in args.once.split(",")]:
        m = channel_metric(K)
        m.evaluate_view_coefficients(coefficients(K))
        m.evaluate_view_coefficients(coefficients(K))
        m.close()
    sys.exit(0)

for K in [int(x) for x in args.channels.split(",")]:
    m = channel_metric(K)
    b_ms = None
    if "b" in args.legs:
        call = m.evaluate if K == 1 else (lambda: m.evaluate_gram(K))
        med, lo, hi, reps = windows(call)
        b_ms = med
        print(json.dumps(dict(rec, leg="b_evaluate" if K == 1 else "b_gram", channels=K, ms_per_call=med, min=lo, max=hi,
                              calls_per_window=reps)), flush=True)
    if "a" in args.legs and HAVE_CALL:
        a = coefficients(K)
        value, grad = m.evaluate_view_coefficients(a)
        assert np.isfinite(value) and np.all(np.isfinite(grad))
        if K == 1:   # all ones on one channel: evaluate()'s bits
            assert m.evaluate_view_coefficients(np.ones((1, n), np.float32))[0] == m.evaluate()
        med, lo, hi, reps = windows(lambda: m.evaluate_view_coefficients(a))
        out = dict(rec, leg="a_view_coefficients", channels=K, ms_per_call=med, min=lo, max=hi, calls_per_window=reps)
        if b_ms is not None:
            out.update(over_b_same_build=med / b_ms)
        print(json.dumps(out), flush=True)
    m.close()
