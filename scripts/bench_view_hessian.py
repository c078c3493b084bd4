#!/usr/bin/env python3
"""Milliseconds per ecc_metric_evaluate_view_hessian against what it is gated on (GPU box):
    python scripts/bench_view_hessian.py [--lib PATH] [--legs abhc] [--views 400] [--bins 768] [--channels 1,2,3,4]
(a) the pair kernel of evaluate_view_hessian(K) (csrc/view_hessian_kernel.hip, pairs_moments_kernel) through enable_timing /
    last_kernel_ms, on a metric of K * views Radon intermediates, POLYNOMIAL;
(b) what it is gated against, under the same timer: the pair kernel of evaluate_gram(K) on the same metric for K = 2 .. 4 -- the same
    4 K gathers per kappa step -- and of evaluate() (no cost image) on a single-channel metric for K = 1.  (b) exists on the parent
    revision too: --lib PATH loads another build of the library, where legs (b) and (c) run.  THE GATE: (a) <= 1.15 x (b) of the
    parent's build; (b) on both builds shows that the existing paths were left alone;
(h) the whole call with H copied to the host, wall clock (the copy is 8 (n K)^2 bytes: 20 MB at 400 views and K = 4);
(c) the only way to the matrix without the call: one evaluate_view_coefficients at one-hot coefficients per column, wall clock per
    call, times n K.  THE GATE: (h) of this build at least 10 x faster than n K x (c) of the parent's build, at K = 2 and K = 4.
Every shape is warmed up; a wall-clock figure is the median of --windows windows of at least --min-seconds each, a kernel figure the
median of the event times of the same calls, with the spread (min .. max) beside it.  Run the builds alternately inside one job
(parent, this, parent, this).  One JSON line per leg and K.
--once K[,K...]: two calls of the whole call per K and nothing else (for a kernel trace: the assembly kernel's time is read there)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default="")
ap.add_argument("--legs", default="abhc")
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
    HAVE_CALL = b"ecc_metric_evaluate_view_hessian" in f.read()
if not HAVE_CALL:  # the parent's build: legs (b) and (c) only
    _lib.SIGNATURES.pop("ecc_metric_evaluate_view_hessian", None)
import epipolarconsistency_amd as E  # noqa: E402
from epipolarconsistency_amd import synthetic  # noqa: E402

ctx = E.Context(0)
ctx.enable_timing(True)
rng = np.random.default_rng(7)
S, n = 1024, args.views
pool = [E.RadonIntermediate.from_host(ctx, rng.standard_normal((args.bins, args.bins)).astype(np.float32), S, S) for _ in range(11)]
Ps = synthetic.short_scan(n, S, S, 0.308)
rec = dict(views=n, bins=args.bins, lib=args.tag or (args.lib or "this"))


def windows(fn, kernel=False):
    """(median, min, max, calls per window) of the wall-clock ms per call; kernel=True: of the pair kernel's event time per call."""
    fn()  # warm-up of this shape
    fn()
    t0 = time.perf_counter()
    fn()
    reps = max(1, int(np.ceil(args.min_seconds / max(time.perf_counter() - t0, 1e-6))))
    ms = []
    for _ in range(args.windows):
        t0, ev = time.perf_counter(), []
        for _ in range(reps):
            fn()
            if kernel:
                ev.append(ctx.last_kernel_ms("pairs"))
        ms.append(float(np.median(ev)) if kernel else 1e3 * (time.perf_counter() - t0) / reps)
    return float(np.median(ms)), float(min(ms)), float(max(ms)), reps


def channel_metric(K):  # K * n intermediates, channel-major, neighbouring channels and views on different arrays (scripts/bench_gram.py)
    return E.MetricRadonIntermediate(ctx, Ps, [pool[(3 * c + v) % len(pool)] for c in range(K) for v in range(n)]).setSampling("polynomial")


if args.once:
    for K in [int(x) for x in args.once.split(",")]:
        m = channel_metric(K)
        m.evaluate_view_hessian(K)
        m.evaluate_view_hessian(K)
        m.close()
    sys.exit(0)

for K in [int(x) for x in args.channels.split(",")]:
    m = channel_metric(K)
    b_ms = None
    if "b" in args.legs:
        call = m.evaluate if K == 1 else (lambda: m.evaluate_gram(K))
        med, lo, hi, reps = windows(call, kernel=True)
        b_ms = med
        print(json.dumps(dict(rec, leg="b_evaluate_kernel" if K == 1 else "b_gram_kernel", channels=K, kernel_ms=med, min=lo, max=hi,
                              calls_per_window=reps)), flush=True)
    if "c" in args.legs:
        a = np.zeros((K, n), np.float32)
        a[K - 1, n // 2] = 1.0
        med, lo, hi, reps = windows(lambda: m.evaluate_view_coefficients(a))
        print(json.dumps(dict(rec, leg="c_one_hot_view_coefficients", channels=K, ms_per_call=med, min=lo, max=hi, calls_per_window=reps,
                              calls_for_the_matrix=n * K, ms_for_the_matrix=med * n * K)), flush=True)
    if "a" in args.legs and HAVE_CALL:
        H = m.evaluate_view_hessian(K)
        assert H.shape == (n * K, n * K) and np.all(np.isfinite(H)) and np.array_equal(H, H.T)
        med, lo, hi, reps = windows(lambda: m.evaluate_view_hessian(K), kernel=True)
        out = dict(rec, leg="a_moments_kernel", channels=K, kernel_ms=med, min=lo, max=hi, calls_per_window=reps)
        if b_ms is not None:
            out.update(over_b_same_build=med / b_ms)
        print(json.dumps(out), flush=True)
    if "h" in args.legs and HAVE_CALL:
        med, lo, hi, reps = windows(lambda: m.evaluate_view_hessian(K))
        print(json.dumps(dict(rec, leg="h_whole_call_with_H", channels=K, ms_per_call=med, min=lo, max=hi, calls_per_window=reps,
                              H_megabytes=8e-6 * (n * K) ** 2)), flush=True)
    m.close()
