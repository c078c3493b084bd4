#!/usr/bin/env python3
"""Milliseconds per ecc_metric_evaluate_weighted against what it is gated on (GPU box):
    python scripts/bench_weighted.py [--lib PATH] [--legs abw] [--views 400] [--bins 768] [--tag NAME]
    python scripts/bench_weighted.py --summarise LINES.jsonl BENCH.jsonl PARENT_REVISION > profiles/weighted_1gpu.json
The metric holds 2 * views Radon intermediates (the data, then the line weights), POLYNOMIAL.
(a) the pair kernel of evaluate_weighted (csrc/weighted_kernel.hip, pairs_weighted_kernel) through enable_timing / last_kernel_ms;
(b) what it is gated against, under the same timer on the same metric: the pair kernel of evaluate_view_coefficients at two channels
    (pairs_coeff_kernel<true, 2>: the same 8 gathers per kappa step, more arithmetic).  (b) exists on the parent revision too:
    --lib PATH loads another build of the library, where leg (b) alone runs.  THE GATE: (a) <= 1.15 x (b) of the parent's build;
    (b) on both builds shows that the existing path was left alone;
(w) the whole evaluate_weighted call, wall clock.
Every shape is warmed up; a wall-clock figure is the median of --windows windows of at least --min-seconds each, a kernel figure the
median of the event times of the same calls, with the spread (min .. max) beside it.  Run the builds alternately inside one job
(parent, this, parent, this; --tag parent_run1, this_run1, ...).  One JSON line per leg.
--summarise: the gate per run from those lines (a of this_runN against b of parent_runN), with bench.py's result lines of
parent / this / parent / this."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default="")
ap.add_argument("--legs", default="abw")
ap.add_argument("--views", type=int, default=400)
ap.add_argument("--bins", type=int, default=768)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--min-seconds", type=float, default=0.3)
ap.add_argument("--tag", default="")
ap.add_argument("--summarise", nargs=3, metavar=("LINES", "BENCH", "PARENT"))
args = ap.parse_args()

if args.summarise:
    lines_path, bench_path, parent = args.summarise
    rows = [json.loads(l) for l in open(lines_path) if l.strip().startswith("{")]
    bench = [json.loads(l) for l in open(bench_path) if l.strip().startswith("{")]

    def pick(tag, leg, key):
        return [r for r in rows if r["lib"] == tag and r["leg"].startswith(leg)][0][key]
    gate = []
    for run in (1, 2):
        a, b = pick("this_run%d" % run, "a_", "kernel_ms"), pick("parent_run%d" % run, "b_", "kernel_ms")
        gate.append(dict(run=run, a_kernel_ms=a, b_parent_kernel_ms=b, b_this_kernel_ms=pick("this_run%d" % run, "b_", "kernel_ms"),
                         a_over_b_parent=a / b, gate_1_15="passes" if a <= 1.15 * b else "missed",
                         w_whole_call_ms=pick("this_run%d" % run, "w_", "ms_per_call")))
    json.dump(dict(what="scripts/bench_weighted.py on one MI355X (--summarise; see its docstring for every field): 400 views of 1024^2, "
                        "768^2 bins, POLYNOMIAL; median of 5 windows >= 0.3 s with min / max; the parent revision's library (%s) and this "
                        "revision's alternated in one job." % parent,
                   gate=gate, bench_py=dict(order=["parent", "this", "parent", "this"], evaluations_per_s=[b["value"] for b in bench],
                                            ms_per_step=[b.get("ms_per_step") for b in bench]), lines=rows), sys.stdout, indent=1)
    print()
    sys.exit(0)

if args.lib:
    os.environ["ECC_HIP_LIB"] = os.path.abspath(args.lib)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epipolarconsistency_amd import _lib  # noqa: E402
with open(_lib.LIB_PATH, "rb") as f:  # (looked up in the file: the package loads the library itself, after torch's runtime)
    HAVE_CALL = b"ecc_metric_evaluate_weighted" in f.read()
if not HAVE_CALL:  # the parent's build: leg (b) only
    _lib.SIGNATURES.pop("ecc_metric_evaluate_weighted", None)
import epipolarconsistency_amd as E  # noqa: E402
from epipolarconsistency_amd import synthetic  # noqa: E402

ctx = E.Context(0)
ctx.enable_timing(True)
rng = np.random.default_rng(7)
S, n = 1024, args.views
pool = [E.RadonIntermediate.from_host(ctx, rng.standard_normal((args.bins, args.bins)).astype(np.float32), S, S) for _ in range(11)]
wpool = [E.RadonIntermediate.from_host(ctx, rng.random((args.bins, args.bins)).astype(np.float32), S, S, filter=E.FILTER_NONE) for _ in range(11)]
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


# the data, then the weights: neighbouring views on different arrays (scripts/bench_gram.py)
m = E.MetricRadonIntermediate(ctx, Ps, [pool[v % len(pool)] for v in range(n)] + [wpool[(v + 3) % len(wpool)] for v in range(n)])
m.setSampling("polynomial")
b_ms = None
if "b" in args.legs:
    coeffs = np.ones((2, n), np.float32)
    med, lo, hi, reps = windows(lambda: m.evaluate_view_coefficients(coeffs), kernel=True)
    b_ms = med
    print(json.dumps(dict(rec, leg="b_view_coefficients_kernel", kernel_ms=med, min=lo, max=hi, calls_per_window=reps)), flush=True)
if "a" in args.legs and HAVE_CALL:
    value, coverage = m.evaluate_weighted()
    assert np.isfinite(value) and 0.0 < coverage < 1.0
    med, lo, hi, reps = windows(m.evaluate_weighted, kernel=True)
    out = dict(rec, leg="a_weighted_kernel", kernel_ms=med, min=lo, max=hi, calls_per_window=reps)
    if b_ms is not None:
        out.update(over_b_same_build=med / b_ms)
    print(json.dumps(out), flush=True)
if "w" in args.legs and HAVE_CALL:
    med, lo, hi, reps = windows(m.evaluate_weighted)
    print(json.dumps(dict(rec, leg="w_whole_call", ms_per_call=med, min=lo, max=hi, calls_per_window=reps)), flush=True)
m.close()
