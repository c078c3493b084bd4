#!/usr/bin/env python3
"""The time of ecc_metric_evaluate_residual_histogram's pair kernel beside the kernels it is measured against (GPU box):
    python scripts/bench_residual_histogram.py [--lib PATH] [--legs rmh] [--views 400] [--bins 768] [--tag NAME]
    python scripts/bench_residual_histogram.py --summarise LINES.jsonl BENCH.jsonl PARENT_REVISION
The metric holds `views` Radon intermediates of 1024^2 images, POLYNOMIAL.  Every leg is a pair kernel's event time through
enable_timing / last_kernel_ms on the same metric:
(r) pairs_robust_kernel through evaluate_robust (truncated loss, delta = 2 x robust_scale): the same 4 gathers per kappa step, no
    counting.  It exists on the parent revision too: --lib PATH loads another build of the library, where legs (r) and (m) run;
(m) pairs_robust_map_kernel through evaluate_robust_map of every view, same loss and delta: eight global 64-bit atomics per sample;
(h) pairs_residual_histogram_kernel through evaluate_residual_histogram at n_bins 64 and 256, the width 4 x robust_scale / n_bins
    (this build only).  THE GATE: (h) < (m) of the parent's build, or the LDS counters have not done their job; (h) / (r) of the
    parent's build is reported with the windows' spread and not gated.
Every shape is warmed up; a figure is the median over --windows windows (at least --min-seconds each) of the median event time of the
window's calls, with the windows' min and max beside it.  Run the builds alternately inside one job (parent, this, parent, this;
--tag parent_run1, this_run1, ...).  One JSON line per leg.
--summarise: the gate and the ratios per run from those lines, with bench.py's result lines of parent / this / parent / this; the exit
status is 1 when any run misses the gate."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default="")
ap.add_argument("--legs", default="rmh")
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

    def pick(tag, leg):
        return [r for r in rows if r["lib"] == tag and r["leg"] == leg][0]
    gate = []
    for run in (1, 2):
        r, m = pick("parent_run%d" % run, "r_robust_kernel"), pick("parent_run%d" % run, "m_robust_map_kernel")
        for B in (64, 256):
            h = pick("this_run%d" % run, "h_histogram_kernel_%d" % B)
            gate.append(dict(run=run, n_bins=B, h_kernel_ms=h["kernel_ms"], h_min=h["min"], h_max=h["max"], r_parent_kernel_ms=r["kernel_ms"],
                             r_this_kernel_ms=pick("this_run%d" % run, "r_robust_kernel")["kernel_ms"], m_parent_kernel_ms=m["kernel_ms"],
                             h_over_r_parent=h["kernel_ms"] / r["kernel_ms"], h_over_r_parent_min=h["min"] / r["max"],
                             h_over_r_parent_max=h["max"] / r["min"], gate_faster_than_map="passes" if h["kernel_ms"] < m["kernel_ms"] else "missed"))
    json.dump(dict(what="scripts/bench_residual_histogram.py on one MI355X (--summarise; see its docstring for every field): 400 views of "
                        "1024^2, 768^2 bins, POLYNOMIAL; median of 5 windows >= 0.3 s with min / max; the parent revision's library (%s) and "
                        "this revision's alternated in one job." % parent,
                   gate=gate, bench_py=dict(order=["parent", "this", "parent", "this"], evaluations_per_s=[b["value"] for b in bench],
                                            ms_per_step=[b.get("ms_per_step") for b in bench]), lines=rows), sys.stdout, indent=1)
    print()
    sys.exit(0 if all(g["gate_faster_than_map"] == "passes" for g in gate) else 1)   # a missed gate fails the job

if args.lib:
    os.environ["ECC_HIP_LIB"] = os.path.abspath(args.lib)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epipolarconsistency_amd import _lib  # noqa: E402
with open(_lib.LIB_PATH, "rb") as f:  # (looked up in the file: the package loads the library itself, after torch's runtime)
    HAVE_CALL = b"ecc_metric_evaluate_residual_histogram" in f.read()
if not HAVE_CALL:  # the parent's build: legs (r) and (m) only
    for name in [k for k in _lib.SIGNATURES if "histogram" in k]:
        _lib.SIGNATURES.pop(name, None)
import epipolarconsistency_amd as E  # noqa: E402
from epipolarconsistency_amd import synthetic  # noqa: E402

ctx = E.Context(0)
ctx.enable_timing(True)
rng = np.random.default_rng(7)
S, n = 1024, args.views
pool = [E.RadonIntermediate.from_host(ctx, rng.standard_normal((args.bins, args.bins)).astype(np.float32), S, S) for _ in range(11)]
rec = dict(views=n, bins=args.bins, lib=args.tag or (args.lib or "this"))


def windows(fn):
    """(median, min, max, calls per window) over the windows of the median event time of the pair kernel per call, in ms."""
    fn()  # warm-up of this shape
    fn()
    t0 = time.perf_counter()
    fn()
    reps = max(1, int(np.ceil(args.min_seconds / max(time.perf_counter() - t0, 1e-6))))
    ms = []
    for _ in range(args.windows):
        ev = []
        for _ in range(reps):
            fn()
            ev.append(ctx.last_kernel_ms("pairs"))
        ms.append(float(np.median(ev)))
    return float(np.median(ms)), float(min(ms)), float(max(ms)), reps


Ps = synthetic.short_scan(n, S, S, 0.308)
m = E.MetricRadonIntermediate(ctx, Ps, [pool[v % len(pool)] for v in range(n)]).setSampling("polynomial")
scale = E.robust_scale(m.evaluate_robust(E.LOSS_TRUNCATED, float("inf"), want_pairs=True)[-1])
delta = float(np.float32(2.0 * scale))
assert scale > 0.0
if "r" in args.legs:
    med, lo, hi, reps = windows(lambda: m.evaluate_robust(E.LOSS_TRUNCATED, delta))
    print(json.dumps(dict(rec, leg="r_robust_kernel", kernel_ms=med, min=lo, max=hi, calls_per_window=reps, delta=delta)), flush=True)
if "m" in args.legs:
    med, lo, hi, reps = windows(lambda: m.evaluate_robust_map(E.LOSS_TRUNCATED, delta))
    print(json.dumps(dict(rec, leg="m_robust_map_kernel", kernel_ms=med, min=lo, max=hi, calls_per_window=reps, delta=delta)), flush=True)
if "h" in args.legs and HAVE_CALL:
    for B in (64, 256):
        width = float(np.float32(4.0 * scale / B))
        counts = m.evaluate_residual_histogram(width, B)
        assert counts.shape == (n, B) and counts.sum() > 0 and np.array_equal(counts, m.evaluate_residual_histogram(width, B))
        med, lo, hi, reps = windows(lambda: m.evaluate_residual_histogram(width, B))
        print(json.dumps(dict(rec, leg="h_histogram_kernel_%d" % B, kernel_ms=med, min=lo, max=hi, calls_per_window=reps, width=width,
                              overflow_share=float(counts[:, -1].sum() / counts.sum()))), flush=True)
m.close()
