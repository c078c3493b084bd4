#!/usr/bin/env python3
"""Milliseconds per pair launch of ecc_metric_evaluate_robust against what it is gated on (GPU box):
    python scripts/bench_robust.py [--lib PATH] [--legs pwr] [--views 400] [--bins 768] [--tag NAME]
    python scripts/bench_robust.py --summarise LINES.jsonl BENCH.jsonl PARENT_REVISION > profiles/robust_1gpu.json
400 views of 1024^2, 768^2 bins, POLYNOMIAL; every kernel figure through enable_timing / last_kernel_ms.
(p) pairs_kernel: evaluate() over all pairs on the metric of n Radon intermediates;
(w) pairs_weighted_kernel: evaluate_weighted on a metric of 2 n intermediates (the same data, then line weights);
(r) pairs_robust_kernel (csrc/robust_kernel.hip): evaluate_robust on the metric of (p), once per loss, at delta = robust_scale of
    its own delta = inf call (a fixed share of the samples outside delta, whatever the data).
(p) and (w) exist on the parent revision too: --lib PATH loads another build of the library, where they alone run.  THE GATE: every
(r) of this revision is below (w) of the parent's build by more than the windows' spread -- max of (r) < min of (w): the kernel does
half of (w)'s gathers, so anything else means spills or a lost dispatch.  (r) / (p) is reported, not gated: what two divisions and
three more float64 sums per kappa step cost beside the same four gathers.
Every shape is warmed up; a figure is the median over --windows windows (of at least --min-seconds each) of the window's median
event time, with the spread (min .. max) beside it.  Run the builds alternately inside one job (parent, this, parent, this; --tag
parent_run1, this_run1, ...).  One JSON line per leg.
--summarise: the gate per run from those lines, with bench.py's result lines of parent / this / parent / this."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default="")
ap.add_argument("--legs", default="pwr")
ap.add_argument("--views", type=int, default=400)
ap.add_argument("--bins", type=int, default=768)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--min-seconds", type=float, default=0.3)
ap.add_argument("--tag", default="")
ap.add_argument("--summarise", nargs=3, metavar=("LINES", "BENCH", "PARENT"))
args = ap.parse_args()

LOSSES = ("huber", "truncated", "geman_mcclure")

if args.summarise:
    lines_path, bench_path, parent = args.summarise
    rows = [json.loads(l) for l in open(lines_path) if l.strip().startswith("{")]
    bench = [json.loads(l) for l in open(bench_path) if l.strip().startswith("{")]

    def pick(tag, leg):
        return [r for r in rows if r["lib"] == tag and r["leg"].startswith(leg)][0]
    gate = []
    for run in (1, 2):
        w, p = pick("parent_run%d" % run, "w_"), pick("parent_run%d" % run, "p_")
        entry = dict(run=run, w_parent_kernel_ms=w["kernel_ms"], w_parent_min=w["min"], w_parent_max=w["max"], p_parent_kernel_ms=p["kernel_ms"],
                     p_this_kernel_ms=pick("this_run%d" % run, "p_")["kernel_ms"], w_this_kernel_ms=pick("this_run%d" % run, "w_")["kernel_ms"])
        ok = True
        for loss in LOSSES:
            r = pick("this_run%d" % run, "r_" + loss)
            entry["r_" + loss] = dict(kernel_ms=r["kernel_ms"], min=r["min"], max=r["max"], over_w_parent=r["kernel_ms"] / w["kernel_ms"],
                                      over_p_parent=r["kernel_ms"] / p["kernel_ms"], inlier_mass=r["inlier_mass"])
            ok = ok and r["max"] < w["min"]
        entry["gate_r_max_below_w_parent_min"] = "passes" if ok else "missed"
        gate.append(entry)
    json.dump(dict(what="scripts/bench_robust.py on one MI355X (--summarise; see its docstring for every field): 400 views of 1024^2, "
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
    HAVE_CALL = b"ecc_metric_evaluate_robust" in f.read()
if not HAVE_CALL:  # the parent's build: legs (p) and (w) only
    for name in ("ecc_metric_evaluate_robust", "ecc_metric_evaluate_robust_pairs", "ecc_host_robust_scale"):
        _lib.SIGNATURES.pop(name, None)
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


def windows(fn):
    """(median, min, max, calls per window) over the windows of the median event time of the pair kernel per call, ms."""
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


# neighbouring views on different arrays (scripts/bench_gram.py)
data = [pool[v % len(pool)] for v in range(n)]
m = E.MetricRadonIntermediate(ctx, Ps, data)
m.setSampling("polynomial")
p_ms = None
if "p" in args.legs:
    med, lo, hi, reps = windows(m.evaluate)
    p_ms = med
    print(json.dumps(dict(rec, leg="p_pairs_kernel", kernel_ms=med, min=lo, max=hi, calls_per_window=reps)), flush=True)
if "w" in args.legs:
    m2 = E.MetricRadonIntermediate(ctx, Ps, data + [wpool[(v + 3) % len(wpool)] for v in range(n)])
    m2.setSampling("polynomial")
    med, lo, hi, reps = windows(m2.evaluate_weighted)
    print(json.dumps(dict(rec, leg="w_weighted_kernel", kernel_ms=med, min=lo, max=hi, calls_per_window=reps)), flush=True)
    m2.close()
if "r" in args.legs and HAVE_CALL:
    value, mass, terms = m.evaluate_robust(E.LOSS_HUBER, float("inf"), want_pairs=True)
    assert value == m.evaluate() and mass == 1.0
    delta = E.robust_scale(terms)
    for code, loss in enumerate(LOSSES):
        value, mass = m.evaluate_robust(code, delta)
        assert np.isfinite(value) and 0.0 < mass < 1.0
        med, lo, hi, reps = windows(lambda: m.evaluate_robust(code, delta))
        out = dict(rec, leg="r_%s_kernel" % loss, kernel_ms=med, min=lo, max=hi, calls_per_window=reps, delta=delta, inlier_mass=mass)
        if p_ms is not None:
            out.update(over_p_same_build=med / p_ms)
        print(json.dumps(out), flush=True)
m.close()
