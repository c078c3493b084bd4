#!/usr/bin/env python3
"""Milliseconds per ecc_metric_evaluate_weighted_pose_deltas against the sequential weighted steps it replaces (GPU box):
    python scripts/bench_weighted_poses.py [--lib PATH] [--legs abcd] [--views 400] [--bins 768] [--tag NAME]
    python scripts/bench_weighted_poses.py --summarise LINES.jsonl BENCH.jsonl PARENT_REVISION > profiles/weighted_poses_1gpu.json
The metric holds 2 * views Radon intermediates (the data, then the line weights of scripts/bench_weighted.py), POLYNOMIAL.
(a) K = 600 poses of one moved view through ecc_metric_evaluate_weighted_pose_deltas, wall clock per call;
(b) the same 600 poses as ecc_metric_set_projections + ecc_metric_evaluate_weighted each -- exists on the parent revision too
    (--lib PATH loads another build, where (b), (c)'s sequential half and (p) alone run).  THE GATE: (b) of the parent / (a) >= 10;
(c) the same two for K = 13 (an optimiser step: the base itself and twelve probes); reported, no gate;
(d) the grid's weighted pair launch of (a) in ns per grid entry through enable_timing / last_kernel_ms, against
(p) the all-pairs pairs_weighted_kernel of evaluate_weighted in ns per pair under the same timer.  THE GATE: (d) <= 1.15 x (p) of the parent;
(e) nothing timed here: ten calls of evaluate_pose_deltas and of the weighted call at K = 600 for a kernel trace, which gives
    sum_poses_kernel's and sum_weighted_poses_kernel's time per launch.
Every shape is warmed up; a figure is the median of --windows windows of at least --min-seconds each, with min and max beside it.
Run the builds alternately inside one job (--tag parent_run1, this_run1, ...).  One JSON line per leg."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default="")
ap.add_argument("--legs", default="abcdp")
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
        t, p = "this_run%d" % run, "parent_run%d" % run
        a, b = pick(t, "a_", "ms_per_call"), pick(p, "b_", "ms_per_call")
        d, pp = pick(t, "d_", "ns_per_entry"), pick(p, "p_", "ns_per_pair")
        gate.append(dict(run=run, a_batch_600_ms=a, b_parent_sequential_600_ms=b, b_over_a=b / a, gate_10="passes" if b / a >= 10 else "missed",
                         c_batch_13_ms=pick(t, "c_batch", "ms_per_call"), c_parent_sequential_13_ms=pick(p, "c_sequential", "ms_per_call"),
                         d_grid_ns_per_entry=d, p_parent_all_pairs_ns_per_pair=pp, d_over_p=d / pp,
                         gate_1_15="passes" if d <= 1.15 * pp else "missed"))
    json.dump(dict(what="scripts/bench_weighted_poses.py on one MI355X (--summarise; see its docstring for every field): 400 views of "
                        "1024^2, 768^2 bins, POLYNOMIAL; median of 5 windows >= 0.3 s with min / max; the parent revision's library (%s) "
                        "and this revision's alternated in one job." % parent,
                   gate=gate, bench_py=dict(order=["parent", "this", "parent", "this"], evaluations_per_s=[b["value"] for b in bench],
                                            ms_per_step=[b.get("ms_per_step") for b in bench]), lines=rows), sys.stdout, indent=1)
    print()
    sys.exit(0)

if args.lib:
    os.environ["ECC_HIP_LIB"] = os.path.abspath(args.lib)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epipolarconsistency_amd import _lib  # noqa: E402
with open(_lib.LIB_PATH, "rb") as f:  # (looked up in the file: the package loads the library itself, after torch's runtime)
    HAVE_CALL = b"ecc_metric_evaluate_weighted_pose_deltas" in f.read()
if not HAVE_CALL:  # the parent's build: the sequential legs only
    for name in ("ecc_metric_evaluate_weighted_pose_deltas", "ecc_metric_evaluate_weighted_pairs"):
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
P0 = E.pack_projection_matrices(Ps)
rec = dict(views=n, bins=args.bins, lib=args.tag or (args.lib or "this"))
n_pairs = n * (n - 1) // 2


def poses(K):
    """K poses that each move one view (never view 0: the automatic object radius follows it): offsets, views, rows."""
    views = np.array([1 + (7 * k) % (n - 1) for k in range(K)], np.int32)
    rows = np.empty((K, 12))
    for k, v in enumerate(views):
        T = E.geometry.rigid_transform(tx=0.11 * (k % 13 + 1), ty=-0.05 * (v % 5), rz=0.0015 * (k % 7 + 1), rx=0.0007 * (v % 3))
        rows[k] = (P0[v].reshape(4, 3).T @ T).T.reshape(12)
    return np.arange(K + 1, dtype=np.int32), views, rows


def windows(fn, kernel=False):
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


m = E.MetricRadonIntermediate(ctx, Ps, [pool[v % len(pool)] for v in range(n)] + [wpool[(v + 3) % len(wpool)] for v in range(n)])
m.setSampling("polynomial")


def sequential(off, views, rows):
    P = P0.copy()
    out = []
    for k, v in enumerate(views):
        P[v] = rows[k]
        out.append(m.setProjectionMatrices(P).evaluate_weighted())
        P[v] = P0[v]
    m.setProjectionMatrices(P0)
    return out


for K, leg_batch, leg_seq in ((600, "a", "b"), (13, "c", "c")):
    off, views, rows = poses(K)
    if leg_batch in args.legs and HAVE_CALL:
        values, coverages = m.evaluate_weighted_pose_deltas_packed(off, views, rows)
        assert np.all(np.isfinite(values)) and np.all((coverages > 0) & (coverages < 1)) and m.last_batched_poses() == K
        med, lo, hi, reps = windows(lambda: m.evaluate_weighted_pose_deltas_packed(off, views, rows))
        name = "a_batch_600" if K == 600 else "c_batch_13"
        print(json.dumps(dict(rec, leg=name, poses=K, ms_per_call=med, min=lo, max=hi, calls_per_window=reps)), flush=True)
        if K == 600 and "d" in args.legs:
            med, lo, hi, reps = windows(lambda: m.evaluate_weighted_pose_deltas_packed(off, views, rows), kernel=True)
            print(json.dumps(dict(rec, leg="d_grid_pair_launch", kernel_ms=med, min=lo, max=hi, entries=n * K,
                                  ns_per_entry=1e6 * med / (n * K), calls_per_window=reps)), flush=True)
    if leg_seq in args.legs:
        med, lo, hi, reps = windows(lambda: sequential(off, views, rows))
        name = "b_sequential_600" if K == 600 else "c_sequential_13"
        print(json.dumps(dict(rec, leg=name, poses=K, ms_per_call=med, min=lo, max=hi, calls_per_window=reps)), flush=True)
if "p" in args.legs:
    med, lo, hi, reps = windows(m.evaluate_weighted, kernel=True)
    print(json.dumps(dict(rec, leg="p_all_pairs_weighted_kernel", kernel_ms=med, min=lo, max=hi, pairs=n_pairs,
                          ns_per_pair=1e6 * med / n_pairs, calls_per_window=reps)), flush=True)
if "e" in args.legs and HAVE_CALL:
    off, views, rows = poses(600)
    for _ in range(10):
        m.evaluate_pose_deltas_packed(off, views, rows)
        m.evaluate_weighted_pose_deltas_packed(off, views, rows)
    print(json.dumps(dict(rec, leg="e_calls_for_a_kernel_trace", calls_each=10, poses=600)), flush=True)
m.close()
