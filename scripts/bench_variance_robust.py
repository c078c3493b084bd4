#!/usr/bin/env python3
"""Milliseconds per ecc_metric_evaluate_variance_robust against what it is gated on (GPU box):
    python scripts/bench_variance_robust.py [--lib PATH] [--legs avwpt] [--views 400] [--bins 768] [--tag NAME]
    python scripts/bench_variance_robust.py --summarise LINES.jsonl BENCH.jsonl PARENT_REVISION
The metric holds 2 * views Radon intermediates, POLYNOMIAL: the data, then one positive field per view (0.25 * 16^U(0, 1) per bin),
which evaluate_weighted_robust reads as line weights and evaluate_variance_robust as variances -- the same 8 gathers per kappa step and
the same five per-lane sums either way.  The loss is the truncated one, delta = 2 x the form's own scale of the delta = inf rows.
(a) the pair kernel of evaluate_weighted_robust (pairs_weighted_robust_kernel) through enable_timing / last_kernel_ms.  It exists on
    the parent revision too: --lib PATH loads another build of the library, where leg (a) alone runs;
(v) the pair kernel of evaluate_variance_robust (csrc/variance_robust_kernel.hip, pairs_variance_robust_kernel) under the same timer
    on the same metric.  THE GATE: (v) <= 1.15 x (a) of the parent's build; (a) on both builds shows that the existing path was left
    alone;
(w) the whole evaluate_variance_robust call, wall clock;
(p) K = 600 poses of one moved view through evaluate_variance_robust_pose_deltas, and the same poses as setProjectionMatrices +
    evaluate_variance_robust each, wall clock per call;
(t) K = 600 transforms of 20 + 20 views through evaluate_variance_robust_transforms, and the same as setProjectionMatrices +
    evaluate_variance_robust_pairs of the cross list each (both under a fixed object radius), wall clock per call.
Every shape is warmed up; a wall-clock figure is the median of --windows windows of at least --min-seconds each, a kernel figure the
median of the event times of the same calls, with the spread (min .. max) beside it.  Run the builds alternately inside one job
(parent, this, parent, this; --tag parent_run1, this_run1, ...).  One JSON line per leg.
--summarise: the gate per run from those lines (v of this_runN against a of parent_runN), with bench.py's result lines of
parent / this / parent / this."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default="")
ap.add_argument("--legs", default="avwpt")
ap.add_argument("--views", type=int, default=400)
ap.add_argument("--bins", type=int, default=768)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--min-seconds", type=float, default=0.3)
ap.add_argument("--floor", type=float, default=1.5)
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
        v, a = pick("this_run%d" % run, "v_", "kernel_ms"), pick("parent_run%d" % run, "a_", "kernel_ms")
        gate.append(dict(run=run, v_kernel_ms=v, a_parent_kernel_ms=a, a_this_kernel_ms=pick("this_run%d" % run, "a_", "kernel_ms"),
                         v_over_a_parent=v / a, gate_1_15="passes" if v <= 1.15 * a else "missed"))
    json.dump(dict(what="scripts/bench_variance_robust.py on one MI355X (--summarise; see its docstring for every field): 400 views of "
                        "1024^2, 768^2 bins, POLYNOMIAL; median of 5 windows >= 0.3 s with min / max; the parent revision's library (%s) and "
                        "this revision's alternated in one job." % parent,
                   gate=gate, bench_py=dict(order=["parent", "this", "parent", "this"], evaluations_per_s=[b["value"] for b in bench],
                                            ms_per_step=[b.get("ms_per_step") for b in bench]), lines=rows), sys.stdout, indent=1)
    print()
    sys.exit(0)

if args.lib:
    os.environ["ECC_HIP_LIB"] = os.path.abspath(args.lib)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epipolarconsistency_amd import _lib  # noqa: E402
with open(_lib.LIB_PATH, "rb") as f:  # (looked up in the file: the package loads the library itself, after torch's runtime)
    HAVE_CALL = b"ecc_metric_evaluate_variance_robust" in f.read()
if not HAVE_CALL:  # the parent's build: leg (a) only
    for name in [k for k in _lib.SIGNATURES if "variance_robust" in k]:
        _lib.SIGNATURES.pop(name, None)
import epipolarconsistency_amd as E  # noqa: E402
from epipolarconsistency_amd import synthetic  # noqa: E402

ctx = E.Context(0)
ctx.enable_timing(True)
rng = np.random.default_rng(7)
S, n = 1024, args.views
LOSS, INF = E.LOSS_TRUNCATED, float("inf")
pool = [E.RadonIntermediate.from_host(ctx, rng.standard_normal((args.bins, args.bins)).astype(np.float32), S, S) for _ in range(11)]
vpool = [E.RadonIntermediate.from_host(ctx, (0.25 * 16.0 ** rng.random((args.bins, args.bins))).astype(np.float32), S, S, filter=E.FILTER_NONE)
         for _ in range(11)]
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


def metric(views):
    """The data, then the fields: neighbouring views on different arrays (scripts/bench_gram.py)."""
    Ps = synthetic.short_scan(views, S, S, 0.308)
    m = E.MetricRadonIntermediate(ctx, Ps, [pool[v % len(pool)] for v in range(views)] + [vpool[(v + 3) % len(vpool)] for v in range(views)])
    return m.setSampling("polynomial"), Ps, E.pack_projection_matrices(Ps)


def sigmas(m):
    """delta = 2 x the form's own scale, a float32."""
    return float(np.float32(E.variance_robust_scale(m.evaluate_variance_robust(LOSS, INF, args.floor, want_pairs=True)[3], 2.0)))


if set(args.legs) & set("avwp"):
    m, Ps, P0 = metric(n)
    a_ms = None
    if "a" in args.legs:
        raw_delta = float(np.float32(E.weighted_robust_scale(m.evaluate_weighted_robust(LOSS, INF, want_pairs=True)[3], 2.0)))
        med, lo, hi, reps = windows(lambda: m.evaluate_weighted_robust(LOSS, raw_delta), kernel=True)
        a_ms = med
        print(json.dumps(dict(rec, leg="a_weighted_robust_kernel", kernel_ms=med, min=lo, max=hi, calls_per_window=reps, delta=raw_delta)), flush=True)
    if HAVE_CALL and set(args.legs) & set("vwp"):
        delta = sigmas(m)
    if "v" in args.legs and HAVE_CALL:
        value, mean_weight, inlier_mass = m.evaluate_variance_robust(LOSS, delta, args.floor)
        assert np.isfinite(value) and 0.0 < mean_weight <= 1.0 / args.floor and 0.0 < inlier_mass < 1.0
        med, lo, hi, reps = windows(lambda: m.evaluate_variance_robust(LOSS, delta, args.floor), kernel=True)
        out = dict(rec, leg="v_variance_robust_kernel", kernel_ms=med, min=lo, max=hi, calls_per_window=reps, floor=args.floor, delta=delta,
                   inlier_mass=inlier_mass)
        if a_ms is not None:
            out.update(over_a_same_build=med / a_ms)
        print(json.dumps(out), flush=True)
    if "w" in args.legs and HAVE_CALL:
        med, lo, hi, reps = windows(lambda: m.evaluate_variance_robust(LOSS, delta, args.floor))
        print(json.dumps(dict(rec, leg="w_whole_call", ms_per_call=med, min=lo, max=hi, calls_per_window=reps)), flush=True)
    if "p" in args.legs and HAVE_CALL:
        K = 600
        views = np.array([1 + (7 * k) % (n - 1) for k in range(K)], np.int32)   # never view 0: the automatic object radius follows it
        rows = np.empty((K, 12))
        for k, v in enumerate(views):
            T = E.geometry.rigid_transform(tx=0.11 * (k % 13 + 1), ty=-0.05 * (v % 5), rz=0.0015 * (k % 7 + 1), rx=0.0007 * (v % 3))
            rows[k] = (P0[v].reshape(4, 3).T @ T).T.reshape(12)
        off = np.arange(K + 1, dtype=np.int32)

        def sequential():
            P = P0.copy()
            out = []
            for k, v in enumerate(views):
                P[v] = rows[k]
                out.append(m.setProjectionMatrices(P).evaluate_variance_robust(LOSS, delta, args.floor)[0])
                P[v] = P0[v]
            m.setProjectionMatrices(P0)
            return np.array(out)
        batch = m.evaluate_variance_robust_pose_deltas_packed(off, views, rows, LOSS, delta, args.floor)[0]
        assert m.last_batched_poses() == K and np.array_equal(batch, sequential())
        med, lo, hi, reps = windows(lambda: m.evaluate_variance_robust_pose_deltas_packed(off, views, rows, LOSS, delta, args.floor))
        print(json.dumps(dict(rec, leg="p_batch_600_poses", ms_per_call=med, min=lo, max=hi, calls_per_window=reps)), flush=True)
        med_s, lo, hi, reps = windows(sequential)
        print(json.dumps(dict(rec, leg="p_sequential_600_poses", ms_per_call=med_s, min=lo, max=hi, calls_per_window=reps,
                              sequential_over_batch=med_s / med)), flush=True)
    m.close()

if "t" in args.legs and HAVE_CALL:
    ns = nt = 20
    K = 600
    m, Ps, P0 = metric(ns + nt)
    m.setObjectRadius(120.0)
    delta = sigmas(m)
    Ts = [E.geometry.rigid_transform(tx=0.9 * (k % 17), ty=-0.4 * (k % 5), tz=0.3 * (k % 3), rz=0.0015 * (k % 11), rx=0.0007 * (k % 4)) for k in range(K)]
    j, i = np.divmod(np.arange(ns * nt), ns)
    idx = np.ascontiguousarray(np.stack([i, ns + j, i, ns + j], axis=1).astype(np.int32))

    def sequential():
        out = []
        for Tk in Ts:
            composed = [E.geometry.compose_transform(P, Tk) for P in Ps[:ns]] + list(Ps[ns:])
            out.append(m.setProjectionMatrices(composed).evaluate_variance_robust_pairs(idx, LOSS, delta, args.floor)[0])
        m.setProjectionMatrices(Ps)
        return np.array(out)
    batch = m.evaluate_variance_robust_transforms(ns, Ts, LOSS, delta, args.floor)[0]
    assert m.last_batched_transforms() == K and np.array_equal(batch, sequential())
    med, lo, hi, reps = windows(lambda: m.evaluate_variance_robust_transforms(ns, Ts, LOSS, delta, args.floor))
    print(json.dumps(dict(rec, leg="t_batch_600_transforms", views=ns + nt, ms_per_call=med, min=lo, max=hi, calls_per_window=reps)), flush=True)
    med_s, lo, hi, reps = windows(sequential)
    print(json.dumps(dict(rec, leg="t_sequential_600_transforms", views=ns + nt, ms_per_call=med_s, min=lo, max=hi, calls_per_window=reps,
                          sequential_over_batch=med_s / med)), flush=True)
    m.close()
