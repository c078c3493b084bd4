#!/usr/bin/env python3
"""Milliseconds per ecc_metric_evaluate_weighted_transforms against the sequential weighted steps it replaces (GPU box):
    python scripts/bench_weighted_transforms.py [--lib PATH] [--legs abtsdepq] [--source 20] [--target 20] [--bins 768] [--tag NAME]
    python scripts/bench_weighted_transforms.py --summarise LINES.jsonl BENCH.jsonl PARENT_REVISION > profiles/weighted_transforms_1gpu.json
20 source + 20 target views of 1024^2, 768^2 bins, POLYNOMIAL, the object radius FIXED (--radius; 0: at the automatic radius of the
base's first view).  The weighted metric holds 2 * views Radon intermediates (the data, then the line weights of
scripts/bench_weighted.py), the unweighted one the data alone.
(a) K = 600 transforms through ecc_metric_evaluate_weighted_transforms, wall clock per call;
(b) the same 600 as ecc_metric_set_projections + ecc_metric_evaluate_weighted_pairs each -- exists on the parent revision too
    (--lib PATH loads another build, where (a) and (d) do not run);
(t) the unweighted ecc_metric_evaluate_transforms of the same 600, and (s) its sequential form, set_projections + evaluate(index list).
    THE CALL GATE: (b) / (a) >= 1/2 x (s) / (t), (b), (s), (t) of the parent: the sequential weighted step has the unweighted step's
    fixed costs and about twice its kernel work, so the batch's advantage may halve and should not do worse;
(d) the grid's weighted pair launch of (a) in ns per grid entry through enable_timing / last_kernel_ms;
(e) the unweighted transform grid's pair launch of (t) per entry under the same timer;
(p), (q) the all-pairs pairs_weighted_kernel of evaluate_weighted and pairs_kernel of evaluate() in ns per pair, at --views 400 views.
    THE KERNEL GATE: (d) / (e) <= 1.15 x (p) / (q), (e), (p), (q) of the parent: per entry the weighted grid may cost over the
    unweighted grid what the weighted kernel costs over pairs_kernel on all pairs, plus 15 %;
(x) nothing timed here: ten calls of (a)'s shape for a kernel trace, which gives sum_weighted_transforms_kernel's time per launch.
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
ap.add_argument("--legs", default="abtsdepq")
ap.add_argument("--source", type=int, default=20)
ap.add_argument("--target", type=int, default=20)
ap.add_argument("--views", type=int, default=400)
ap.add_argument("--bins", type=int, default=768)
ap.add_argument("--K", type=int, default=600)
ap.add_argument("--radius", type=float, default=0.0)
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
        t_, p_ = "this_run%d" % run, "parent_run%d" % run
        a, b = pick(t_, "a_", "ms_per_call"), pick(p_, "b_", "ms_per_call")
        t, s = pick(p_, "t_", "ms_per_call"), pick(p_, "s_", "ms_per_call")
        d, e = pick(t_, "d_", "ns_per_entry"), pick(p_, "e_", "ns_per_entry")
        p, q = pick(p_, "p_", "ns_per_pair"), pick(p_, "q_", "ns_per_pair")
        gate.append(dict(run=run, a_batch_600_ms=a, b_parent_sequential_600_ms=b, b_over_a=b / a, t_parent_unweighted_batch_600_ms=t,
                         s_parent_unweighted_sequential_600_ms=s, s_over_t=s / t, call_gate_b_over_a_at_least=0.5 * s / t,
                         call_gate="passes" if b / a >= 0.5 * s / t else "missed",
                         d_weighted_grid_ns_per_entry=d, e_parent_unweighted_grid_ns_per_entry=e, d_over_e=d / e,
                         p_parent_all_pairs_weighted_ns_per_pair=p, q_parent_all_pairs_ns_per_pair=q, p_over_q=p / q,
                         kernel_gate_d_over_e_at_most=1.15 * p / q, kernel_gate="passes" if d / e <= 1.15 * p / q else "missed"))
    json.dump(dict(what="scripts/bench_weighted_transforms.py on one MI355X (--summarise; see its docstring for every field): 20 + 20 "
                        "views of 1024^2, 768^2 bins, POLYNOMIAL, fixed radius, K = 600; (p), (q) at 400 views; median of 5 windows "
                        ">= 0.3 s with min / max; the parent revision's library (%s) and this revision's alternated in one job." % parent,
                   gate=gate, bench_py=dict(order=["parent", "this", "parent", "this"], evaluations_per_s=[b["value"] for b in bench],
                                            ms_per_step=[b.get("ms_per_step") for b in bench]), lines=rows), sys.stdout, indent=1)
    print()
    sys.exit(0)

if args.lib:
    os.environ["ECC_HIP_LIB"] = os.path.abspath(args.lib)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epipolarconsistency_amd import _lib  # noqa: E402
with open(_lib.LIB_PATH, "rb") as f:  # (looked up in the file: the package loads the library itself, after torch's runtime)
    HAVE_CALL = b"ecc_metric_evaluate_weighted_transforms" in f.read()
if not HAVE_CALL:  # the parent's build: the legs that exist there
    _lib.SIGNATURES.pop("ecc_metric_evaluate_weighted_transforms", None)
import epipolarconsistency_amd as E  # noqa: E402
from epipolarconsistency_amd import geometry, synthetic  # noqa: E402

ctx = E.Context(0)
ctx.enable_timing(True)
rng = np.random.default_rng(7)
S, ns, nt, K = 1024, args.source, args.target, args.K
n, count = ns + nt, ns * nt
pool = [E.RadonIntermediate.from_host(ctx, rng.standard_normal((args.bins, args.bins)).astype(np.float32), S, S) for _ in range(11)]
wpool = [E.RadonIntermediate.from_host(ctx, rng.random((args.bins, args.bins)).astype(np.float32), S, S, filter=E.FILTER_NONE) for _ in range(11)]
rec = dict(n_source=ns, n_target=nt, bins=args.bins, lib=args.tag or (args.lib or "this"))


def dealt(views):
    """the data, then the weights: neighbouring views on different arrays (scripts/bench_weighted.py)"""
    return [pool[v % len(pool)] for v in range(views)], [wpool[(v + 3) % len(wpool)] for v in range(views)]


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


if set(args.legs) & set("abtsdex"):
    Ps = synthetic.short_scan(n, S, S, 0.308)
    radius = args.radius if args.radius > 0 else float(E.host_object_radius(Ps[0], S, S))
    rec.update(radius_mm=radius, transforms=K, entries=count * K)
    data, weights = dealt(n)
    Ts = np.stack([geometry.rigid_transform(tx=0.05 * k, ty=-0.02 * (k % 7), tz=0.01 * (k % 5), rz=1e-4 * k, rx=5e-5 * (k % 3)) for k in range(K)])
    composed = [E.pack_projection_matrices([geometry.compose_transform(P, T) for P in Ps[:ns]] + list(Ps[ns:])) for T in Ts]
    P0 = E.pack_projection_matrices(Ps)
    j, i = np.divmod(np.arange(count), ns)
    idx = np.ascontiguousarray(np.stack([i, ns + j, i, ns + j], axis=1).astype(np.int32))
    mw = E.MetricRadonIntermediate(ctx, Ps, data + weights).setSampling("polynomial")
    mu = E.MetricRadonIntermediate(ctx, Ps, data).setSampling("polynomial")
    mw.setObjectRadius(radius)
    mu.setObjectRadius(radius)
    out = np.zeros(count, np.float32)

    def weighted_sequential():
        r = [mw.setProjectionMatrices(P).evaluate_weighted_pairs(idx) for P in composed]
        mw.setProjectionMatrices(P0)
        return r

    def unweighted_sequential():
        r = [mu.setProjectionMatrices(P).evaluate(idx, out) for P in composed]
        mu.setProjectionMatrices(P0)
        return r

    if HAVE_CALL and set(args.legs) & set("adx"):
        values, coverages = mw.evaluate_weighted_transforms(ns, Ts)
        assert np.all(np.isfinite(values)) and np.all((coverages > 0) & (coverages < 1)) and mw.last_batched_transforms() == K
        first = mw.setProjectionMatrices(composed[1]).evaluate_weighted_pairs(idx)
        mw.setProjectionMatrices(P0)
        assert (values[1], coverages[1]) == first, "the batch and the sequential step disagree"
        if "a" in args.legs:
            med, lo, hi, reps = windows(lambda: mw.evaluate_weighted_transforms(ns, Ts))
            print(json.dumps(dict(rec, leg="a_weighted_batch", ms_per_call=med, min=lo, max=hi, transforms_per_s=1e3 * K / med,
                                  calls_per_window=reps)), flush=True)
        if "d" in args.legs:
            med, lo, hi, reps = windows(lambda: mw.evaluate_weighted_transforms(ns, Ts), kernel=True)
            print(json.dumps(dict(rec, leg="d_weighted_grid_pair_launch", kernel_ms=med, min=lo, max=hi, ns_per_entry=1e6 * med / (count * K),
                                  calls_per_window=reps)), flush=True)
        if "x" in args.legs:
            for _ in range(10):
                mw.evaluate_weighted_transforms(ns, Ts)
            print(json.dumps(dict(rec, leg="x_calls_for_a_kernel_trace", calls=10)), flush=True)
    if "b" in args.legs:
        med, lo, hi, reps = windows(weighted_sequential)
        print(json.dumps(dict(rec, leg="b_weighted_sequential", ms_per_call=med, min=lo, max=hi, transforms_per_s=1e3 * K / med,
                              calls_per_window=reps)), flush=True)
    if "t" in args.legs:
        med, lo, hi, reps = windows(lambda: mu.evaluate_transforms(ns, Ts))
        print(json.dumps(dict(rec, leg="t_unweighted_batch", ms_per_call=med, min=lo, max=hi, transforms_per_s=1e3 * K / med,
                              calls_per_window=reps)), flush=True)
    if "e" in args.legs:
        med, lo, hi, reps = windows(lambda: mu.evaluate_transforms(ns, Ts), kernel=True)
        print(json.dumps(dict(rec, leg="e_unweighted_grid_pair_launch", kernel_ms=med, min=lo, max=hi, ns_per_entry=1e6 * med / (count * K),
                              calls_per_window=reps)), flush=True)
    if "s" in args.legs:
        med, lo, hi, reps = windows(unweighted_sequential)
        print(json.dumps(dict(rec, leg="s_unweighted_sequential", ms_per_call=med, min=lo, max=hi, transforms_per_s=1e3 * K / med,
                              calls_per_window=reps)), flush=True)
    mw.close()
    mu.close()

if set(args.legs) & set("pq"):
    N = args.views
    Ps = synthetic.short_scan(N, S, S, 0.308)
    data, weights = dealt(N)
    n_pairs = N * (N - 1) // 2
    if "p" in args.legs:
        m = E.MetricRadonIntermediate(ctx, Ps, data + weights).setSampling("polynomial")
        med, lo, hi, reps = windows(m.evaluate_weighted, kernel=True)
        print(json.dumps(dict(rec, leg="p_all_pairs_weighted_kernel", views=N, kernel_ms=med, min=lo, max=hi, pairs=n_pairs,
                              ns_per_pair=1e6 * med / n_pairs, calls_per_window=reps)), flush=True)
        m.close()
    if "q" in args.legs:
        m = E.MetricRadonIntermediate(ctx, Ps, data).setSampling("polynomial")
        med, lo, hi, reps = windows(m.evaluate, kernel=True)
        print(json.dumps(dict(rec, leg="q_all_pairs_kernel", views=N, kernel_ms=med, min=lo, max=hi, pairs=n_pairs,
                              ns_per_pair=1e6 * med / n_pairs, calls_per_window=reps)), flush=True)
        m.close()
