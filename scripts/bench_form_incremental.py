#!/usr/bin/env python3
"""Milliseconds per optimiser step with and without kept base columns (ecc_metric_set_form_incremental; GPU box):
    python scripts/bench_form_incremental.py [--lib PATH] [--mode off|on] [--views 400] [--bins 768] [--tag NAME]
    python scripts/bench_form_incremental.py --summarise LINES.jsonl
One step is what a pose optimiser does per iteration: setProjectionMatrices with ONE view changed, then a 12-probe
evaluate_robust_pose_deltas of that view (leg r) -- and the same with evaluate_variance_robust_pose_deltas on the 2 n metric (leg v).
400 views of 1024^2, 768^2 bins, POLYNOMIAL.  The views walk through the scan (never view 0: the automatic object radius follows it),
and a view's matrix alternates between two perturbations, so every step really changes one view.  Wall clock per step, the median of
--windows windows of at least --min-seconds each, with the spread (min .. max) beside it.
Three legs, one process each, alternated in one job (parent, off, on, parent, off, on; --tag parent_run1, off_run1, ...):
    --lib PARENT.so                 the parent revision's library (it has no switch: the mode is off)
    --mode off                      this build, the mode off
    --mode on                       this build, the mode on; before timing, one step's results are compared bit for bit with a
                                    mode-off metric's, and the counter must read n - 1 after a step
One JSON line per (leg, form).  --summarise: per form and run whether the mode-off windows overlap the parent's and whether the
mode-on windows lie wholly below the mode-off ones, and the ratio of the medians."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default="")
ap.add_argument("--mode", default="off", choices=("off", "on"))
ap.add_argument("--forms", default="rv")
ap.add_argument("--views", type=int, default=400)
ap.add_argument("--bins", type=int, default=768)
ap.add_argument("--probes", type=int, default=12)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--min-seconds", type=float, default=0.3)
ap.add_argument("--floor", type=float, default=1.5)
ap.add_argument("--tag", default="")
ap.add_argument("--summarise", metavar="LINES")
args = ap.parse_args()

if args.summarise:
    rows = [json.loads(l) for l in open(args.summarise) if l.strip().startswith("{")]
    out = []
    for form in sorted({r["form"] for r in rows}):
        for run in sorted({r["lib"].rsplit("_run", 1)[1] for r in rows if "_run" in r["lib"]}):
            def pick(leg):
                return [r for r in rows if r["form"] == form and r["lib"] == "%s_run%s" % (leg, run)][0]
            p, off, on = pick("parent"), pick("off"), pick("on")
            out.append(dict(form=form, run=int(run), parent_ms=p["ms_per_step"], off_ms=off["ms_per_step"], on_ms=on["ms_per_step"],
                            off_overlaps_parent=bool(off["min"] <= p["max"] and p["min"] <= off["max"]),
                            on_wholly_below_off=bool(on["max"] < off["min"]), on_over_off=on["ms_per_step"] / off["ms_per_step"]))
    json.dump(dict(what="scripts/bench_form_incremental.py on one MI355X (--summarise; see its docstring): ms per step = one view set + a "
                        "12-probe pose-delta call; median of 5 windows >= 0.3 s with min / max; parent, mode off, mode on alternated in one job.",
                   conditions=out, lines=rows), sys.stdout, indent=1)
    print()
    sys.exit(0)

if args.lib:
    os.environ["ECC_HIP_LIB"] = os.path.abspath(args.lib)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epipolarconsistency_amd import _lib  # noqa: E402
with open(_lib.LIB_PATH, "rb") as f:  # (looked up in the file: the package loads the library itself, after torch's runtime)
    HAVE_MODE = b"ecc_metric_set_form_incremental" in f.read()
if not HAVE_MODE:  # the parent's build
    assert args.mode == "off", "this library has no ecc_metric_set_form_incremental"
    for name in ("ecc_metric_set_form_incremental", "ecc_metric_last_form_base_pairs"):
        _lib.SIGNATURES.pop(name, None)
import epipolarconsistency_amd as E  # noqa: E402
from epipolarconsistency_amd import synthetic  # noqa: E402

ctx = E.Context(0)
rng = np.random.default_rng(7)
S, n, Q = 1024, args.views, args.probes
LOSS, INF = E.LOSS_TRUNCATED, float("inf")
pool = [E.RadonIntermediate.from_host(ctx, rng.standard_normal((args.bins, args.bins)).astype(np.float32), S, S) for _ in range(11)]
vpool = [E.RadonIntermediate.from_host(ctx, (0.25 * 16.0 ** rng.random((args.bins, args.bins))).astype(np.float32), S, S, filter=E.FILTER_NONE)
         for _ in range(11)]
Ps = synthetic.short_scan(n, S, S, 0.308)
P0 = E.pack_projection_matrices(Ps)
data = [pool[v % len(pool)] for v in range(n)]
fields = [vpool[(v + 3) % len(vpool)] for v in range(n)]
rec = dict(views=n, bins=args.bins, probes=Q, mode=args.mode, lib=args.tag or (args.lib or "this"))


def moved(P12, k, v):
    T = E.geometry.rigid_transform(tx=0.11 * (k % 13 + 1), ty=-0.05 * (v % 5), rz=0.0015 * (k % 7 + 1), rx=0.0007 * (v % 3))
    return (P12.reshape(4, 3).T @ T).T.reshape(12)


# the walk: up to 48 different views, two matrices each (visited alternately), and the 12 probes around each of them
WALK = list(dict.fromkeys(1 + (7 * s) % (n - 1) for s in range(48)))
SET = {(v, alt): moved(P0[v], 3 + alt, v) for v in WALK for alt in (0, 1)}
PROBES = {key: np.ascontiguousarray(np.stack([moved(row, 20 + q, key[0]) for q in range(Q)])) for key, row in SET.items()}
OFF = np.arange(Q + 1, dtype=np.int32)
VIEWS = {v: np.full(Q, v, np.int32) for v in WALK}


def metric(form, mode):
    m = E.MetricRadonIntermediate(ctx, Ps, data + (fields if form == "v" else [])).setSampling("polynomial")
    if mode == "on":
        m.setFormIncremental(True)
    return m


def deltas(m, form):
    if form == "v":
        return float(np.float32(E.variance_robust_scale(m.evaluate_variance_robust(LOSS, INF, args.floor, want_pairs=True)[3], 2.0)))
    return float(np.float32(E.robust_scale(m.evaluate_robust(LOSS, INF, want_pairs=True)[2], 2.0)))


class Walk:
    """The optimiser's loop on one metric: step() sets the next view of the walk and probes it."""

    def __init__(self, m, form, delta):
        self.m, self.form, self.delta, self.P, self.s = m, form, delta, P0.copy(), 0

    def step(self):
        v = WALK[self.s % len(WALK)]
        key = (v, (self.s // len(WALK)) & 1)
        self.s += 1
        self.P[v] = SET[key]
        self.m.setProjectionMatrices(self.P)
        if self.form == "v":
            return self.m.evaluate_variance_robust_pose_deltas_packed(OFF, VIEWS[v], PROBES[key], LOSS, self.delta, args.floor)
        return self.m.evaluate_robust_pose_deltas_packed(OFF, VIEWS[v], PROBES[key], LOSS, self.delta)


def windows(fn):
    """(median, min, max, steps per window) of the wall-clock ms per step"""
    for _ in range(3):
        fn()  # warm-up of this shape (mode on: the first step is the miss)
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


for form in args.forms:
    m = metric(form, args.mode)
    delta = deltas(m, form)
    w = Walk(m, form, delta)
    first = w.step()
    assert m.last_batched_poses() == Q and np.all(np.isfinite(first[0])) and np.all((first[-1] > 0) & (first[-1] < 1))
    extra = {}
    if args.mode == "on":  # the same walk on a mode-off metric: the same bits, step by step; n - 1 base pairs per step after the first
        ref = metric(form, "off")
        r = Walk(ref, form, delta)
        got = [first] + [w.step() for _ in range(3)]
        want = [r.step() for _ in range(4)]
        for g, x in zip(got, want):
            assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(g, x))
        assert m.last_form_base_pairs() == n - 1 and ref.last_form_base_pairs() == n * (n - 1) // 2
        ref.close()
        for _ in range(2 * len(WALK)):  # two rounds of the walk: every step refreshes exactly one view
            w.step()
            assert m.last_form_base_pairs() == n - 1
        extra = dict(base_pairs_per_step=n - 1, bits_equal_mode_off=True)
    med, lo, hi, reps = windows(w.step)
    if args.mode == "on":
        assert m.last_form_base_pairs() == n - 1
    print(json.dumps(dict(rec, form="robust" if form == "r" else "variance_robust", ms_per_step=med, min=lo, max=hi, steps_per_window=reps,
                          delta=delta, **extra)), flush=True)
    m.close()
