#!/usr/bin/env python3
"""Microseconds per finite-difference gradient of one view (GPU box):
    python scripts/bench_gradient.py [--lib PATH] [--legs abc] [--sizes 400,64,258] [--bins 768] [--view -1]
(a) ecc_metric_evaluate_gradient with ecc_debug_set_gradient_launch(m, 1) (csrc/ecc_gradient.hip, csrc/small_poses_kernel.hip): the
    metric and the twelve probes of six rigid parameters in one call; the path of every call is checked to be 2 (the probes' own
    launch).  Without the switch the call is leg (b) plus one pose that moves nothing;
(b) ecc_metric_evaluate_pose_deltas with the same twelve probes -- the call a caller without (a) makes.  It exists on older
    revisions too: --lib PATH loads another build of the library (one made from the parent revision), where only --legs bc run.
    THE YARDSTICK for (a) is (b) on the parent revision; (b) on both revisions shows that the existing path was left alone;
(c) twelve sequential steps of the pose-delta mode (setIncremental: setProjectionMatrices + evaluate per probe), for scale.
Every shape is warmed up; the figure is the median of --windows windows of at least --min-seconds each, with the spread
(min .. max) beside it.  Run the builds alternately inside one job (parent, this, parent, this).  One JSON line per (views, leg).
--once: one call of leg (a) per size and nothing else (for a kernel trace)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default="")
ap.add_argument("--legs", default="abc")
ap.add_argument("--sizes", default="400,64,258")
ap.add_argument("--bins", type=int, default=768)
ap.add_argument("--view", type=int, default=-1, help="the moved view; -1: the middle one")
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--min-seconds", type=float, default=0.3)
ap.add_argument("--tag", default="")
ap.add_argument("--once", action="store_true")
args = ap.parse_args()
if args.lib:
    os.environ["ECC_HIP_LIB"] = os.path.abspath(args.lib)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epipolarconsistency_amd import _lib  # noqa: E402
with open(_lib.LIB_PATH, "rb") as f:  # (looked up in the file: the package loads the library itself, after torch's runtime)
    HAVE_GRADIENT = b"ecc_metric_evaluate_gradient" in f.read()
if not HAVE_GRADIENT:  # an older build: the calls of legs (b) and (c) only
    for name in ("ecc_metric_evaluate_gradient", "ecc_metric_last_gradient_path", "ecc_debug_set_gradient_launch"):
        _lib.SIGNATURES.pop(name, None)
import epipolarconsistency_amd as E  # noqa: E402
from epipolarconsistency_amd import geometry, synthetic  # noqa: E402

STEPS = np.array([0.5, 0.5, 0.5, np.deg2rad(0.1), np.deg2rad(0.1), np.deg2rad(0.1)])
NAMES = ("tx", "ty", "tz", "rx", "ry", "rz")
ctx = E.Context(0)
rng = np.random.default_rng(7)
S = 1024
pool = [E.RadonIntermediate.from_host(ctx, rng.standard_normal((args.bins, args.bins)).astype(np.float32), S, S) for _ in range(8)]


def windows(fn):
    fn()  # warm-up of this shape
    fn()
    t0 = time.perf_counter()
    fn()
    reps = max(1, int(np.ceil(args.min_seconds / max(time.perf_counter() - t0, 1e-6))))
    us = []
    for _ in range(args.windows):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        us.append(1e6 * (time.perf_counter() - t0) / reps)
    return float(np.median(us)), float(min(us)), float(max(us)), reps


for n in [int(x) for x in args.sizes.split(",")]:
    view = n // 2 if args.view < 0 else args.view
    Ps = synthetic.short_scan(n, S, S, 0.308)
    P0 = E.pack_projection_matrices(Ps)
    dtrs = [pool[v % len(pool)] for v in range(n)]
    P34 = np.asarray(Ps[view], np.float64)
    rows = E.pack_projection_matrices([geometry.compose_transform(P34, geometry.rigid_transform(**{NAMES[k]: s * STEPS[k]}))
                                       for k in range(6) for s in (1.0, -1.0)])
    plus, minus = np.ascontiguousarray(rows[0::2]), np.ascontiguousarray(rows[1::2])
    off, views = np.arange(13, dtype=np.int32), np.full(12, view, np.int32)
    m = E.MetricRadonIntermediate(ctx, Ps, dtrs)
    if HAVE_GRADIENT:
        m.debugSetGradientLaunch(True)   # leg (a) is the probes' own launch (opt-in); legs (b), (c) do not go through it
    rec = dict(views=n, view=view, bins=args.bins, lib=args.tag or (args.lib or "this"), probes=12)
    if args.once:
        m.evaluate_gradient(view, plus, minus, STEPS)
        m.evaluate_gradient(view, plus, minus, STEPS)
        m.close()
        continue
    want = m.evaluate_pose_deltas_packed(off, views, rows)
    if "a" in args.legs and HAVE_GRADIENT:
        value, grad, probes = m.evaluate_gradient(view, plus, minus, STEPS, want_probes=True)
        assert m.last_gradient_path() == 2 and np.array_equal(probes, want)
        med, lo, hi, reps = windows(lambda: m.evaluate_gradient(view, plus, minus, STEPS))
        assert m.last_gradient_path() == 2
        print(json.dumps(dict(rec, leg="a_gradient", us_per_call=med, min=lo, max=hi, calls_per_window=reps)), flush=True)
    if "b" in args.legs:
        med, lo, hi, reps = windows(lambda: m.evaluate_pose_deltas_packed(off, views, rows))
        assert m.last_batched_poses() == 12
        print(json.dumps(dict(rec, leg="b_pose_deltas", us_per_call=med, min=lo, max=hi, calls_per_window=reps)), flush=True)
    if "c" in args.legs:
        inc = E.MetricRadonIntermediate(ctx, Ps, dtrs).setIncremental(True)
        poses = []
        for row in rows:
            P = P0.copy()
            P[view] = row
            poses.append(P)

        def loop():
            for P in poses:
                inc.setProjectionMatrices(P).evaluate()
        loop()
        assert np.array_equal(np.array([inc.setProjectionMatrices(P).evaluate() for P in poses]), want)
        med, lo, hi, reps = windows(loop)
        print(json.dumps(dict(rec, leg="c_sequential_steps", us_per_call=med, min=lo, max=hi, calls_per_window=reps)), flush=True)
        inc.close()
    m.close()
