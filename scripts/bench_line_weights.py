#!/usr/bin/env python3
"""Milliseconds per stack of line weights: the device path against the host round trip it replaces and the Radon floor (GPU box):
    python scripts/bench_line_weights.py [--lib PATH] [--legs abc] [--images 16] [--size 1024] [--bins 768] [--tag NAME]
    python scripts/bench_line_weights.py --summarise LINES.jsonl BENCH.jsonl PARENT_REVISION > profiles/line_weights_1gpu.json
16 flagged images of 1024^2 (instrument-like blocks and a blade at an edge), 768^2 bins, zero_at_px = 1, guard_bins = 1, dilate_px = 3.
(a) line_weights on the stack dilated in numpy OUTSIDE the timed window: Radon kernel, 16 readbacks, numpy clip and minimum, 16
    uploads -- exists on the parent revision too (--lib PATH loads another build, where (c) does not run);
(b) RadonIntermediate.compute_batch(FILTER_NONE) of the dilated stack from a device tensor: the floor both paths share;
(c) line_weights_device from the device-resident flagged stack: dilation, Radon kernel, clip + minimum, slabs written completely.
    THE GATE: (c) <= 1.10 x (b), (b) of the parent.  (a) / (c) is recorded.
(x) nothing timed here: ten calls of (c)'s shape for a kernel trace, which gives the two new kernels' times per launch.
Every call ends in a synchronise (the handles are closed inside the window, which drains the stream); every shape is warmed up; a
figure is the median of --windows windows of at least --min-seconds each, with min and max beside it.  Run the builds alternately
inside one job (--tag parent_run1, this_run1, ...).  One JSON line per leg."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default="")
ap.add_argument("--legs", default="abc")
ap.add_argument("--images", type=int, default=16)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--bins", type=int, default=768)
ap.add_argument("--dilate", type=int, default=3)
ap.add_argument("--guard", type=int, default=1)
ap.add_argument("--zero-at", type=float, default=1.0)
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
        return [r for r in rows if r["lib"] == tag and r["leg"].startswith(leg)][0]["ms_per_stack"]
    gate = []
    for run in (1, 2):
        t_, p_ = "this_run%d" % run, "parent_run%d" % run
        a, b, c = pick(p_, "a_"), pick(p_, "b_"), pick(t_, "c_")
        gate.append(dict(run=run, a_parent_line_weights_ms=a, b_parent_radon_floor_ms=b, c_line_weights_device_ms=c, c_over_b=c / b,
                         gate_c_over_b_at_most=1.10, gate="passes" if c <= 1.10 * b else "missed", a_over_c=a / c,
                         b_this_radon_floor_ms=pick(t_, "b_"), a_this_line_weights_ms=pick(t_, "a_")))
    json.dump(dict(what="scripts/bench_line_weights.py on one MI355X (--summarise; see its docstring for every field): 16 flagged images "
                        "of 1024^2, 768^2 bins, zero_at_px 1, guard_bins 1, dilate_px 3; ms per stack, median of 5 windows >= 0.3 s with "
                        "min / max; the parent revision's library (%s) and this revision's alternated in one job." % parent,
                   gate=gate, bench_py=dict(order=["parent", "this", "parent", "this"], evaluations_per_s=[b["value"] for b in bench],
                                            ms_per_step=[b.get("ms_per_step") for b in bench]), lines=rows), sys.stdout, indent=1)
    print()
    sys.exit(0)

if args.lib:
    os.environ["ECC_HIP_LIB"] = os.path.abspath(args.lib)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epipolarconsistency_amd import _lib  # noqa: E402
NEW = ("ecc_line_weights_defaults", "ecc_radon_line_weights", "ecc_radon_line_weights_into", "ecc_dtr_line_weights")
with open(_lib.LIB_PATH, "rb") as f:  # (looked up in the file: the package loads the library itself, after torch's runtime)
    HAVE_CALL = NEW[1].encode() in f.read()
if not HAVE_CALL:  # the parent's build: the legs that exist there
    for name in NEW:
        _lib.SIGNATURES.pop(name, None)
import torch  # noqa: E402
import epipolarconsistency_amd as E  # noqa: E402

ctx = E.Context(0)
n, S, B, R = args.images, args.size, args.bins, args.dilate
rng = np.random.default_rng(7)
flagged = np.zeros((n, S, S), np.float32)
for k in range(n):  # an instrument somewhere in the view, a second piece, and in every other view a blade along an edge
    for _ in range(2):
        y, x, h, w = rng.integers(0, S - 200), rng.integers(0, S - 200), rng.integers(20, 200), rng.integers(20, 200)
        flagged[k, y:y + h, x:x + w] = 1.0
    if k % 2:
        flagged[k, :, :int(rng.integers(4, 40))] = 1.0


def dilate(f, r):
    p = np.pad(f, ((0, 0), (r, r), (r, r)), mode="edge")
    out = f.copy()
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            np.maximum(out, p[:, dy:dy + S, dx:dx + S], out=out)
    return out


dilated = dilate(flagged, R) if R else flagged.copy()
flagged_t, dilated_t = torch.from_numpy(flagged).cuda(), torch.from_numpy(dilated).cuda()
rec = dict(images=n, size=S, bins=B, zero_at_px=args.zero_at, guard_bins=args.guard, dilate_px=R, lib=args.tag or (args.lib or "this"))


def close(dtrs):
    for d in dtrs:
        d.close()
    ctx.synchronize()


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
        ctx.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / reps)
    return float(np.median(ms)), float(min(ms)), float(max(ms)), reps


def report(leg, fn):
    med, lo, hi, reps = windows(fn)
    print(json.dumps(dict(rec, leg=leg, ms_per_stack=med, min=lo, max=hi, ms_per_image=med / n, calls_per_window=reps)), flush=True)


if HAVE_CALL and set(args.legs) & set("cx"):  # the two paths agree before either is timed
    dev = E.line_weights_device(ctx, flagged_t[:2], B, B, args.zero_at, args.guard, R)
    host = E.line_weights(ctx, dilated[:2], B, B, args.zero_at, args.guard)
    for d, h in zip(dev, host):
        assert np.array_equal(d.readback().view(np.uint32), h.readback().view(np.uint32)), "the device path and line_weights disagree"
    close(dev + host)
if "a" in args.legs:
    report("a_line_weights_host_round_trip", lambda: close(E.line_weights(ctx, dilated, B, B, args.zero_at, args.guard)))
if "b" in args.legs:
    report("b_radon_floor_compute_batch", lambda: close(E.RadonIntermediate.compute_batch(ctx, dilated_t, B, B, E.FILTER_NONE)))
if HAVE_CALL and "c" in args.legs:
    report("c_line_weights_device", lambda: close(E.line_weights_device(ctx, flagged_t, B, B, args.zero_at, args.guard, R)))
if HAVE_CALL and "x" in args.legs:
    for _ in range(10):
        close(E.line_weights_device(ctx, flagged_t, B, B, args.zero_at, args.guard, R))
    print(json.dumps(dict(rec, leg="x_calls_for_a_kernel_trace", calls=10)), flush=True)
ctx.close()
