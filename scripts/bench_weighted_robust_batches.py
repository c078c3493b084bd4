#!/usr/bin/env python3
"""Rates of ecc_metric_evaluate_weighted_robust_pose_deltas / ecc_metric_evaluate_weighted_robust_transforms against the sequential
steps they replace (GPU box), in the manner of scripts/bench_robust_batches.py:
    python scripts/bench_weighted_robust_batches.py [--legs psPSbwectq] [--views 400] [--bins 768] [--K 600] [--loss 0] [--commit REVISION]
1024^2 detector, POLYNOMIAL sampling, 2 n intermediates: the data of every view, then line weights made on the device from a flagged
block near a corner of the detector (its size differs from view to view); delta = weighted_robust_scale(the base's rows
at delta = inf, 0.5); Huber by default.
Pose deltas: --views views (400), view views // 2 swept over the six rigid parameters, K / 6 steps each (the 6-DoF sweep of bench.py):
(p) the K poses through evaluate_weighted_robust_pose_deltas, wall clock per call (with the pair launch's HIP-event time);
(s) the same K as setProjectionMatrices + evaluate_weighted_robust each, then the base again;
(P) the 12 probes of a central-difference gradient (the first and last step of each parameter) through the call, and
(S) the same 12 the sequential way;
(b) evaluate_weighted_robust at the base alone: what the base columns of (p) and (P) cost per call;
(w) the same K poses through evaluate_weighted_pose_deltas, and (e), (c) evaluate_weighted / evaluate_weighted_robust at the base: (p) is
    held against (w) times the ratio (c) / (e).
Transforms: --source + --target views (20 + 20), the object radius fixed at the automatic radius of the base's first view:
(t) K transforms through evaluate_weighted_robust_transforms; (q) the same K as setProjectionMatrices(composed) +
evaluate_weighted_robust_pairs(cross list).
Every leg checks first that the batch and the sequential step agree bit for bit on a few items.  Every shape is warmed up twice; a
figure is the median of --windows windows of at least --min-seconds each, with min and max beside it; socket power and engine clock
are read from the card's hwmon files (read-only) every 20 ms while a leg's windows run, their means printed with the leg (null: the
card's files were not found).  One JSON line per leg, also appended to --out (profiles/weighted_robust_batches_1gpu.jsonl)."""
import argparse
import glob
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="psPSbwectq")
ap.add_argument("--views", type=int, default=400)
ap.add_argument("--source", type=int, default=20)
ap.add_argument("--target", type=int, default=20)
ap.add_argument("--bins", type=int, default=768)
ap.add_argument("--K", type=int, default=600)
ap.add_argument("--loss", type=int, default=0)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--min-seconds", type=float, default=0.5)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_robust_batches_1gpu.jsonl"))
args = ap.parse_args()

sys.path.insert(0, ROOT)
import epipolarconsistency_amd as E  # noqa: E402
from epipolarconsistency_amd import geometry, synthetic  # noqa: E402

ctx = E.Context(0)
ctx.enable_timing(True)
rng = np.random.default_rng(7)
S, K, LOSS, INF = 1024, args.K, args.loss, float("inf")
pool = [E.RadonIntermediate.from_host(ctx, rng.standard_normal((args.bins, args.bins)).astype(np.float32), S, S) for _ in range(11)]
flagged = np.zeros((11, S, S), np.float32)
for q in range(11):
    flagged[q, 64:64 + 96 + 8 * q, 32:32 + 96 + 8 * q] = 1.0     # a block of 96 .. 176 pixels near a corner
wpool = E.line_weights_device(ctx, flagged, args.bins, args.bins)
rec = dict(bins=args.bins, loss=LOSS, commit=args.commit)

# the hwmon files of the card this process runs on (by its PCI address; a one-GPU box shows its own card's only)
HW = [d for d in sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*")) if os.path.exists(d + "/power1_input") and os.path.exists(d + "/freq1_input")]
try:
    import torch
    pr = torch.cuda.get_device_properties(0)
    pci = "%04x:%02x" % (pr.pci_domain_id, pr.pci_bus_id)
    mine = [d for d in HW if pci in os.path.realpath(os.path.dirname(os.path.dirname(d)))]
except Exception:
    mine = []
HW = mine if mine else (HW if len(HW) == 1 else [])
rec["hwmon"] = HW[0] if HW else None


def windows(fn):
    """median, min, max of the windows' ms per call; calls per window; mean socket watts and engine MHz while they ran"""
    fn()  # warm-up of this shape
    fn()
    t0 = time.perf_counter()
    fn()
    reps = max(1, int(np.ceil(args.min_seconds / max(time.perf_counter() - t0, 1e-6))))
    samples, stop = [], [False]

    def sampler():
        while not stop[0]:
            try:
                samples.append((float(open(HW[0] + "/power1_input").read()) * 1e-6, float(open(HW[0] + "/freq1_input").read()) * 1e-6))
            except Exception:
                pass
            time.sleep(0.02)
    th = threading.Thread(target=sampler)
    if HW:
        th.start()
    ms = []
    for _ in range(args.windows):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()    # (every call here returns with its results on the host: the clock stops behind the device)
        ms.append(1e3 * (time.perf_counter() - t0) / reps)
    stop[0] = True
    if HW:
        th.join()
    state = dict(watts=float(np.mean([p for p, f in samples])), sclk_mhz=float(np.mean([f for p, f in samples]))) if samples else \
        dict(watts=None, sclk_mhz=None)
    return dict(ms_per_call=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)), calls_per_window=reps, **state)


def report(leg, items, w, **more):
    line = json.dumps(dict(rec, leg=leg, items=items, items_per_s=1e3 * items / w["ms_per_call"], **w, **more))
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


def same(x, y):
    return np.float64(x).tobytes() == np.float64(y).tobytes()


if set(args.legs) & set("psPSbwec"):
    n = args.views
    Ps = synthetic.short_scan(n, S, S, 0.308)
    P0 = E.pack_projection_matrices(Ps)
    dtrs = [pool[v % len(pool)] for v in range(n)] + [wpool[v % len(wpool)] for v in range(n)]
    m = E.MetricRadonIntermediate(ctx, Ps, dtrs).setSampling("polynomial")
    delta = float(np.float32(E.weighted_robust_scale(m.evaluate_weighted_robust(LOSS, INF, want_pairs=True)[3], 0.5)))
    v, steps = n // 2, K // 6
    names = ("tx", "ty", "tz", "rx", "ry", "rz")
    rows = []
    for a, name in enumerate(names):
        for k in range(steps):
            amount = (k - steps // 2 + 0.5) * (0.02 if a < 3 else 2e-5)
            rows.append((P0[v].reshape(4, 3).T @ geometry.rigid_transform(**{name: amount})).T.reshape(12))
    rows = np.stack(rows)
    Kp = len(rows)
    off, views = np.arange(Kp + 1, dtype=np.int32), np.full(Kp, v, np.int32)
    probes = np.array([a * steps + k for a in range(6) for k in (0, steps - 1)])
    full = P0.copy()

    def sequential(which):
        out = []
        for k in which:
            full[v] = rows[k]
            out.append(m.setProjectionMatrices(full).evaluate_weighted_robust(LOSS, delta))
        full[v] = P0[v]
        m.setProjectionMatrices(P0)
        return out

    for _ in range(3):   # (the third call is warm: its pair launch's event time is reported)
        values, coverages, masses = m.evaluate_weighted_robust_pose_deltas_packed(off, views, rows, LOSS, delta)
    pair_ms = ctx.last_kernel_ms("pairs")     # the batch's pair launch over the n x K grid (the last pair launch of the call)
    assert m.last_batched_poses() == Kp and np.all((masses > 0) & (masses < 1)) and np.all((coverages > 0) & (coverages < 1))
    for k, (val, cov, mass) in zip(probes, sequential(probes)):
        assert same(values[k], val) and same(coverages[k], cov) and same(masses[k], mass), "the batch and the sequential step disagree"
    rec_p = dict(views=n, pairs=n * (n - 1) // 2, moved_view=v, delta=delta, coverage=float(coverages.mean()), inlier_mass=float(masses.mean()))
    if "p" in args.legs:
        report("p_weighted_robust_pose_deltas", Kp, windows(lambda: m.evaluate_weighted_robust_pose_deltas_packed(off, views, rows, LOSS, delta)),
               batch_pair_launch_ms=pair_ms, **rec_p)
    if "s" in args.legs:
        report("s_sequential_poses", Kp, windows(lambda: sequential(range(Kp))), **rec_p)
    if "P" in args.legs:
        o12, v12, r12 = np.arange(13, dtype=np.int32), views[:12], np.ascontiguousarray(rows[probes])
        report("P_weighted_robust_pose_deltas_12", 12, windows(lambda: m.evaluate_weighted_robust_pose_deltas_packed(o12, v12, r12, LOSS, delta)), **rec_p)
    if "S" in args.legs:
        report("S_sequential_poses_12", 12, windows(lambda: sequential(probes)), **rec_p)
    if "b" in args.legs:
        report("b_evaluate_weighted_robust_at_the_base", 1, windows(lambda: m.evaluate_weighted_robust(LOSS, delta)), **rec_p)
    if "w" in args.legs:
        report("w_weighted_pose_deltas", Kp, windows(lambda: m.evaluate_weighted_pose_deltas_packed(off, views, rows)), **rec_p)
    if "e" in args.legs:
        report("e_evaluate_weighted_at_the_base", 1, windows(m.evaluate_weighted), **rec_p)
    if "c" in args.legs:
        report("c_evaluate_weighted_robust_at_the_base", 1, windows(lambda: m.evaluate_weighted_robust(LOSS, delta)), **rec_p)
    m.close()

if set(args.legs) & set("tq"):
    ns, nt = args.source, args.target
    n, count = ns + nt, ns * nt
    Ps = synthetic.short_scan(n, S, S, 0.308)
    P0 = E.pack_projection_matrices(Ps)
    radius = float(E.host_object_radius(Ps[0], S, S))
    dtrs = [pool[v % len(pool)] for v in range(n)] + [wpool[v % len(wpool)] for v in range(n)]
    m = E.MetricRadonIntermediate(ctx, Ps, dtrs).setSampling("polynomial")
    m.setObjectRadius(radius)
    Ts = np.stack([geometry.rigid_transform(tx=0.05 * k, ty=-0.02 * (k % 7), tz=0.01 * (k % 5), rz=1e-4 * k, rx=5e-5 * (k % 3)) for k in range(K)])
    composed = [E.pack_projection_matrices([geometry.compose_transform(P, T) for P in Ps[:ns]] + list(Ps[ns:])) for T in Ts]
    j, i = np.divmod(np.arange(count), ns)
    idx = np.ascontiguousarray(np.stack([i, ns + j, i, ns + j], axis=1).astype(np.int32))
    delta = float(np.float32(E.weighted_robust_scale(m.evaluate_weighted_robust_pairs(idx, LOSS, INF, want_pairs=True)[3], 0.5)))

    def sequential():
        out = [m.setProjectionMatrices(P).evaluate_weighted_robust_pairs(idx, LOSS, delta) for P in composed]
        m.setProjectionMatrices(P0)
        return out

    for _ in range(3):
        values, coverages, masses = m.evaluate_weighted_robust_transforms(ns, Ts, LOSS, delta)
    pair_ms = ctx.last_kernel_ms("pairs")
    assert m.last_batched_transforms() == K and np.all((masses > 0) & (masses < 1)) and np.all((coverages > 0) & (coverages < 1))
    for k in (0, 1, K - 1):
        val, cov, mass = m.setProjectionMatrices(composed[k]).evaluate_weighted_robust_pairs(idx, LOSS, delta)
        assert same(values[k], val) and same(coverages[k], cov) and same(masses[k], mass), "the batch and the sequential step disagree"
    m.setProjectionMatrices(P0)
    rec_t = dict(n_source=ns, n_target=nt, entries=count * K, radius_mm=radius, delta=delta, coverage=float(coverages.mean()),
                 inlier_mass=float(masses.mean()))
    if "t" in args.legs:
        report("t_weighted_robust_transforms", K, windows(lambda: m.evaluate_weighted_robust_transforms(ns, Ts, LOSS, delta)),
               batch_pair_launch_ms=pair_ms, **rec_t)
    if "q" in args.legs:
        report("q_sequential_transforms", K, windows(sequential), **rec_t)
    m.close()
