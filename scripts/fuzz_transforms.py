#!/usr/bin/env python3
"""Randomised sweep of the batched registration (GPU box): python scripts/fuzz_transforms.py [cases] [seed]
csrc/ecc_transforms.hip against the sequential calls of the SAME library -- setProjectionMatrices(composed matrices) +
evaluate(index list) per transform -- the contract is bit identity of every mean and every pair value, so no tolerance: random
numbers of source and target views (1 ... 70 each: lists below and above the one-launch bound, the automatic mode's threshold,
every tail length), bin grids, sampling modes, automatic / fixed object radius, dkappa, use_corr, 1 ... 40 transforms (the identity,
rotations, translations that change the automatic radius, duplicates), with and without pair values, and ordinary evaluations
and parameter changes between the batches; the metric must be left as it was found.
ref for the pattern: tools/Registration/Registration3D3D.hxx:56-62, :91-110."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import epipolarconsistency_amd as E  # noqa: E402
from epipolarconsistency_amd import geometry, synthetic  # noqa: E402

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 6
rng = np.random.default_rng(seed)
ctx = E.Context(0)
bad = 0
t0 = time.time()


def eq(x, y):
    return x == y or (np.isnan(x) and np.isnan(y))


def cross_list(ns, nt):
    """entry q = j * ns + i -> (i, ns + j, i, ns + j), source index fast"""
    j, i = np.divmod(np.arange(ns * nt), ns)
    return np.ascontiguousarray(np.stack([i, ns + j, i, ns + j], axis=1).astype(np.int32))


sizes = [1, 2, 3, 4, 5, 7, 9, 13, 14, 20, 22, 23, 33, 47, 64, 70]
for c in range(cases):
    ns, nt = int(rng.choice(sizes)), int(rng.choice(sizes))
    n = ns + nt
    S = int(rng.choice([64, 96, 128]))
    Ba, Bt = int(rng.choice([32, 48, 64])), int(rng.choice([32, 48, 80]))
    Ps = synthetic.short_scan(n, S, S, 0.308 * 1024 / S, span_deg=float(rng.choice([200.0, 120.0, 360.0])))
    if rng.integers(0, 2):
        Ps = [P @ geometry.rigid_transform(*(rng.normal(0, 1.0, 3)), *(rng.normal(0, 0.01, 3))) for P in Ps]
    order = rng.permutation(n)  # source and target views interleaved along the trajectory
    Ps = [Ps[v] for v in order]
    pool = [E.RadonIntermediate.from_host(ctx, rng.standard_normal((Bt, Ba)).astype(np.float32), S, S) for _ in range(min(n, 6))]
    dtrs = [pool[v % len(pool)] for v in range(n)]
    mode = str(rng.choice(["auto", "polynomial", "per_sample", "reference"], p=[.4, .3, .2, .1]))
    if mode == "reference" and ns * nt > 2000:
        mode = "auto"
    radius = float(rng.choice([0.0, 0.0, 60.0, 110.0]))
    dkappa = float(rng.choice([0.0, 0.0, 0.0, 0.006]))
    corr = bool(rng.integers(0, 5) == 0)
    a = E.MetricRadonIntermediate(ctx, Ps, dtrs).setSampling(mode)
    b = E.MetricRadonIntermediate(ctx, Ps, dtrs).setSampling(mode)
    for m in (a, b):
        m.setObjectRadius(radius)
        m.setEpipolarPlaneStep(dkappa)
        m.useCorrelation(corr)
    if rng.integers(0, 4) == 0:
        a.setIncremental(True)
    idx = cross_list(ns, nt)
    ok, why = True, ""
    for rnd in range(int(rng.integers(1, 4))):
        K = int(rng.integers(1, 41 if ns * nt <= 1000 else 9))
        Ts = []
        for k in range(K):
            kind = rng.integers(0, 8)
            if kind == 0:
                T = np.eye(4)
            elif kind == 1 and Ts:
                T = Ts[int(rng.integers(0, len(Ts)))].copy()
            elif kind == 2:
                T = geometry.rigid_transform(rx=rng.normal(0, 0.02), ry=rng.normal(0, 0.02), rz=rng.normal(0, 0.02))
            elif kind == 3:
                T = geometry.rigid_transform(*(rng.normal(0, 8.0, 3)))
            else:
                T = geometry.rigid_transform(*(rng.normal(0, 2.0, 3)), *(rng.normal(0, 0.01, 3)))
            Ts.append(T)
        before = a.evaluate() if rng.integers(0, 2) else None
        want_m, want_p = np.zeros(K), np.zeros((K, nt, ns), np.float32)
        for k, T in enumerate(Ts):
            comp = [geometry.compose_transform(P, T) for P in Ps[:ns]] + list(Ps[ns:])
            out = np.zeros(ns * nt, np.float32)
            want_m[k] = b.setProjectionMatrices(comp).evaluate(idx, out)
            want_p[k] = out.reshape(nt, ns)
        if rng.integers(0, 2):
            got_m, got_p = a.evaluate_transforms(ns, Ts, want_pairs=True)
            same = np.array_equal(got_m, want_m, equal_nan=True) and np.array_equal(got_p, want_p, equal_nan=True)
        else:
            got_m = a.evaluate_transforms(ns, Ts)
            same = np.array_equal(got_m, want_m, equal_nan=True)
        batched = a.last_batched_transforms()
        if not same or batched != K:
            d = [int(q) for q in range(K) if not eq(got_m[q], want_m[q])]
            ok, why = False, "round %d K %d batched %d; transforms %s got %s want %s" % (
                rnd, K, batched, d[:4], [float(got_m[q]) for q in d[:4]], [float(want_m[q]) for q in d[:4]])
            break
        if before is not None:
            after = a.evaluate()
            if not eq(before, after):
                ok, why = False, "evaluate() before / after the batch: %r vs %r" % (before, after)
                break
        other = int(rng.integers(0, 3))
        if other == 0:
            x, y = a.evaluate(), b.setProjectionMatrices(Ps).evaluate()
            if not eq(x, y):
                ok, why = False, "evaluate after batch: %r vs %r" % (x, y)
        elif other == 1:
            radius2 = float(rng.choice([0.0, 75.0]))
            a.setObjectRadius(radius2)
            b.setObjectRadius(radius2)
        if not ok:
            break
    bad += 0 if ok else 1
    print("case %3d: %2d x %2d %3d^2 bins %dx%d %-10s r=%5.1f dk=%.3f corr %d: %s %s" % (c, ns, nt, S, Ba, Bt, mode, radius, dkappa, corr,
                                                                                    "ok" if ok else "MISMATCH", why), flush=True)
    a.close()
    b.close()
    for d in pool:
        d.close()
print("%d of %d cases differ, %.1f s" % (bad, cases, time.time() - t0))
sys.exit(1 if bad else 0)
