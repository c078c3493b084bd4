"""MetricDirect's index lists and pose batches against the all-pairs call (GPU only; DESIGN.md 4.27 holds the figures).

1024^2 images, 8 and 32 views, derivative and fan-beam (FBCC) forms.  Per configuration, in one process and alternating the
contestants window by window:
  a. the list of ONE moved view (n - 1 pairs, evaluate_pairs) against evaluate() (all n (n - 1) / 2 pairs);
  b. a 12-pose batch for one view (evaluate_pose_deltas: 12 (n - 1) pairs, one call) against 12 x (setProjectionMatrices +
     evaluate()), what a 12-probe central difference costs without it;
  c. the per-pair time of the list launch against the all-pairs launch's, with the list grown from n - 1 pairs to the all-pairs
     count: where a short list leaves the device underfilled, the per-pair time says so.
Every figure is the median over WINDOWS windows of a host clock around calls that end in a stream synchronise (both calls wait
for the device before they return), after warm-up; the spread beside it is the windows' minimum and maximum.

usage: python scripts/bench_direct_lists.py [--size 1024] [--views 8 32] [--windows 7] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def window(fn, min_seconds=0.15, min_calls=2):
    """Seconds per call over one window of at least min_seconds."""
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        dt = time.perf_counter() - t0
        if calls >= min_calls and dt >= min_seconds:
            return dt / calls


def contest(fns, windows):
    """Alternating windows of every contestant -> per contestant (median, min, max) in milliseconds."""
    for fn in fns.values():  # warm-up: every shape once, scratch grown
        fn()
        fn()
    t = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            t[k].append(1e3 * window(fn))
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in t.items()}


def fmt(s):
    return "%.3f ms [%.3f .. %.3f]" % s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--views", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import geometry, synthetic
    if not torch.cuda.is_available():
        sys.exit("bench_direct_lists.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    ctx = E.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    S, moved, results = a.size, 3, []
    for n in a.views:
        Ps = synthetic.short_scan(n, S, S, 0.308 * 1024 / S)
        imgs = synthetic.projections_torch(Ps, S, S, synthetic.sphere_phantom(), dev)
        n_all = n * (n - 1) // 2
        one_view = E.direct_pose_pairs(n, [moved])
        probes = [[Ps[moved] @ geometry.rigid_transform(tx=0.2 * (k - 5.5), rz=0.002 * (k - 5.5))] for k in range(12)]
        all_pairs = np.asarray([E.get_ij(ij, n) * 2 for ij in range(n_all)], np.int32)
        for fbcc in (False, True):
            m = E.MetricDirect(ctx, Ps, imgs).setFanBeamConsistency(fbcc)
            whole, listed = m.evaluate(), m.evaluate_pairs(all_pairs)  # the list path computes what the all-pairs path computes
            assert listed == whole or (np.isnan(listed) and np.isnan(whole)), (listed, whole)  # (the fan-beam form of the reference
            # is not finite on some lines of pairs about three quarters of the short scan apart: oracle, all-pairs and list agree)

            def sequential_probes():
                for P in probes:
                    Pk = list(Ps)
                    Pk[moved] = P[0]
                    m.setProjectionMatrices(Pk).evaluate()
                m.setProjectionMatrices(Ps)

            r = dict(size=S, views=n, fbcc=fbcc, all_pairs=n_all, list_pairs=len(one_view), all_pairs_sum=whole)
            r["a"] = contest({"all_pairs_evaluate": m.evaluate, "one_view_list": lambda: m.evaluate_pairs(one_view)}, a.windows)
            r["b"] = contest({"sequential_12": sequential_probes,
                              "pose_batch_12": lambda: m.evaluate_pose_deltas([[moved]] * 12, probes)}, a.windows)
            lengths = sorted({len(one_view), min(4 * len(one_view), n_all), n_all})
            lists = {"list_%d" % k: (lambda idx=np.ascontiguousarray(np.resize(all_pairs, (k, 4))): m.evaluate_pairs(idx)) for k in lengths}
            r["c"] = contest(dict(all_pairs_evaluate=m.evaluate, **lists), a.windows)
            m.close()
            results.append(r)
            tag = "%d views of %d^2, %s" % (n, S, "FBCC" if fbcc else "derivative")
            ev, li = r["a"]["all_pairs_evaluate"], r["a"]["one_view_list"]
            print("%s | a. evaluate() %d pairs %s; one view's list %d pairs %s; ratio %.2f (pairs: %.2f)"
                  % (tag, n_all, fmt(ev), len(one_view), fmt(li), ev[0] / li[0], n_all / len(one_view)))
            sq, pb = r["b"]["sequential_12"], r["b"]["pose_batch_12"]
            print("%s | b. 12 x (setProjectionMatrices + evaluate) %s; 12-pose batch %s; ratio %.2f" % (tag, fmt(sq), fmt(pb), sq[0] / pb[0]))
            per_pair = ["evaluate() %.2f us/pair" % (1e3 * r["c"]["all_pairs_evaluate"][0] / n_all)]
            per_pair += ["list of %d: %.2f us/pair [%.2f .. %.2f]" % ((k,) + tuple(1e3 * x / k for x in r["c"]["list_%d" % k])) for k in lengths]
            print("%s | c. %s" % (tag, "; ".join(per_pair)), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
