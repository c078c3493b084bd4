#!/usr/bin/env python3
"""profiles/view_hessian_1gpu.json from the outputs of one measurement job of scripts/bench_view_hessian.py:
    python scripts/profile_view_hessian.py LINES.jsonl BENCH.jsonl TRACE.db PARENT_REVISION > profiles/view_hessian_1gpu.json
LINES.jsonl: the JSON lines of four runs of scripts/bench_view_hessian.py in one job, tagged --tag parent_run1 (with --lib, the
parent revision's library), this_run1, parent_run2, this_run2 -- kept unchanged under "lines".  BENCH.jsonl: the result lines of
bench.py --gpus 1 --steps 200 --warmup 20 --no-live-pmc --no-cpu-baseline on the parent's tree, this one, the parent's, this one.
TRACE.db: the database rocprofv3 --kernel-trace writes for scripts/bench_view_hessian.py --once 2,4 (per K the metric's set-up, then
two calls).  "gate": per K and run, a = this revision's a_moments_kernel, b = the PARENT's b_* kernel of the same run number, h = this
revision's h_whole_call_with_H, c = the PARENT's c_one_hot_view_coefficients ms_for_the_matrix; the gates are a <= 1.15 b and
c >= 10 h.  "kernel_trace_us": the durations of the record, moment and assembly kernels in dispatch order, K = 2 first."""
import json
import re
import sqlite3
import sys

lines_path, bench_path, trace_path, parent = sys.argv[1:5]
rows = [json.loads(l) for l in open(lines_path) if l.strip()]
bench = [json.loads(l) for l in open(bench_path) if l.strip()]


def pick(tag, leg, K, key):
    return [r for r in rows if r["lib"] == tag and r["leg"].startswith(leg) and r["channels"] == K][0][key]


gate = []
for K in sorted({r["channels"] for r in rows}):
    for run in (1, 2):
        a, b = pick("this_run%d" % run, "a_", K, "kernel_ms"), pick("parent_run%d" % run, "b_", K, "kernel_ms")
        h, c = pick("this_run%d" % run, "h_", K, "ms_per_call"), pick("parent_run%d" % run, "c_", K, "ms_for_the_matrix")
        gate.append(dict(channels=K, run=run, a_kernel_ms=a, b_parent_kernel_ms=b, b_this_kernel_ms=pick("this_run%d" % run, "b_", K, "kernel_ms"),
                         a_over_b_parent=a / b, gate_1_15="passes" if a <= 1.15 * b else "missed", h_whole_call_ms=h,
                         c_parent_one_hot_calls_ms=c, c_over_h=c / h, gate_10x="passes" if c >= 10 * h else "missed"))
trace = {}
for name, start, end in sqlite3.connect(trace_path).execute("select name, start, end from kernels order by start"):
    for kernel in ("k01_kernel", "pairs_moments_kernel", "assemble_view_hessian_kernel"):
        if re.search(r"\b%s\b" % kernel, name):
            trace.setdefault(kernel, []).append((end - start) / 1e3)
json.dump(dict(what="scripts/bench_view_hessian.py on one MI355X, summarised by scripts/profile_view_hessian.py (see its docstring for "
                    "every field): 400 views of 1024^2, 768^2 bins, POLYNOMIAL; median of 5 windows >= 0.3 s with min / max; the parent "
                    "revision's library (%s) and this revision's alternated in one job." % parent,
               gate=gate, kernel_trace_us=trace,
               bench_py=dict(order=["parent", "this", "parent", "this"], evaluations_per_s=[b["value"] for b in bench],
                             ms_per_step=[b["ms_per_step"] for b in bench]), lines=rows), sys.stdout, indent=1)
