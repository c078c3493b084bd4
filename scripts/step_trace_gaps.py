#!/usr/bin/env python3
"""The optimiser step's kernel boundaries from a rocprofv3 --kernel-trace run (no counters in that run) of bench.py:
    python scripts/step_trace_gaps.py <trace directory> [steps to keep, default 50]
Prints, over the last steps of the trace, the medians of: the all-pairs launch's duration, the time from its end to the sum
kernel's start (the join), and the time from the sum kernel's end to the next all-pairs launch's start (the front: result
seen, matrices staged, change detection, launch, dispatch).  The all-pairs launch is told from the moved view's list launch
of the same kernel by its duration."""
import csv
import glob
import statistics as st
import sys

root = sys.argv[1]
keep = int(sys.argv[2]) if len(sys.argv) > 2 else 50
rows = []
for f in glob.glob(root + "/**/*kernel_trace.csv", recursive=True):
    rows += list(csv.DictReader(open(f)))
ev = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows), key=lambda t: t[0])
pairs = [e for e in ev if "pairs_kernel" in e[2] and "sum_pairs" not in e[2]]
longest = max(e[1] - e[0] for e in pairs)
big = [e for e in pairs if e[1] - e[0] > longest / 2]
sums = [e for e in ev if "sum_pairs" in e[2]]
big = big[-keep:]
join, front = [], []
for k, b in enumerate(big):
    after = [s for s in sums if s[0] >= b[1] and (k + 1 == len(big) or s[0] < big[k + 1][0])]
    if not after:
        continue
    join.append((after[0][0] - b[1]) / 1e3)
    if k + 1 < len(big):
        front.append((big[k + 1][0] - after[0][1]) / 1e3)
print("steps %d | all-pairs launch: median %.1f us | its end -> sum start: median %.2f us (min %.2f) | sum end -> next all-pairs start: "
      "median %.2f us (min %.2f)" % (len(big), st.median((b[1] - b[0]) / 1e3 for b in big), st.median(join), min(join),
                                     st.median(front), min(front)))
