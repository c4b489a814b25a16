"""One median step of the default QC workload from a rocprofv3 kernel trace: every launch in order, its duration
and the gap in front of it.

    rocprofv3 --kernel-trace -d DIR -o out --output-format csv -- python bench.py --gpus 1 --steps 20 --warmup 5 --no-timing
    python tools/step_gaps.py DIR [STEPS]

A step starts at a k_fields launch and ends in front of the next one.  Only the last STEPS (default 20) steps with the most
common launch sequence are used; the step after the last has no end and is dropped.  "gap" is the launch's start minus the
latest end of any earlier launch of the trace: negative when it started beside a kernel that was still running (k_cov_stream_corun
beside k_gc).  The gap in front of k_fields holds the host's part of the step (ngsq_finalize's read-back, ngsq_reset).  All
figures are medians over the steps, in microseconds.
"""
from __future__ import annotations

import csv
import os
import re
import sys
from statistics import median


def find_trace(root: str) -> str:
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith("kernel_trace.csv"):
                return os.path.join(d, f)
    raise SystemExit(f"no *kernel_trace.csv under {root}")


def short(name: str) -> str:
    name = re.sub(r"\(.*$", "", name)            # the argument list
    name = re.sub(r"^(void|static|inline)\s+", "", name)
    name = name.replace("ngsq::", "").replace("(anonymous namespace)::", "")
    return name.strip()


def main() -> None:
    root = sys.argv[1]
    want = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rows = []
    with open(find_trace(root), newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    rows.sort()
    gaps, latest = [], None
    for s, e, _ in rows:
        gaps.append(0.0 if latest is None else (s - latest) / 1e3)
        latest = e if latest is None else max(latest, e)
    heads = [i for i, r in enumerate(rows) if r[2].startswith("k_fields")]
    steps = [(heads[k], heads[k + 1]) for k in range(len(heads) - 1)]
    seqs = [tuple(r[2] for r in rows[a:b]) for a, b in steps]
    common = max(set(seqs), key=seqs.count)
    steps = [st for st, q in zip(steps, seqs) if q == common][-want:]
    print(f"{len(steps)} steps of {len(common)} launches; medians, microseconds")
    print(f"{'#':>3} {'kernel':<44} {'gap':>9} {'duration':>9} {'start':>9}")
    tot_gap = tot_dur = 0.0
    for j, name in enumerate(common):
        g = median(gaps[a + j] for a, _ in steps)
        d = median((rows[a + j][1] - rows[a + j][0]) / 1e3 for a, _ in steps)
        s = median((rows[a + j][0] - rows[a][0]) / 1e3 for a, _ in steps)
        if g > 0:
            tot_gap += g
        tot_dur += d
        print(f"{j:>3} {name[:44]:<44} {g:>9.1f} {d:>9.1f} {s:>9.1f}")
    step = median((rows[b][0] - rows[a][0]) / 1e3 for a, b in steps)
    busy = []
    for a, b in steps:  # time of the step during which at least one kernel runs
        t, hi = 0, rows[a][0]
        for s, e, _ in rows[a:b]:
            if e > hi:
                t += e - max(s, hi)
                hi = e
        busy.append(t / 1e3)
    print(f"step (k_fields start to the next k_fields start) {step:.1f}; some kernel running {median(busy):.1f}; "
          f"no kernel running {step - median(busy):.1f}; sum of the positive gaps {tot_gap:.1f}")


if __name__ == "__main__":
    main()
