"""`ngs convert --gzip device --sort coordinate <BAM> <BAM>` in rounds on the MI355X: what a round costs.
The bench cannot use a file larger than the card, so the budget is shrunk instead: the shuffled BAMs of tools/bench_bam_sort.py
are converted into /dev/null in process, in memory and at budgets of 1/2, 1/4 and 1/8 of the resident need, beside the bare
ingest scan of the same file in the same run.

    python tools/bench_bam_sort_rounds.py [--plain-records N] [--aligner-records N] [--reps K] [--dir D] [--out JSON]

The figure per file and budget: (time in R rounds - time in memory) / ((R + 1) x bare scan) -- the design's cost of R rounds is
the in-memory time, one bare scan for the survey and one per round, so it predicts about 1.  (The attempt that overflows before
the survey is a further partial walk: the figure carries it.)

Every step that uses the GPU is a child process of its own under `timeout`, and the first step that fails ends the run:
  make <file>    tools/bench_bam_sort.py's: the shuffled BAM (and its text, removed here)
  scan <file>    tools/bench_bam_sort.py's: the bare device ingest of the shuffled BAM
  rounds <file>  after one warm-up: ngsq_bam_write_sorted_bam of the shuffled BAM, then ngsq_bam_write_sorted_bam_rounds at each
                 budget, --reps times over; medians, and the medians of the reports' splits
Medians of --reps runs.  One JSON line on stdout."""
from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ngs_amd import build, ffi, host  # noqa: E402
from tools import bench_bam_sort as bbs  # noqa: E402

FRACTIONS = (2, 4, 8)
SPLIT = ("scan_ms", "keep_ms", "sort_ms", "gather_ms", "deflate_ms", "d2h_ms", "write_ms")


def step_make(args, d, label, n):
    out = bbs.step_make(args, d, label, n)
    os.remove(bbs.paths(d, label)["shuf.sam"])  # (the SAM route takes no part here)
    return out


def step_rounds(args, d, label):
    lib = ffi.load_library()
    src = bbs.paths(d, label)["shuf.bam"]
    med = statistics.median
    first = host.bam_to_sorted_bam(src, "/dev/null", lib=lib)  # warm-up: the page cache, the process's block cache
    need = first["resident_bytes"]
    budgets = {f: -(-need // f) for f in FRACTIONS}
    runs = {0: []}
    runs.update({f: [] for f in FRACTIONS})
    for _ in range(args.reps):
        for f in (0,) + FRACTIONS:
            t0 = time.perf_counter()
            if f:
                rep, rr = host.bam_to_sorted_bam(src, "/dev/null", lib=lib, max_resident_bytes=budgets[f], rounds=True)
                rep.update(rr)
            else:
                rep = host.bam_to_sorted_bam(src, "/dev/null", lib=lib)
            rep["wall_ms"] = (time.perf_counter() - t0) * 1e3
            runs[f].append(rep)
    out = {"records": first["records"], "resident_need": need, "input_bytes": os.path.getsize(src),
           "memory_ms": round(med(r["wall_ms"] for r in runs[0]), 1), "memory_all_ms": [round(r["wall_ms"], 1) for r in runs[0]],
           "memory_split": {k: round(med(r[k] for r in runs[0]), 1) for k in SPLIT}, "budgets": {}}
    for f in FRACTIONS:
        rs = runs[f]
        assert all(r["compressed_bytes"] == first["compressed_bytes"] and r["records"] == first["records"] for r in rs)
        out["budgets"][f"1/{f}"] = {"budget": budgets[f], "rounds": rs[0]["rounds"], "walks": rs[0]["walks"], "survey_bytes": rs[0]["survey_bytes"],
                                    "resident_bytes": rs[0]["resident_bytes"], "ms": round(med(r["wall_ms"] for r in rs), 1),
                                    "all_ms": [round(r["wall_ms"], 1) for r in rs], "survey_ms": round(med(r["survey_ms"] for r in rs), 1),
                                    "split": {k: round(med(r[k] for r in rs), 1) for k in SPLIT}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain-records", type=int, default=60_000_000)
    ap.add_argument("--aligner-records", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-seconds", type=int, default=900, help="time limit of one step")
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--step", nargs="+", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        fn = {"make": step_make, "scan": bbs.step_scan, "rounds": step_rounds}[args.step[0]]
        print(json.dumps(fn(args, args.dir, *args.step[1:])))
        return
    build.build(verbose=False)
    tmp = tempfile.TemporaryDirectory(dir=args.dir)
    result = {"reps": args.reps, "files": {}}
    ok = True

    def run_step(*st):
        nonlocal ok
        cmd = ["timeout", "-k", "10", str(args.step_seconds), sys.executable, os.path.abspath(__file__), "--dir", tmp.name, "--reps", str(args.reps),
               "--step", *[str(x) for x in st]]
        child = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        t0 = time.time()
        while True:  # (a long step says that it is still running)
            try:
                so, se = child.communicate(timeout=60)
                break
            except subprocess.TimeoutExpired:
                print(f"[bench_bam_sort_rounds] {' '.join(str(x) for x in st)}: {time.time() - t0:.0f} s", file=sys.stderr, flush=True)
        if child.returncode != 0:  # (nothing more is started on the GPU behind a step that failed)
            print(f"[bench_bam_sort_rounds] step {' '.join(str(x) for x in st)} ended with {child.returncode}:\n{se[-4000:]}", file=sys.stderr, flush=True)
            result["failed_step"] = " ".join(str(x) for x in st)
            ok = False
            return None
        out = json.loads(so.strip().splitlines()[-1])
        print(f"[bench_bam_sort_rounds] {' '.join(str(x) for x in st)}: {json.dumps(out)}", file=sys.stderr, flush=True)
        return out

    for label, asked in (("plain", args.plain_records), ("aligner", args.aligner_records)):
        if not ok or asked <= 0:
            continue
        per = 2 * bbs.TEXT_PER_RECORD[label] + 2 * bbs.BAM_PER_RECORD[label]  # the text twice and the BAM twice while the file is made
        room = int(shutil.disk_usage(tmp.name).free * 0.9)
        n = min(asked, max(1000, room // per))
        f = {"records_asked": asked, "records": n, "scaled_down": n < asked}
        for st in ("make", "scan", "rounds"):
            out = run_step(st, label, n) if st == "make" else run_step(st, label)
            if not ok:
                break
            f[st] = out
        if ok:  # the figure: what a round costs, in bare scans
            scan, mem = f["scan"]["scan_ms"], f["rounds"]["memory_ms"]
            for b in f["rounds"]["budgets"].values():
                b["over_memory_ms"] = round(b["ms"] - mem, 1)
                b["cost_in_scans"] = round((b["ms"] - mem) / ((b["rounds"] + 1) * scan), 3)
        result["files"][label] = f
        for q in bbs.paths(tmp.name, label).values():
            for x in (q, q + ".bai"):
                if os.path.exists(x):
                    os.remove(x)
    tmp.cleanup()
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(line + "\n")
    print(line)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
