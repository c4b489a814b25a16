"""`ngs convert --gzip device --sort coordinate --write-index` on the MI355X: what writing the BAI with the
sorted BAM adds to the sorted conversion, beside what `ngs index` of the written file takes, and the done-when checks at size.

    python tools/bench_sort_index.py [--plain-records N] [--aligner-records N] [--reps K] [--dir D] [--out JSON]

Files: the two shuffled files of tools/bench_bam_sort.py (its `make` step is used as it is): 60 M plain records and 50 M
aligner-shaped ones on the 195 @SQ of GRCh38 no-alt.  When --dir has no room, fewer records of the same shape are used, and
the result says so.

Every step that uses the GPU is a child process of its own under `timeout`, and the first step that fails ends the run:
  make <file>     the shuffled BAM (and its text, which this tool does not use)
  convert <file>  in process into /dev/null, after one warm-up, alternating: ngsq_bam_write_sorted_bam, the yardstick, and
                  ngsq_bam_write_sorted_bam_indexed with its BAI into --dir; the medians, their difference, and the split of
                  the addition into index pass, block-table appends, translation (device times) and the BAI file
  index <file>    the indexed conversion into a file; then ngsq_bam_build_index of that file in process, after one warm-up;
                  whether its BAI equals the one written with the BAM
  cli <file>      through the command line: `convert` then `index`, against `convert --write-index`; whether the two BAIs are
                  equal; `ngs view` of a 1 Mbp region answered from the index written with the BAM
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
from tools.bench_bam_sort import BAM_PER_RECORD, TEXT_PER_RECORD, paths, step_make  # noqa: E402

SPLIT = ("pass_ms", "blocks_ms", "translate_ms", "write_ms")
REGION = "chr1:50000000-51000000"   # 1 Mbp


def remove(*files):
    for f in files:
        if os.path.exists(f):
            os.remove(f)


def step_convert(args, d, label):
    lib = ffi.load_library()
    p = paths(d, label)
    bai = p["sorted.bam"] + ".inproc.bai"
    host.bam_to_sorted_bam(p["shuf.bam"], "/dev/null", lib=lib)  # warm-up: the page cache, the process's block cache
    plain, indexed, ireps = [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        rep = host.bam_to_sorted_bam(p["shuf.bam"], "/dev/null", lib=lib)
        plain.append((time.perf_counter() - t0) * 1e3)
        remove(bai)
        t0 = time.perf_counter()
        rep, irep = host.bam_to_sorted_bam(p["shuf.bam"], "/dev/null", lib=lib, bai_path=bai)
        indexed.append((time.perf_counter() - t0) * 1e3)
        ireps.append(irep)
    med = statistics.median
    out = {"records": rep["records"], "bam_bytes": rep["bam_bytes"], "pieces": rep["pieces"], "blocks": rep["blocks"],
           "runs": ireps[0]["runs"], "bins": ireps[0]["bins"], "n_no_coor": ireps[0]["n_no_coor"], "bai_bytes": os.path.getsize(bai),
           "plain_ms": round(med(plain), 1), "plain_all_ms": [round(x, 1) for x in plain],
           "indexed_ms": round(med(indexed), 1), "indexed_all_ms": [round(x, 1) for x in indexed],
           "split": {k: round(med(r[k] for r in ireps), 2) for k in SPLIT}}
    out["added_ms"] = round(out["indexed_ms"] - out["plain_ms"], 1)
    out["split_sum_ms"] = round(sum(out["split"].values()), 1)
    remove(bai)
    return out


def step_index(args, d, label):
    lib = ffi.load_library()
    p = paths(d, label)
    out_bam, other = p["sorted.bam"], p["sorted.bam"] + ".by_index.bai"
    remove(out_bam + ".bai")
    host.bam_to_sorted_bam(p["shuf.bam"], out_bam, lib=lib, bai_path=out_bam + ".bai")
    runs = []
    for k in range(args.reps + 1):  # the first one is the warm-up
        remove(other)
        t0 = time.perf_counter()
        rep = host.build_bam_index(out_bam, bai_path=other, lib=lib)
        runs.append((time.perf_counter() - t0) * 1e3)
    same = open(other, "rb").read() == open(out_bam + ".bai", "rb").read()
    remove(other, out_bam, out_bam + ".bai")
    return {"records": rep["records"], "build_index_ms": round(statistics.median(runs[1:]), 1), "build_index_all_ms": [round(x, 1) for x in runs[1:]],
            "bai_equals_ngs_index": same}


def step_cli(args, d, label):
    ngs = build.build_cli(verbose=False)
    p = paths(d, label)
    two, one = p["sorted.bam"], p["sorted.bam"] + ".wi.bam"
    run = lambda *a: subprocess.run([ngs, *a], capture_output=True, text=True)

    def timed(*a):
        t0 = time.perf_counter()
        r = run(*a)
        assert r.returncode == 0, r.stderr
        return (time.perf_counter() - t0) * 1e3
    chain, conv, idx, with_index = [], [], [], []
    for _ in range(args.reps):
        remove(two + ".bai", one + ".bai")
        a = timed("convert", "--gzip", "device", "--sort", "coordinate", p["shuf.bam"], two)
        b = timed("index", two)
        conv.append(a), idx.append(b), chain.append(a + b)
        with_index.append(timed("convert", "--gzip", "device", "--sort", "coordinate", "--write-index", p["shuf.bam"], one))
    med = statistics.median
    same = open(two + ".bai", "rb").read() == open(one + ".bai", "rb").read() and os.path.getsize(two) == os.path.getsize(one)
    remove(two, two + ".bai")
    r = subprocess.run([ngs, "view", "-m", "records-only", one, REGION], capture_output=True)   # no `ngs index` in between
    out = {"convert_ms": round(med(conv), 1), "index_ms": round(med(idx), 1), "convert_then_index_ms": round(med(chain), 1),
           "convert_write_index_ms": round(med(with_index), 1), "chain_all_ms": [round(x, 1) for x in chain],
           "write_index_all_ms": [round(x, 1) for x in with_index], "bai_equals_ngs_index": same,
           "view_region": REGION, "view_answers": r.returncode == 0, "view_records": r.stdout.count(b"\n"),
           "view_stderr": r.stderr[-300:].decode("utf-8", "replace") if r.returncode else ""}
    out["saved_ms"] = round(out["convert_then_index_ms"] - out["convert_write_index_ms"], 1)
    remove(one, one + ".bai")
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
        fn = {"make": step_make, "convert": step_convert, "index": step_index, "cli": step_cli}[args.step[0]]
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
                print(f"[bench_sort_index] {' '.join(str(x) for x in st)}: {time.time() - t0:.0f} s", file=sys.stderr, flush=True)
        if child.returncode != 0:  # (nothing more is started on the GPU behind a step that failed)
            print(f"[bench_sort_index] step {' '.join(str(x) for x in st)} ended with {child.returncode}:\n{se[-4000:]}", file=sys.stderr, flush=True)
            result["failed_step"] = " ".join(str(x) for x in st)
            ok = False
            return None
        out = json.loads(so.strip().splitlines()[-1])
        print(f"[bench_sort_index] {' '.join(str(x) for x in st)}: {json.dumps(out)}", file=sys.stderr, flush=True)
        return out

    for label, asked in (("plain", args.plain_records), ("aligner", args.aligner_records)):
        if not ok or asked <= 0:
            continue
        # the text twice while it is shuffled, the BAM three times (the shuffled one and the two sorted ones of the cli step)
        per = 2 * TEXT_PER_RECORD[label] + 3 * BAM_PER_RECORD[label]
        room = int(shutil.disk_usage(tmp.name).free * 0.9)
        n = min(asked, max(1000, room // per))
        f = {"records_asked": asked, "records": n, "scaled_down": n < asked}
        for st in ("make", "convert", "index", "cli"):
            out = run_step(st, label, n) if st == "make" else run_step(st, label)
            if not ok:
                break
            if st == "make":
                remove(paths(tmp.name, label)["shuf.sam"])  # (the text is not used here)
            f[st] = out
        result["files"][label] = f
        for q in paths(tmp.name, label).values():
            remove(q, q + ".bai")
    tmp.cleanup()
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(line + "\n")
    print(line)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
