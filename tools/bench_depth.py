"""`ngs depth <BAM> [QUERY]` on the MI355X: what the depth of a file, of a chromosome and of 1 Mbp costs
against the bare scan of the same walks and against the time the text's bytes need over the pinned device-to-host link.

    python tools/bench_depth.py [--plain-records N] [--aligner-records N] [--reps K] [--dir D] [--out JSON] [--step-timeout S]

Files: those of tools/bench_convert.py (the plain file of bench.py's file leg, the aligner-shaped one of its realistic leg), with
the index the synthetic writer puts beside them.  Every step that uses the GPU is a child process of this one under its own time
limit, and the first one that fails ends the run: nothing more is started.  Per file: the file is written, a warm-up scan (the
page cache) and --reps bare scans; then, for the whole file, the whole first sequence and 1 Mbp in its middle, --reps times in
process into /dev/null:
  depth_ms       open, context and ngsq_bam_depth, as a caller sees it (depth_call_ms: the library call alone)
  scan_ms        the bare scan of the same walks: every batch of ngsq_bam_next_batch_device, nothing else (for a region:
                 ngsq_bam_range_begin per walk the call made, same coalescing)
  bound_ms       the larger of scan_ms and text_bytes / D2H_GBPS (the pinned rate of DESIGN.md section 13.5)
  *_gpu_ms       the report's split of the kernels' GPU time: add, runs, format; copy
  format_gbps    text_bytes over format_gpu_ms: what the size pass, its scan and the write pass reach together
Then, in the same run and on the whole file, `ngs depth --by` at 500 and 1000 positions a window and over a
BED file the tool makes (--bed-intervals intervals of 100 to 300 positions, spread over the file's sequences by their length):
  by_ms          open, context and ngsq_bam_depth_windows (by_call_ms: the library call alone; for the BED leg the file is read
                 outside the clock and handed over as a list)
  by_over_depth  by_call_ms over the whole file's depth_call_ms of the same run
  *_gpu_ms       the report's split: add, reduce (block sums, offsets, prefix sums, window or interval sums), format; copy
Then the thresholds legs, each beside the plain `--by` leg of the same file in the same run: `--by 1000
--thresholds 1,10,20,30` and the same BED with the same list (ngsq_bam_depth_thresholds):
  thr_over_by         by_call_ms over the plain leg's by_call_ms
  reduce_over_by      reduce_gpu_ms over the plain leg's: the reduce pass moves 16 + 2 K bytes a position where it moved 16
  covered             the report's K totals: positions of all lines at or above each depth
Medians of --reps runs.  One JSON line on stdout."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D2H_GBPS = 56.0  # pinned device-to-host copies of 32 MiB
THRESHOLDS = "1,10,20,30"  # the thresholds legs' list


def child(args):
    """One GPU step; its result is one JSON line on stdout."""
    from ngs_amd import ffi, host
    from tools.bench_index import bare_scan_ms, write_file
    from tools.bench_view import GAP, range_scan_ms
    lib = ffi.load_library()
    med = statistics.median
    path = args.path
    if args.child == "write":
        t0 = time.perf_counter()
        write_file(lib, path, args.records, args.aligner)
        bam = C.c_void_p()
        assert lib.ngsq_bam_open(path.encode(), 1, C.byref(bam)) == 0
        out = {"records": args.records, "bytes": os.path.getsize(path), "write_s": round(time.perf_counter() - t0, 1),
               "sequence": lib.ngsq_bam_ref_name(bam, 0).decode(), "sequence_length": lib.ngsq_bam_ref_len(bam, 0), "sequences": lib.ngsq_bam_n_refs(bam)}
        lib.ngsq_bam_close(bam)
    elif args.child == "scan":
        bare_scan_ms(lib, path)  # warm-up: the page cache, the process's block cache
        scans = [bare_scan_ms(lib, path)[0] for _ in range(args.reps)]
        out = {"scan_ms": round(med(scans), 1), "all_ms": [round(x, 1) for x in scans]}
    elif args.child == "by":
        intervals = None
        if args.by == "bed":
            write_bed(lib, path, args.bed, args.bed_intervals)
            intervals = host.depth_read_bed(path, args.bed, lib=lib)
        kw = dict(intervals=intervals) if intervals is not None else dict(window=int(args.by))
        if args.thresholds:
            kw["thresholds"] = [int(t) for t in args.thresholds.split(",")]
        bare_scan_ms(lib, path)  # warm-up
        walls, reps = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            reps.append(host.bam_depth_windows(path, "/dev/null", lib=lib, **kw))
            walls.append((time.perf_counter() - t0) * 1e3)
        r0 = reps[0]
        out = {"by": args.by, "intervals": len(intervals) if intervals is not None else None, "records_scanned": r0["records_scanned"],
               "records_counted": r0["records_counted"], "lines": r0["lines"], "text_bytes": r0["text_bytes"], "sequences": r0["sequences"],
               "depth_sum": r0["depth_sum"], "tiles": r0["tiles"], "passes": r0["passes"], "batches": r0["batches"],
               "by_ms": round(med(walls), 1), "by_call_ms": round(med(r["total_ms"] for r in reps), 1),
               "ingest_ms": round(med(r["scan_ms"] for r in reps), 1), "add_gpu_ms": round(med(r["add_ms"] for r in reps), 1),
               "reduce_gpu_ms": round(med(r["reduce_ms"] for r in reps), 1), "format_gpu_ms": round(med(r["format_ms"] for r in reps), 1),
               "copy_gpu_ms": round(med(r["copy_ms"] for r in reps), 1), "write_ms": round(med(r["write_ms"] for r in reps), 1),
               "all_ms": {"by": [round(x, 1) for x in walls], "by_call": [round(r["total_ms"], 1) for r in reps],
                          "reduce_gpu": [round(r["reduce_ms"], 2) for r in reps]}}
        if args.thresholds:
            out["thresholds"], out["covered"] = kw["thresholds"], r0["covered"]
    else:
        query = args.query or None
        chunks = host.bam_query_chunks(path, query, lib=lib)[3] if query else None
        bare_scan_ms(lib, path) if not query else range_scan_ms(lib, path, chunks)  # warm-up
        walls, reps, bare = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            reps.append(host.bam_depth(path, "/dev/null", query=query, coalesce_gap=GAP, lib=lib))
            walls.append((time.perf_counter() - t0) * 1e3)
            bare.append(range_scan_ms(lib, path, chunks)[0] if query else bare_scan_ms(lib, path)[0])
        r0 = reps[0]
        scan, text = med(bare), r0["text_bytes"]
        bound = max(scan, text / (D2H_GBPS * 1e6))
        fmt = med(r["format_ms"] for r in reps)
        out = {"query": query, "records_scanned": r0["records_scanned"], "records_counted": r0["records_counted"], "runs": r0["runs"],
               "text_bytes": text, "sequences": r0["sequences"], "tiles": r0["tiles"], "batches": r0["batches"], "ranges": r0["ranges"],
               "depth_ms": round(med(walls), 1), "depth_call_ms": round(med(r["total_ms"] for r in reps), 1), "scan_ms": round(scan, 1),
               "text_over_d2h_ms": round(text / (D2H_GBPS * 1e6), 1), "bound_ms": round(bound, 1), "depth_over_bound": round(med(walls) / bound, 2),
               "ingest_ms": round(med(r["scan_ms"] for r in reps), 1), "add_gpu_ms": round(med(r["add_ms"] for r in reps), 1),
               "runs_gpu_ms": round(med(r["runs_ms"] for r in reps), 1), "format_gpu_ms": round(fmt, 1),
               "copy_gpu_ms": round(med(r["copy_ms"] for r in reps), 1), "write_ms": round(med(r["write_ms"] for r in reps), 1),
               "format_gbps": round(text / (fmt * 1e6), 1) if fmt > 0 else None,
               "all_ms": {"depth": [round(x, 1) for x in walls], "scan": [round(x, 1) for x in bare]}}
    print(json.dumps(out))


def write_bed(lib, path, bed, n):
    """Some n intervals of 100 to 300 positions over the sequences of the BAM `path`, by their length, in no order: host work."""
    import numpy as np
    bam = C.c_void_p()
    assert lib.ngsq_bam_open(path.encode(), 1, C.byref(bam)) == 0
    seqs = [(lib.ngsq_bam_ref_name(bam, r).decode(), lib.ngsq_bam_ref_len(bam, r)) for r in range(lib.ngsq_bam_n_refs(bam))]
    lib.ngsq_bam_close(bam)
    seqs = [(name, ln) for name, ln in seqs if ln > 300]
    total = sum(ln for _, ln in seqs)
    rng = np.random.default_rng(24)
    with open(bed, "w") as f:
        for name, ln in seqs:
            k = max(1, round(n * ln / total))
            starts = rng.integers(0, ln - 300, size=k)
            lens = rng.integers(100, 301, size=k)
            f.write("".join(f"{name}\t{s}\t{s + w}\n" for s, w in zip(starts.tolist(), lens.tolist())))


def step(limit, *argv):
    """A child under its time limit; None: it failed (the run ends there)."""
    cmd = [sys.executable, os.path.abspath(__file__), *[str(a) for a in argv]]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"[bench_depth] time limit of {limit} s: {' '.join(cmd)}", file=sys.stderr, flush=True)
        return None
    if r.returncode != 0:
        print(f"[bench_depth] exit {r.returncode}: {' '.join(cmd)}\n{r.stderr[-2000:]}", file=sys.stderr, flush=True)
        return None
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain-records", type=int, default=60_000_000)
    ap.add_argument("--aligner-records", type=int, default=150_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds a child may take")
    ap.add_argument("--bed-intervals", type=int, default=200_000, help="intervals of the BED leg")
    ap.add_argument("--child", choices=["write", "scan", "depth", "by"], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--by", default="", help=argparse.SUPPRESS)
    ap.add_argument("--bed", default="", help=argparse.SUPPRESS)
    ap.add_argument("--thresholds", default="", help=argparse.SUPPRESS)
    ap.add_argument("--path", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--records", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--aligner", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--query", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    from ngs_amd import build
    build.build(verbose=False)
    tmp = tempfile.TemporaryDirectory(dir=args.dir)
    result = {"reps": args.reps, "d2h_gbps": D2H_GBPS, "files": {}, "complete": False}
    ok = True
    for label, n, aligner in (("plain", args.plain_records, False), ("aligner", args.aligner_records, True)):
        if n <= 0 or not ok:
            continue
        path = os.path.join(tmp.name, f"{label}.bam")
        entry = step(args.step_timeout, "--child", "write", "--path", path, "--records", n, *(["--aligner"] if aligner else []))
        ok = entry is not None
        if ok:
            scan = step(args.step_timeout, "--child", "scan", "--path", path, "--reps", args.reps)
            ok = scan is not None
        if ok:
            entry["scan_ms"], entry["scan_all_ms"] = scan["scan_ms"], scan["all_ms"]
            name, ln = entry["sequence"], entry["sequence_length"]
            for what, query in (("whole_file", ""), ("chromosome", name), ("region_1mbp", f"{name}:{ln // 2}-{ln // 2 + 999_999}")):
                got = step(args.step_timeout, "--child", "depth", "--path", path, "--reps", args.reps, "--query", query)
                if got is None:
                    ok = False
                    break
                entry[what] = got
                print(f"[bench_depth] {label} {what}: {json.dumps(got)}", file=sys.stderr, flush=True)
            for by in ("500", "1000", "bed") if ok else ():
                got = step(args.step_timeout, "--child", "by", "--path", path, "--reps", args.reps, "--by", by, "--bed", os.path.join(tmp.name, f"{label}.bed"),
                           "--bed-intervals", args.bed_intervals)
                if got is None:
                    ok = False
                    break
                got["by_over_depth"] = round(got["by_call_ms"] / entry["whole_file"]["depth_call_ms"], 2)
                entry["by_" + by] = got
                print(f"[bench_depth] {label} --by {by}: {json.dumps(got)}", file=sys.stderr, flush=True)
            for by in ("1000", "bed") if ok else ():
                got = step(args.step_timeout, "--child", "by", "--path", path, "--reps", args.reps, "--by", by, "--bed", os.path.join(tmp.name, f"{label}.bed"),
                           "--bed-intervals", args.bed_intervals, "--thresholds", THRESHOLDS)
                if got is None:
                    ok = False
                    break
                base = entry["by_" + by]
                got["by_over_depth"] = round(got["by_call_ms"] / entry["whole_file"]["depth_call_ms"], 2)
                got["thr_over_by"] = round(got["by_call_ms"] / base["by_call_ms"], 2)
                got["reduce_over_by"] = round(got["reduce_gpu_ms"] / base["reduce_gpu_ms"], 2) if base["reduce_gpu_ms"] > 0 else None
                entry["by_" + by + "_thresholds"] = got
                print(f"[bench_depth] {label} --by {by} --thresholds {THRESHOLDS}: {json.dumps(got)}", file=sys.stderr, flush=True)
            result["files"][label] = entry
        if os.path.exists(path):
            os.remove(path)
    tmp.cleanup()
    result["complete"] = ok
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
