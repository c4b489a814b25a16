"""`ngs convert --gzip device --sort coordinate <BAM> <BAM>` on the MI355X: the sorted conversion of a BAM
whose records are shuffled, beside the bare ingest scan of the same file and beside the SAM route (ngsq_sam_write_sorted_bam on
the same records' text), and the done-when checks at size.

    python tools/bench_bam_sort.py [--plain-records N] [--aligner-records N] [--reps K] [--slice-records N] [--dir D] [--out JSON]

Files: the plain file of bench.py's file leg (chr1 + chr2, 150 bp, 60 M records) and the aligner-shaped one of its realistic leg
(the 195 @SQ of GRCh38 no-alt, 150 M records), as tools/bench_sam_sort.py makes them: the SAM text with its record lines shuffled
by `shuf` (its random source: the BAM's own bytes, so a run can be repeated), and the BAM of that text in the same order, written
by `ngs convert --gzip device`.  When --dir has no room, fewer records of the same shape are used, and the result says so.

Every step that uses the GPU is a child process of its own under `timeout`, and the first step that fails ends the run:
  make <file>     the BAM, its SAM text, the shuffled text, the shuffled BAM (the file and the text in order are removed)
  scan <file>     the bare device ingest of the shuffled BAM: every batch of ngsq_bam_next_batch_device, nothing done with it
  convert <file>  in process into /dev/null, after one warm-up: ngsq_bam_write_sorted_bam of the shuffled BAM and
                  ngsq_sam_write_sorted_bam of the shuffled text, alternating; the ratio of the medians and both reports' splits
  check <file>    `ngs convert --gzip device --sort coordinate` into a file, `ngs index` of it; then the first --slice-records
                  records as a BAM of their own: sorted, and compared with the model (tests/bam_sort_model.py) byte for byte
Medians of --reps runs.  One JSON line on stdout."""
from __future__ import annotations

import argparse
import ctypes as C
import gzip
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

FILES = {"plain": False, "aligner": True}
TEXT_PER_RECORD = {"plain": 350, "aligner": 475}
BAM_PER_RECORD = {"plain": 110, "aligner": 160}
BATCH_RECORDS = 1 << 22  # the conversion's own batch size


def paths(d, label):
    return {k: os.path.join(d, f"{label}.{k}") for k in ("bam", "sam", "shuf.sam", "shuf.bam", "sorted.bam", "slice.in.bam", "slice.bam")}


def step_make(args, d, label, n):
    from tools.bench_index import write_file
    lib = ffi.load_library()
    ngs = build.build_cli(verbose=False)
    p = paths(d, label)
    write_file(lib, p["bam"], int(n), FILES[label])
    if os.path.exists(p["bam"] + ".bai"):
        os.remove(p["bam"] + ".bai")
    r = subprocess.run([ngs, "convert", p["bam"], p["sam"]], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the header stays in front; the record lines behind it are shuffled
    head = 0
    with open(p["sam"], "rb") as f:
        for ln in f:
            if not ln.startswith(b"@"):
                break
            head += len(ln)
    with open(p["sam"], "rb") as f, open(p["shuf.sam"], "wb") as o:
        o.write(f.read(head))
        o.flush()
        tail = subprocess.Popen(["tail", "-c", f"+{head + 1}", p["sam"]], stdout=subprocess.PIPE)
        rc = subprocess.run(["shuf", f"--random-source={p['bam']}"], stdin=tail.stdout, stdout=o).returncode
        assert tail.wait() == 0 and rc == 0
    sam_bytes = os.path.getsize(p["sam"])
    assert os.path.getsize(p["shuf.sam"]) == sam_bytes
    os.remove(p["sam"])
    os.remove(p["bam"])
    r = subprocess.run([ngs, "convert", "--gzip", "device", p["shuf.sam"], p["shuf.bam"]], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return {"records": int(n), "bam_bytes": os.path.getsize(p["shuf.bam"]), "sam_bytes": sam_bytes}


def step_scan(args, d, label):
    lib = ffi.load_library()
    src = paths(d, label)["shuf.bam"]

    def once():
        t0 = time.perf_counter()
        n = 0
        with host._reader_and_plain_context(lib, src, 0) as (bam, ctx):
            while True:
                b = ffi.Batch()
                rc = lib.ngsq_bam_next_batch_device(bam, ctx, BATCH_RECORDS, C.byref(b))
                assert rc == ffi.OK, lib.ngsq_bam_last_error()
                if not b.n_records:
                    break
                n += int(b.n_records)
            dt = (time.perf_counter() - t0) * 1e3
        return n, dt
    once()  # warm-up: the page cache, the process's block cache
    runs = [once() for _ in range(args.reps)]
    return {"records": runs[0][0], "scan_ms": round(statistics.median(r[1] for r in runs), 1), "all_ms": [round(r[1], 1) for r in runs]}


def step_convert(args, d, label):
    lib = ffi.load_library()
    p = paths(d, label)
    host.bam_to_sorted_bam(p["shuf.bam"], "/dev/null", lib=lib)  # warm-up: the page cache, the process's block cache
    runs = {"bam": [], "sam": []}
    for _ in range(args.reps):
        for kind, fn, src in (("bam", host.bam_to_sorted_bam, p["shuf.bam"]), ("sam", host.sam_to_sorted_bam, p["shuf.sam"])):
            t0 = time.perf_counter()
            rep = fn(src, "/dev/null", lib=lib)
            rep["wall_ms"] = (time.perf_counter() - t0) * 1e3
            runs[kind].append(rep)
    med = statistics.median
    first = runs["bam"][0]
    out = {k: first[k] for k in ("records", "bam_bytes", "compressed_bytes", "passes_run", "batches", "slabs", "pieces", "resident_bytes")}
    out["input_bytes"] = os.path.getsize(p["shuf.bam"])
    out["text_bytes"] = runs["sam"][0]["text_bytes"]
    assert runs["sam"][0]["records"] == first["records"]
    for kind, keys in (("bam", ("scan_ms", "keep_ms", "sort_ms", "gather_ms", "deflate_ms", "d2h_ms", "write_ms")),
                       ("sam", ("read_ms", "h2d_ms", "parse_ms", "sort_ms", "gather_ms", "deflate_ms", "d2h_ms", "write_ms"))):
        out[kind + "_ms"] = round(med(r["wall_ms"] for r in runs[kind]), 1)
        out[kind + "_all_ms"] = [round(r["wall_ms"], 1) for r in runs[kind]]
        out[kind + "_split"] = {k: round(med(r[k] for r in runs[kind]), 1) for k in keys}
    out["bam_over_sam"] = round(out["bam_ms"] / out["sam_ms"], 3)
    return out


def step_check(args, d, label):
    from tests import bam_sort_model as bsm
    ngs = build.build_cli(verbose=False)
    p = paths(d, label)
    run = lambda *a: subprocess.run([ngs, *a], capture_output=True, text=True)
    t0 = time.perf_counter()
    r = run("convert", "--gzip", "device", "--sort", "coordinate", p["shuf.bam"], p["sorted.bam"])
    assert r.returncode == 0, r.stderr
    cli_ms = (time.perf_counter() - t0) * 1e3
    r = run("index", p["sorted.bam"])
    out = {"cli_convert_ms": round(cli_ms, 1), "sorted_bam_bytes": os.path.getsize(p["sorted.bam"]), "index_accepts": r.returncode == 0,
           "index_stderr": r.stderr[-300:] if r.returncode else ""}
    if r.returncode == 0:
        out["bai_bytes"] = os.path.getsize(p["sorted.bam"] + ".bai")
        os.remove(p["sorted.bam"] + ".bai")
    os.remove(p["sorted.bam"])
    # the slice: the first records of the shuffled text as a BAM of their own, sorted, against the model
    r = run("convert", "--gzip", "device", "-n", str(args.slice_records), p["shuf.sam"], p["slice.in.bam"])
    assert r.returncode == 0, r.stderr
    r = run("convert", "--gzip", "device", "--sort", "coordinate", p["slice.in.bam"], p["slice.bam"])
    assert r.returncode == 0, r.stderr
    want = bsm.bam_stream(open(p["slice.in.bam"], "rb").read())
    out.update({"slice_records": args.slice_records, "slice_equals_model": gzip.decompress(open(p["slice.bam"], "rb").read()) == want})
    for q in ("slice.in.bam", "slice.bam"):
        os.remove(p[q])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain-records", type=int, default=60_000_000)
    ap.add_argument("--aligner-records", type=int, default=150_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slice-records", type=int, default=200_000)
    ap.add_argument("--step-seconds", type=int, default=900, help="time limit of one step")
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--step", nargs="+", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        fn = {"make": step_make, "scan": step_scan, "convert": step_convert, "check": step_check}[args.step[0]]
        print(json.dumps(fn(args, args.dir, *args.step[1:])))
        return
    build.build(verbose=False)
    tmp = tempfile.TemporaryDirectory(dir=args.dir)
    result = {"reps": args.reps, "files": {}}
    ok = True

    def run_step(*st):
        nonlocal ok
        cmd = ["timeout", "-k", "10", str(args.step_seconds), sys.executable, os.path.abspath(__file__), "--dir", tmp.name, "--reps", str(args.reps),
               "--slice-records", str(args.slice_records), "--step", *[str(x) for x in st]]
        child = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        t0 = time.time()
        while True:  # (a long step says that it is still running)
            try:
                so, se = child.communicate(timeout=60)
                break
            except subprocess.TimeoutExpired:
                print(f"[bench_bam_sort] {' '.join(str(x) for x in st)}: {time.time() - t0:.0f} s", file=sys.stderr, flush=True)
        if child.returncode != 0:  # (nothing more is started on the GPU behind a step that failed)
            print(f"[bench_bam_sort] step {' '.join(str(x) for x in st)} ended with {child.returncode}:\n{se[-4000:]}", file=sys.stderr, flush=True)
            result["failed_step"] = " ".join(str(x) for x in st)
            ok = False
            return None
        out = json.loads(so.strip().splitlines()[-1])
        print(f"[bench_bam_sort] {' '.join(str(x) for x in st)}: {json.dumps(out)}", file=sys.stderr, flush=True)
        return out

    for label, asked in (("plain", args.plain_records), ("aligner", args.aligner_records)):
        if not ok or asked <= 0:
            continue
        # the text twice (in order, shuffled) and the BAM three times (the source, the shuffled one, the sorted conversion's)
        per = 2 * TEXT_PER_RECORD[label] + 3 * BAM_PER_RECORD[label]
        room = int(shutil.disk_usage(tmp.name).free * 0.9)
        n = min(asked, max(1000, room // per))
        f = {"records_asked": asked, "records": n, "scaled_down": n < asked}
        for st in ("make", "scan", "convert", "check"):
            out = run_step(st, label, n) if st == "make" else run_step(st, label)
            if not ok:
                break
            f[st] = out
        result["files"][label] = f
        for q in paths(tmp.name, label).values():
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
