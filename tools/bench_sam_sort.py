"""`ngs convert --gzip device --sort coordinate <SAM> <BAM>` on the MI355X: the sort alone beside its
traffic bound, the sorted conversion beside the unsorted one of the same text in the same run, and the done-when checks at size.

    python tools/bench_sam_sort.py [--plain-records N] [--aligner-records N] [--reps K] [--slice-records N] [--dir D] [--out JSON]

Files: the SAM text of the plain file of bench.py's file leg (chr1 + chr2, 150 bp, 60 M records) and of the aligner-shaped one
of its realistic leg (the 195 @SQ of GRCh38 no-alt, 150 M records), as tools/bench_sam_to_bam.py makes them, with the record
lines shuffled by `shuf` (its random source: the BAM's own bytes, so a run can be repeated).  When --dir has no room, fewer
records of the same shape are used, and the result says so.

Every step that uses the GPU is a child process of its own under `timeout`, and the first step that fails ends the run:
  make <file>     the BAM, its SAM text, the shuffled text (the text in order is removed)
  sort <file>     ngsq_sort_u64_device on the file's keys -- (refID, pos) of the BAM's records through the host reader, under
                  the key rule of section 19.1, in a seeded random order -- its GPU time, the passes it ran, and the traffic
                  bound passes x 24 bytes x n / HBM_GBS
  convert <file>  in process into /dev/null, after one warm-up: ngsq_sam_write_sorted_bam and ngsq_sam_write_bam of the shuffled
                  text, alternating; the ratio of the medians and both reports' splits
  check <file>    `ngs convert --gzip device --sort coordinate` into a file, `ngs index` of it; then the first --slice-records
                  records: converted with -n, converted back, compared with the model (tests/sort_model.py) byte for byte
Medians of --reps runs.  One JSON line on stdout."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ngs_amd import build, ffi, host  # noqa: E402

HBM_GBS = 6290.0  # the copy rate measured on an MI355X (8.0 TB/s is the specification's)
FILES = {"plain": False, "aligner": True}
TEXT_PER_RECORD = {"plain": 350, "aligner": 475}
BAM_PER_RECORD = {"plain": 110, "aligner": 160}


def paths(d, label):
    return {k: os.path.join(d, f"{label}.{k}") for k in ("bam", "sam", "shuf.sam", "sorted.bam", "slice.sam", "slice.bam", "back.sam")}


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
    return {"records": int(n), "bam_bytes": os.path.getsize(p["bam"]), "sam_bytes": sam_bytes}


def file_keys(lib, path):
    """The keys of section 19.1 of every record of the BAM, through the host reader."""
    h = C.c_void_p()
    assert lib.ngsq_bam_open(path.encode(), 16, C.byref(h)) == 0, lib.ngsq_bam_last_error()
    out = []
    try:
        while True:
            b = ffi.Batch()
            assert lib.ngsq_bam_next_batch(h, 4 << 20, C.byref(b)) == 0, lib.ngsq_bam_last_error()
            n = int(b.n_records)
            if not n:
                break
            col = lambda p: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), shape=(n,)).astype(np.int64)
            ref, pos = col(b.ref_id), col(b.pos)
            hi = np.where((ref < 0) | (pos < 0), 0xFFFFFFFF, ref).astype(np.uint64)
            out.append(hi << np.uint64(32) | ((pos + 1) & 0xFFFFFFFF).astype(np.uint64))
    finally:
        lib.ngsq_bam_close(h)
    return np.concatenate(out) if out else np.zeros(0, np.uint64)


def step_sort(args, d, label):
    lib = ffi.load_library()
    keys = file_keys(lib, paths(d, label)["bam"])
    keys = keys[np.random.default_rng(19).permutation(len(keys))]
    perm, _ = host.sort_u64(keys, lib=lib)  # warm-up; its answer is checked once
    s = keys[perm]
    assert np.all(s[1:] >= s[:-1]) and np.all((perm[1:] > perm[:-1]) | (s[1:] != s[:-1]))
    reps = [host.sort_u64(keys, lib=lib)[1] for _ in range(args.reps)]
    ms = statistics.median(r["sort_ms"] for r in reps)
    bound = reps[0]["passes_run"] * 24 * len(keys) / (HBM_GBS * 1e9) * 1e3
    return {"keys": len(keys), "passes_run": reps[0]["passes_run"], "sort_ms": round(ms, 2), "all_ms": [round(r["sort_ms"], 2) for r in reps],
            "traffic_bound_ms": round(bound, 2), "sort_over_bound": round(ms / bound, 2) if bound else None, "hbm_gbs": HBM_GBS}


def step_convert(args, d, label):
    lib = ffi.load_library()
    src = paths(d, label)["shuf.sam"]
    host.sam_to_bam(src, "/dev/null", lib=lib)  # warm-up: the page cache, the process's block cache
    runs = {"sorted": [], "unsorted": []}
    for _ in range(args.reps):
        for kind, fn in (("sorted", host.sam_to_sorted_bam), ("unsorted", host.sam_to_bam)):
            t0 = time.perf_counter()
            rep = fn(src, "/dev/null", lib=lib)
            rep["wall_ms"] = (time.perf_counter() - t0) * 1e3
            runs[kind].append(rep)
    med = statistics.median
    out = {"records": runs["sorted"][0]["records"], "text_bytes": runs["sorted"][0]["text_bytes"], "bam_bytes": runs["sorted"][0]["bam_bytes"],
           "passes_run": runs["sorted"][0]["passes_run"], "chunks": runs["sorted"][0]["chunks"], "pieces": runs["sorted"][0]["pieces"],
           "resident_bytes": runs["sorted"][0]["resident_bytes"]}
    for kind, keys in (("sorted", ("read_ms", "h2d_ms", "parse_ms", "sort_ms", "gather_ms", "deflate_ms", "d2h_ms", "write_ms")),
                       ("unsorted", ("read_ms", "h2d_ms", "parse_ms", "deflate_ms", "d2h_ms", "write_ms"))):
        out[kind + "_ms"] = round(med(r["wall_ms"] for r in runs[kind]), 1)
        out[kind + "_all_ms"] = [round(r["wall_ms"], 1) for r in runs[kind]]
        out[kind + "_split"] = {k: round(med(r[k] for r in runs[kind]), 1) for k in keys}
    out["sorted_over_unsorted"] = round(out["sorted_ms"] / out["unsorted_ms"], 3)
    return out


def step_check(args, d, label):
    from tests import bam_text_model as tm
    from tests import sort_model as som
    ngs = build.build_cli(verbose=False)
    p = paths(d, label)
    run = lambda *a: subprocess.run([ngs, *a], capture_output=True, text=True)
    t0 = time.perf_counter()
    r = run("convert", "--gzip", "device", "--sort", "coordinate", p["shuf.sam"], p["sorted.bam"])
    assert r.returncode == 0, r.stderr
    cli_ms = (time.perf_counter() - t0) * 1e3
    r = run("index", p["sorted.bam"])
    out = {"cli_convert_ms": round(cli_ms, 1), "sorted_bam_bytes": os.path.getsize(p["sorted.bam"]), "index_accepts": r.returncode == 0,
           "index_stderr": r.stderr[-300:] if r.returncode else ""}
    if r.returncode == 0:
        out["bai_bytes"] = os.path.getsize(p["sorted.bam"] + ".bai")
        os.remove(p["sorted.bam"] + ".bai")
    os.remove(p["sorted.bam"])
    # the slice: the first records of the shuffled text against the model
    with open(p["shuf.sam"], "rb") as f, open(p["slice.sam"], "wb") as o:
        k = 0
        for ln in f:
            if not ln.startswith(b"@"):
                k += 1
                if k > args.slice_records:
                    break
            o.write(ln)
    r = run("convert", "--gzip", "device", "--sort", "coordinate", p["slice.sam"], p["slice.bam"])
    assert r.returncode == 0, r.stderr
    r = run("convert", p["slice.bam"], p["back.sam"])
    assert r.returncode == 0, r.stderr
    sam = open(p["slice.sam"], "rb").read()
    want = som.sorted_header(tm.split_header(sam)[0]) + b"".join(x + b"\n" for x in som.sorted_lines(sam))
    out.update({"slice_records": min(k, args.slice_records), "slice_equals_model": open(p["back.sam"], "rb").read() == want})
    for q in ("slice.sam", "slice.bam", "back.sam"):
        os.remove(p[q])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain-records", type=int, default=60_000_000)
    ap.add_argument("--aligner-records", type=int, default=150_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slice-records", type=int, default=1_000_000)
    ap.add_argument("--step-seconds", type=int, default=900, help="time limit of one step")
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--step", nargs="+", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        fn = {"make": step_make, "sort": step_sort, "convert": step_convert, "check": step_check}[args.step[0]]
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
                print(f"[bench_sam_sort] {' '.join(str(x) for x in st)}: {time.time() - t0:.0f} s", file=sys.stderr, flush=True)
        if child.returncode != 0:  # (nothing more is started on the GPU behind a step that failed)
            print(f"[bench_sam_sort] step {' '.join(str(x) for x in st)} ended with {child.returncode}:\n{se[-4000:]}", file=sys.stderr, flush=True)
            result["failed_step"] = " ".join(str(x) for x in st)
            ok = False
            return None
        out = json.loads(so.strip().splitlines()[-1])
        print(f"[bench_sam_sort] {' '.join(str(x) for x in st)}: {json.dumps(out)}", file=sys.stderr, flush=True)
        return out

    for label, asked in (("plain", args.plain_records), ("aligner", args.aligner_records)):
        if not ok or asked <= 0:
            continue
        # the text twice (in order, shuffled) and the BAM twice (the source and the sorted conversion's)
        per = 2 * TEXT_PER_RECORD[label] + 2 * BAM_PER_RECORD[label]
        room = int(shutil.disk_usage(tmp.name).free * 0.9)
        n = min(asked, max(1000, room // per))
        f = {"records_asked": asked, "records": n, "scaled_down": n < asked}
        for st in ("make", "sort", "convert", "check"):
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
