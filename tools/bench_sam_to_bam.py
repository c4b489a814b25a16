"""`ngs convert --gzip device <SAM> <BAM>` on the MI355X: what the conversion costs against three bounds
taken in the same run, and what it writes beside the BAM its text came from.

    python tools/bench_sam_to_bam.py [--plain-records N] [--aligner-records N] [--reps K] [--deflate-mb N] [--chunk-mb N] [--dir D] [--out JSON]

Files: the SAM text (`ngs convert <BAM> <SAM>`) of the plain file of bench.py's file leg (chr1 + chr2, 150 bp, 60 M records)
and of the aligner-shaped one of its realistic leg (the 195 @SQ of GRCh38 no-alt, 150 M records), both written by the library's
synthetic writer at zlib level 6 (tools/bench_index.py's files).  When --dir has no room for a file's text twice and its BAM
twice, fewer records of the same shape are used, and the result says so (records_asked, records, scaled_down).

Every step that uses the GPU is a child process of its own under `timeout`, and the first step that fails ends the run:
  make <file>       the BAM and its SAM text, written into --dir
  h2d               pinned host-to-device bandwidth in one process: 32 MiB copies from one pinned buffer, back to back
  read <file>       the bare file read: the text through pread in 64 MiB pieces, nothing else (no GPU; the first run warms the page cache)
  convert <file>    ngsq_sam_write_bam in process into /dev/null with the report's split (read / up / parse / deflate / down /
                    write), after one warm-up; then once into a file, for the size and the round trip
  deflate <file>    the encoder alone (ngsq_bgzf_deflate_device: its GPU time of deflate, CRC, scan and pack) on the first
                    --deflate-mb MB of the record bytes the conversion wrote, scaled to all of them
  roundtrip <file>  `ngs convert` of the BAM the conversion wrote back to SAM, compared with the input text byte for byte
Per file: bound_ms = max(text bytes / h2d_gbs, read_ms, deflate_ms), which of the three it is, and convert_ms over it.
Medians of --reps runs.  One JSON line on stdout."""
from __future__ import annotations

import argparse
import ctypes as C
import filecmp
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

PIECE = 32 << 20
FILES = {"plain": False, "aligner": True}
# bytes per record of the text and of the level-6 BAM (DESIGN.md section 13.5's files), to see whether a file fits --dir
TEXT_PER_RECORD = {"plain": 350, "aligner": 475}
BAM_PER_RECORD = {"plain": 110, "aligner": 160}


def paths(d, label):
    return {k: os.path.join(d, f"{label}.{k}") for k in ("bam", "sam", "out.bam", "back.sam")}


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
    return {"records": int(n), "bam_bytes": os.path.getsize(p["bam"]), "sam_bytes": os.path.getsize(p["sam"])}


def step_h2d(args, d):
    """Pinned H2D bandwidth: PIECE-sized hipMemcpyAsync from one pinned buffer into one device buffer, on one stream."""
    hip = C.CDLL("libamdhip64.so")
    dev, pin, st = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipSetDevice(0) == 0
    assert hip.hipMalloc(C.byref(dev), C.c_size_t(PIECE)) == 0
    assert hip.hipHostMalloc(C.byref(pin), C.c_size_t(PIECE), 0) == 0
    assert hip.hipStreamCreate(C.byref(st)) == 0
    C.memset(pin, 1, PIECE)
    runs = []
    try:
        n = max(1, (8 << 30) // PIECE)
        for _ in range(args.reps + 1):  # the first run is the warm-up
            t0 = time.perf_counter()
            for _ in range(n):
                assert hip.hipMemcpyAsync(dev, pin, C.c_size_t(PIECE), 1, st) == 0   # hipMemcpyHostToDevice
            assert hip.hipStreamSynchronize(st) == 0
            runs.append(n * PIECE / (time.perf_counter() - t0) / 1e9)
    finally:
        hip.hipStreamDestroy(st)
        hip.hipHostFree(pin)
        hip.hipFree(dev)
    return {"h2d_gbs": round(statistics.median(runs[1:]), 2), "all_gbs": [round(x, 2) for x in runs]}


def step_read(args, d, label):
    p = paths(d, label)
    buf = bytearray(64 << 20)
    runs = []
    for _ in range(args.reps + 1):
        fd = os.open(p["sam"], os.O_RDONLY)
        try:
            t0 = time.perf_counter()
            at = 0
            while True:
                r = os.preadv(fd, [buf], at)
                if r <= 0:
                    break
                at += r
            runs.append((time.perf_counter() - t0) * 1e3)
        finally:
            os.close(fd)
    return {"bytes": at, "read_ms": round(statistics.median(runs[1:]), 1), "all_ms": [round(x, 1) for x in runs]}


def step_convert(args, d, label):
    lib = ffi.load_library()
    p = paths(d, label)
    chunk = args.chunk_mb << 20
    host.sam_to_bam(p["sam"], "/dev/null", chunk_bytes=chunk, lib=lib)  # warm-up: the page cache, the process's block cache
    wall, reps = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        reps.append(host.sam_to_bam(p["sam"], "/dev/null", chunk_bytes=chunk, lib=lib))
        wall.append((time.perf_counter() - t0) * 1e3)
    rep = host.sam_to_bam(p["sam"], p["out.bam"], chunk_bytes=chunk, lib=lib)
    med = statistics.median
    out = {"records": rep["records"], "convert_ms": round(med(wall), 1), "all_ms": [round(x, 1) for x in wall], "out_bytes": os.path.getsize(p["out.bam"])}
    for k in ("header_bytes", "text_bytes", "bam_bytes", "compressed_bytes", "chunks", "blocks", "stored_blocks"):
        out[k] = rep[k]
    for k in ("read_ms", "h2d_ms", "parse_ms", "deflate_ms", "d2h_ms", "write_ms", "total_ms"):
        out["convert_" + k] = round(med(r[k] for r in reps), 1)
    return out


def step_deflate(args, d, label):
    lib = ffi.load_library()
    p = paths(d, label)
    with gzip.open(p["out.bam"], "rb") as f:
        data = f.read(args.deflate_mb << 20)
    # (the whole stream's size comes from the convert step: the parent scales the time to it)
    host.bgzf_deflate(data[:1 << 24], eof=False, lib=lib)  # warm-up
    reps = [host.bgzf_deflate(data, eof=False, lib=lib)[1] for _ in range(args.reps)]
    gpu = statistics.median(r["deflate_ms"] + r["crc_ms"] + r["pack_ms"] for r in reps)
    return {"in_bytes": len(data), "out_bytes": reps[0]["out_bytes"], "encoder_gpu_ms": round(gpu, 2), "input_gbs": round(len(data) / gpu / 1e6, 2)}


def step_roundtrip(args, d, label):
    ngs = build.build_cli(verbose=False)
    p = paths(d, label)
    r = subprocess.run([ngs, "convert", p["out.bam"], p["back.sam"]], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    same = filecmp.cmp(p["sam"], p["back.sam"], shallow=False)
    os.remove(p["back.sam"])
    return {"text_reads_back": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain-records", type=int, default=60_000_000)
    ap.add_argument("--aligner-records", type=int, default=150_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--deflate-mb", type=int, default=512)
    ap.add_argument("--chunk-mb", type=int, default=0, help="chunk_bytes of the conversion in MiB (0: the library's default)")
    ap.add_argument("--step-seconds", type=int, default=900, help="time limit of one step")
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--step", nargs="+", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        fn = {"make": step_make, "h2d": step_h2d, "read": step_read, "convert": step_convert, "deflate": step_deflate, "roundtrip": step_roundtrip}[args.step[0]]
        print(json.dumps(fn(args, args.dir, *args.step[1:])))
        return
    build.build(verbose=False)
    tmp = tempfile.TemporaryDirectory(dir=args.dir)
    result = {"reps": args.reps, "chunk_mb": args.chunk_mb, "deflate_mb": args.deflate_mb, "files": {}}
    ok = True

    def run_step(*st):
        nonlocal ok
        cmd = ["timeout", "-k", "10", str(args.step_seconds), sys.executable, os.path.abspath(__file__), "--dir", tmp.name, "--reps", str(args.reps),
               "--deflate-mb", str(args.deflate_mb), "--chunk-mb", str(args.chunk_mb), "--step", *[str(x) for x in st]]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:  # (nothing more is started on the GPU behind a step that failed)
            print(f"[bench_sam_to_bam] step {' '.join(str(x) for x in st)} ended with {r.returncode}:\n{r.stderr[-4000:]}", file=sys.stderr, flush=True)
            result["failed_step"] = " ".join(str(x) for x in st)
            ok = False
            return None
        out = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"[bench_sam_to_bam] {' '.join(str(x) for x in st)}: {json.dumps(out)}", file=sys.stderr, flush=True)
        return out

    h2d = run_step("h2d")
    if ok:
        result["h2d"] = h2d
    for label, asked in (("plain", args.plain_records), ("aligner", args.aligner_records)):
        if not ok or asked <= 0:
            continue
        # the text twice (the input and the round trip's) and the BAM twice (the source and the conversion's)
        per = 2 * TEXT_PER_RECORD[label] + 2 * BAM_PER_RECORD[label]
        room = int(shutil.disk_usage(tmp.name).free * 0.9)
        n = min(asked, max(1000, room // per))
        f = {"records_asked": asked, "records": n, "scaled_down": n < asked}
        if n < asked:
            print(f"[bench_sam_to_bam] {label}: {asked} records need {asked * per / 1e9:.0f} GB and {room / 1e9:.0f} GB are free: {n} records of the same shape",
                  file=sys.stderr, flush=True)
        for st in ("make", "read", "convert", "deflate", "roundtrip"):
            out = run_step(st, label, n) if st == "make" else run_step(st, label)
            if not ok:
                break
            f[st] = out
        if ok:
            text = f["convert"]["header_bytes"] + f["convert"]["text_bytes"]
            bounds = {"h2d": text / (h2d["h2d_gbs"] * 1e9) * 1e3, "read": f["read"]["read_ms"],
                      "deflate": f["deflate"]["encoder_gpu_ms"] * f["convert"]["bam_bytes"] / f["deflate"]["in_bytes"]}
            largest = max(bounds, key=bounds.get)
            f.update({"text_gb": round(text / 1e9, 3), "bound_ms": {k: round(v, 1) for k, v in bounds.items()}, "largest_bound": largest,
                      "convert_over_bound": round(f["convert"]["convert_ms"] / bounds[largest], 3),
                      "text_gbs": round(text / f["convert"]["convert_ms"] / 1e6, 2),
                      "out_over_source_bam": round(f["convert"]["out_bytes"] / f["make"]["bam_bytes"], 3)})
        result["files"][label] = f
        for q in paths(tmp.name, label).values():
            if os.path.exists(q):
                os.remove(q)
    tmp.cleanup()
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(line + "\n")
    print(line)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
