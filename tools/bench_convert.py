"""`ngs convert <BAM> <SAM>` on the MI355X: what the conversion costs against a bare device-ingest scan
and against the device-to-host copy of its text.

    python tools/bench_convert.py [--plain-records N] [--aligner-records N] [--cli-records N] [--reps K] [--dir D] [--out JSON]

Files: the plain file of bench.py's file leg (chr1 + chr2, 150 bp) and the aligner-shaped one of its realistic leg (the 195
@SQ of GRCh38 no-alt at full length, NGSQ_SYNTH_FILE_REALISTIC), both written by the library's synthetic writer at zlib
level 6 (tools/bench_index.py's files).  Per file, after one warm-up scan (the page cache):
  scan_ms       the device ingest alone: every batch of ngsq_bam_next_batch_device on a context without facets
  convert_ms    ngsq_bam_write_sam in process into /dev/null, with the report's split (ingest / format / copy / write)
  d2h_gbs       pinned device-to-host bandwidth in this process: copies of the library's ring piece (32 MiB) into one
                pinned buffer, back to back on one stream
  bound_ms      max(scan_ms, text bytes / d2h_gbs): what the conversion would take if the copies hid everything else
and once: cli_ms, `ngs convert` wall clock of a --cli-records aligner-shaped file into a SAM file of a temporary directory
(removed afterwards).  Medians of --reps runs.  One JSON line on stdout."""
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

from ngs_amd import build, ffi, host  # noqa: E402
from tools.bench_index import bare_scan_ms, write_file  # noqa: E402

PIECE = 32 << 20  # sam.cpp RING_PIECE


def d2h_gbs(total_bytes: int = 8 << 30) -> float:
    """Pinned D2H bandwidth: PIECE-sized hipMemcpyAsync from one device buffer into one pinned buffer, on one stream."""
    hip = C.CDLL("libamdhip64.so")
    dev, pin, st = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipSetDevice(0) == 0
    assert hip.hipMalloc(C.byref(dev), C.c_size_t(PIECE)) == 0
    assert hip.hipHostMalloc(C.byref(pin), C.c_size_t(PIECE), 0) == 0
    assert hip.hipStreamCreate(C.byref(st)) == 0
    try:
        n = max(1, total_bytes // PIECE)
        for _ in range(4):  # warm-up
            assert hip.hipMemcpyAsync(pin, dev, C.c_size_t(PIECE), 2, st) == 0
        assert hip.hipStreamSynchronize(st) == 0
        t0 = time.perf_counter()
        for _ in range(n):
            assert hip.hipMemcpyAsync(pin, dev, C.c_size_t(PIECE), 2, st) == 0   # hipMemcpyDeviceToHost
        assert hip.hipStreamSynchronize(st) == 0
        return n * PIECE / (time.perf_counter() - t0) / 1e9
    finally:
        hip.hipStreamDestroy(st)
        hip.hipHostFree(pin)
        hip.hipFree(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain-records", type=int, default=60_000_000)
    ap.add_argument("--aligner-records", type=int, default=150_000_000)
    ap.add_argument("--cli-records", type=int, default=5_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--convert-only", action="store_true", help="no bare scans and no D2H runs (a kernel trace of the conversion)")
    args = ap.parse_args()
    build.build(verbose=False)
    ngs = build.build_cli(verbose=False)
    lib = ffi.load_library()
    tmp = tempfile.TemporaryDirectory(dir=args.dir)
    med = statistics.median
    result = {"reps": args.reps, "ring_piece_bytes": PIECE, "files": {}}
    for label, n, aligner in (("plain", args.plain_records, False), ("aligner", args.aligner_records, True)):
        if n <= 0:
            continue
        path = os.path.join(tmp.name, f"{label}.bam")
        t0 = time.perf_counter()
        write_file(lib, path, n, aligner)
        write_s = time.perf_counter() - t0
        os.remove(path + ".bai")
        bare_scan_ms(lib, path)  # warm-up: the page cache, the process's block cache
        scans = [bare_scan_ms(lib, path)[0] for _ in range(0 if args.convert_only else args.reps)] or [0.0]
        conv, reps = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            rep = host.bam_to_sam(path, "/dev/null", lib=lib)
            conv.append((time.perf_counter() - t0) * 1e3)
            reps.append(rep)
            assert rep["records"] == n
        bw = [d2h_gbs() for _ in range(0 if args.convert_only else args.reps)] or [float("nan")]
        text = reps[0]["header_bytes"] + reps[0]["text_bytes"]
        copy_bound = text / (med(bw) * 1e9) * 1e3 if not args.convert_only else float("nan")
        bound = max(med(scans), copy_bound) if not args.convert_only else float("nan")
        result["files"][label] = {
            "records": n, "bytes": os.path.getsize(path), "write_s": round(write_s, 1), "text_gb": round(text / 1e9, 3),
            "text_bytes_per_record": round(text / n, 1), "batches": reps[0]["batches"],
            "scan_ms": round(med(scans), 1), "convert_ms": round(med(conv), 1),
            "convert_ingest_ms": round(med(r["scan_ms"] for r in reps), 1), "convert_format_gpu_ms": round(med(r["format_ms"] for r in reps), 1),
            "convert_copy_gpu_ms": round(med(r["copy_ms"] for r in reps), 1), "convert_write_ms": round(med(r["write_ms"] for r in reps), 1),
            "d2h_gbs": round(med(bw), 2), "copy_bound_ms": round(copy_bound, 1), "bound_ms": round(bound, 1),
            "convert_over_bound": round(med(conv) / bound, 3) if bound > 0 else None, "text_gbs": round(text / med(conv) / 1e6, 2),
            "all_ms": {"scan": [round(x, 1) for x in scans], "convert": [round(x, 1) for x in conv], "d2h_gbs": [round(x, 2) for x in bw]},
        }
        os.remove(path)
        print(f"[bench_convert] {label}: {json.dumps(result['files'][label])}", file=sys.stderr, flush=True)
    if args.cli_records > 0:
        path = os.path.join(tmp.name, "cli.bam")
        write_file(lib, path, args.cli_records, True)
        os.remove(path + ".bai")
        out = os.path.join(tmp.name, "cli.sam")
        cli = []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            r = subprocess.run([ngs, "convert", path, out], capture_output=True, text=True, timeout=1800)
            cli.append((time.perf_counter() - t0) * 1e3)
            assert r.returncode == 0, r.stderr
            size = os.path.getsize(out)
            os.remove(out)
        result["cli"] = {"records": args.cli_records, "sam_bytes": size, "cli_ms": round(med(cli[1:]), 1),
                         "all_ms": [round(x, 1) for x in cli]}
        os.remove(path)
    tmp.cleanup()
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
