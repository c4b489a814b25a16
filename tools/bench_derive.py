"""`ngs derive instrument` on the MI355X: what the name scan costs over a bare device-ingest scan of
the same file.

    python tools/bench_derive.py [--plain-records N] [--aligner-records N] [--reps K] [--dir D] [--out JSON]

Files: the records of bench.py's file leg (chr1 + chr2, 150 bp) with an aligner's names and tags (NGSQ_SYNTH_FILE_ALIGNER: the
plain style names its reads r0, r1, ..., which are no Illumina names and end the command at the first record) and the
aligner-shaped file of its realistic leg (the 195 @SQ of GRCh38 no-alt at full length, NGSQ_SYNTH_FILE_REALISTIC), both
written by the library's synthetic writer at zlib level 6.  Per file, after one warm-up scan (the page cache):
  scan_ms       the device ingest alone: every batch of ngsq_bam_next_batch_device on a context without facets
  derive_ms     ngsq_bam_derive_instrument in process (scan + name kernel + the sets), with its ingest / kernel split
  cli_ms        `ngs derive instrument <BAM>` wall clock (process start, HIP start, everything)
Medians of --reps runs.  The document is checked once per file (NovaSeq, high).  One JSON line on stdout."""
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
from ngs_amd.genome_shape import grch38_no_alt  # noqa: E402


def write_file(lib, path, n, aligner):
    if aligner:
        names, lens, _ = grch38_no_alt()
        cfg = host.synth_config(n, read_len=150, genome=lens, file_style=ffi.SYNTH_FILE_REALISTIC,
                                seq_model=ffi.SYNTH_SEQ_FROM_REFERENCE, lib=lib)
        arr = (C.c_char_p * len(names))(*[x.encode() for x in names])
        rc = lib.ngsq_synth_write_bam_named(C.byref(cfg), arr, path.encode(), n, 6, 0)
    else:
        cfg = host.synth_config(n, file_style=ffi.SYNTH_FILE_ALIGNER)
        rc = lib.ngsq_synth_write_bam(C.byref(cfg), path.encode(), n, 6, 0)
    assert rc == 0, lib.ngsq_bam_last_error()


def bare_scan_ms(lib, path):
    """Every batch of the device ingest, nothing else (a context without facets)."""
    bam = C.c_void_p()
    assert lib.ngsq_bam_open(path.encode(), 0, C.byref(bam)) == 0
    try:
        n_refs = lib.ngsq_bam_n_refs(bam)
        import numpy as np
        lens = np.array([lib.ngsq_bam_ref_len(bam, r) for r in range(n_refs)], dtype=np.uint32)
        cfg = ffi.Config()
        cfg.struct_size = C.sizeof(ffi.Config)
        cfg.facets, cfg.device, cfg.n_refs = 0, 0, n_refs
        cfg.ref_len = lens.ctypes.data_as(ffi.u32p)
        ctx = ffi.ctx_p()
        assert lib.ngsq_create(C.byref(cfg), C.byref(ctx)) == 0
        try:
            t0 = time.perf_counter()
            b, n = ffi.Batch(), 0
            while True:
                assert lib.ngsq_bam_next_batch_device(bam, ctx, 1 << 22, C.byref(b)) == 0, lib.ngsq_bam_last_error()
                if not b.n_records:
                    break
                n += b.n_records
            ms = (time.perf_counter() - t0) * 1e3
        finally:
            lib.ngsq_destroy(ctx)
    finally:
        lib.ngsq_bam_close(bam)
    return ms, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain-records", type=int, default=60_000_000)
    ap.add_argument("--aligner-records", type=int, default=150_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    build.build(verbose=False)
    ngs = build.build_cli(verbose=False)
    lib = ffi.load_library()
    tmp = tempfile.TemporaryDirectory(dir=args.dir)
    result = {"reps": args.reps, "files": {}}
    for label, n, aligner in (("plain", args.plain_records, False), ("aligner", args.aligner_records, True)):
        if n <= 0:
            continue
        path = os.path.join(tmp.name, f"{label}.bam")
        t0 = time.perf_counter()
        write_file(lib, path, n, aligner)
        write_s = time.perf_counter() - t0
        bare_scan_ms(lib, path)  # warm-up: the page cache, the process's block cache
        scans = [bare_scan_ms(lib, path)[0] for _ in range(args.reps)]
        derive, ingest_part, kernel_part = [], [], []
        for k in range(args.reps):
            t0 = time.perf_counter()
            ins, fcs, doc, rep = host.derive_instrument(path, lib=lib)
            derive.append((time.perf_counter() - t0) * 1e3)
            ingest_part.append(rep["scan_ms"])
            kernel_part.append(rep["kernel_ms"])
            assert doc["succeeded"] and doc["instruments"] == ["NovaSeq"] and doc["confidence"] == "high", doc
        cli = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r = subprocess.run([ngs, "derive", "instrument", path], capture_output=True, text=True, timeout=1800)
            cli.append((time.perf_counter() - t0) * 1e3)
            assert r.returncode == 0 and json.loads(r.stdout) == doc, r.stderr
        med = statistics.median
        result["files"][label] = {
            "records": n, "bytes": os.path.getsize(path), "write_s": round(write_s, 1),
            "instruments": [x.decode() for x in ins], "flowcells": [x.decode() for x in fcs], "batches": rep["batches"],
            "entries": rep["entries"], "candidates": rep["candidates"],
            "scan_ms": round(med(scans), 1), "derive_ms": round(med(derive), 1), "derive_ingest_ms": round(med(ingest_part), 1),
            "derive_kernel_ms": round(med(kernel_part), 2), "cli_ms": round(med(cli), 1),
            "overhead_vs_scan": round(med(derive) / med(scans) - 1.0, 3),
            "all_ms": {"scan": [round(x, 1) for x in scans], "derive": [round(x, 1) for x in derive], "cli": [round(x, 1) for x in cli]},
        }
        os.remove(path)
        os.remove(path + ".bai")
        print(f"[bench_derive] {label}: {json.dumps(result['files'][label])}", file=sys.stderr, flush=True)
    tmp.cleanup()
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
