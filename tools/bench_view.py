"""`ngs view <BAM> <QUERY>` on the MI355X: what a region costs against the bare range scan of the same
byte ranges and against the only way to those lines without it, `ngs convert` of the whole file.

    python tools/bench_view.py [--plain-records N] [--aligner-records N] [--reps K] [--dir D] [--out JSON]

Files: those of tools/bench_convert.py (the plain file of bench.py's file leg, the aligner-shaped one of its realistic leg), with
the index the synthetic writer puts beside them.  Per file, after one warm-up scan (the page cache), in process into /dev/null:
  region_1mbp   ngsq_bam_view of 1 Mbp in the middle of the first sequence, with the report's split (view_ms: open, context
                and call, as a caller sees it; view_call_ms: the library call alone, which is what range_scan_ms times)
  chromosome    ngsq_bam_view of the whole first sequence
  range_scan_ms the bare range scan of the same merged chunks: ngsq_bam_range_begin per walk the view made (same coalescing),
                every batch of ngsq_bam_next_batch_device, nothing else
  convert_ms    ngsq_bam_write_sam of the whole file (the parent's way to the region's lines)
  full_view_ms  ngsq_bam_view without a query, to hold against convert_ms
Medians of --reps runs.  One JSON line on stdout."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ngs_amd import build, ffi, host  # noqa: E402
from tools.bench_index import bare_scan_ms, write_file  # noqa: E402

GAP = 64 << 20  # coalesce_gap, given to the view and used by the bare range scan alike


def range_scan_ms(lib, path, chunks):
    """The walks ngsq_bam_view makes for these merged chunks, without selection or text."""
    walks, k = [], 0
    while k < len(chunks):
        j = k
        while j + 1 < len(chunks) and (chunks[j + 1][0] >> 16) - (chunks[j][1] >> 16) < GAP:
            j += 1
        walks.append((chunks[k][0], chunks[j][1]))
        k = j + 1
    with host._reader_and_plain_context(lib, path, 0) as (bam, ctx):
        t0 = time.perf_counter()
        b, n = ffi.Batch(), 0
        for lo, hi in walks:
            assert lib.ngsq_bam_range_begin(bam, ctx, lo, hi) == 0, lib.ngsq_bam_last_error()
            while True:
                assert lib.ngsq_bam_next_batch_device(bam, ctx, 1 << 20, C.byref(b)) == 0, lib.ngsq_bam_last_error()
                if not b.n_records:
                    break
                n += b.n_records
        return (time.perf_counter() - t0) * 1e3, n, len(walks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain-records", type=int, default=60_000_000)
    ap.add_argument("--aligner-records", type=int, default=150_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    build.build(verbose=False)
    lib = ffi.load_library()
    tmp = tempfile.TemporaryDirectory(dir=args.dir)
    med = statistics.median
    result = {"reps": args.reps, "coalesce_gap": GAP, "files": {}}
    for label, n, aligner in (("plain", args.plain_records, False), ("aligner", args.aligner_records, True)):
        if n <= 0:
            continue
        path = os.path.join(tmp.name, f"{label}.bam")
        t0 = time.perf_counter()
        write_file(lib, path, n, aligner)
        write_s = time.perf_counter() - t0
        bam = C.c_void_p()
        assert lib.ngsq_bam_open(path.encode(), 1, C.byref(bam)) == 0
        name, ln = lib.ngsq_bam_ref_name(bam, 0).decode(), lib.ngsq_bam_ref_len(bam, 0)
        lib.ngsq_bam_close(bam)
        bare_scan_ms(lib, path)  # warm-up: the page cache, the process's block cache
        entry = {"records": n, "bytes": os.path.getsize(path), "write_s": round(write_s, 1), "sequence": name, "sequence_length": ln}
        scans = [bare_scan_ms(lib, path)[0] for _ in range(args.reps)]
        entry["scan_ms"] = round(med(scans), 1)
        for what, query in (("region_1mbp", f"{name}:{ln // 2}-{ln // 2 + 999_999}"), ("chromosome", name)):
            chunks = host.bam_query_chunks(path, query, lib=lib)[3]
            views, reps, bare = [], [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                reps.append(host.bam_view(path, "/dev/null", query=query, mode="records-only", coalesce_gap=GAP, lib=lib))
                views.append((time.perf_counter() - t0) * 1e3)
                bare.append(range_scan_ms(lib, path, chunks))
            r0 = reps[0]
            assert bare[0][1] == r0["records_scanned"] and bare[0][2] == r0["ranges"]
            entry[what] = {
                "query": query, "chunks": r0["chunks"], "ranges": r0["ranges"], "records_scanned": r0["records_scanned"],
                "records_written": r0["records_written"], "text_bytes": r0["text_bytes"],
                "view_ms": round(med(views), 1), "view_call_ms": round(med(r["total_ms"] for r in reps), 1), "range_scan_ms": round(med(x[0] for x in bare), 1),
                "view_over_range_scan": round(med(views) / med(x[0] for x in bare), 3),
                "ingest_ms": round(med(r["scan_ms"] for r in reps), 1), "select_gpu_ms": round(med(r["select_ms"] for r in reps), 2),
                "format_gpu_ms": round(med(r["format_ms"] for r in reps), 1), "copy_gpu_ms": round(med(r["copy_ms"] for r in reps), 1),
                "all_ms": {"view": [round(x, 1) for x in views], "range_scan": [round(x[0], 1) for x in bare]},
            }
        conv, full = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            rep = host.bam_to_sam(path, "/dev/null", lib=lib)
            conv.append((time.perf_counter() - t0) * 1e3)
            assert rep["records"] == n
            t0 = time.perf_counter()
            rep = host.bam_view(path, "/dev/null", lib=lib)
            full.append((time.perf_counter() - t0) * 1e3)
            assert rep["records_written"] == n
        entry.update(convert_ms=round(med(conv), 1), full_view_ms=round(med(full), 1), full_view_over_convert=round(med(full) / med(conv), 3),
                     convert_over_region_1mbp=round(med(conv) / entry["region_1mbp"]["view_ms"], 1),
                     convert_over_chromosome=round(med(conv) / entry["chromosome"]["view_ms"], 2),
                     all_ms={"scan": [round(x, 1) for x in scans], "convert": [round(x, 1) for x in conv], "full_view": [round(x, 1) for x in full]})
        result["files"][label] = entry
        os.remove(path)
        print(f"[bench_view] {label}: {json.dumps(entry)}", file=sys.stderr, flush=True)
    tmp.cleanup()
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
