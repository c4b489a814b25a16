"""`ngs markdup` on the MI355X: what marking the duplicates of a BAM costs against a bare device-ingest
scan and against `ngs convert --sort coordinate` of the same file -- the same keep, the same encoder and the same writer, so
the yardstick -- on the two files of tools/bench_fastq.py, in one run.

    python tools/bench_markdup.py [--plain-records N] [--aligner-records N] [--reps K] [--parent-lib SO] [--dir D] [--out JSON]

Per file, after one warm-up scan, --reps runs each, in process, the output into /dev/null, of
  scan_ms     the device ingest alone (tools/bench_index.bare_scan_ms)
  sorted      ngsq_bam_write_sorted_bam (host.bam_to_sorted_bam), with its report's split
  markdup     ngsq_bam_mark_duplicates, with the report's split (walk, of which ingest / ends / match / mark / gather / deflate /
              copy / write), the counts, and the ends pass's rate: the QUAL bytes of the file, and all its record bytes, over ends_ms
Medians of the repeats, with the repeats.  --parent-lib: a libngsq.so built from the parent commit; `convert --sort coordinate`
and `fastq --collate` are then timed with that library and with this tree's in fresh processes, alternating, on the same file
(the check that neither slowed down: a difference inside the repeats' own spread is no difference).  One JSON line on stdout."""
from __future__ import annotations

import argparse
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

med = statistics.median
READ_LEN = 150  # of both files (host.synth_config's default and tools/bench_index.write_file's)


def spread(xs):
    return round((max(xs) - min(xs)) / med(xs), 3) if len(xs) > 1 and med(xs) > 0 else 0.0


def timed(fn, reps):
    """reps runs behind one warm-up: (wall clocks in ms, reports)."""
    wall, out = [], []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        rep = fn()
        if k:
            wall.append((time.perf_counter() - t0) * 1e3)
            out.append(rep)
    return wall, out


def sort_run(lib, path):
    return host.bam_to_sorted_bam(path, "/dev/null", lib=lib)


def collate_run(lib, path):
    return host.bam_to_fastq_collated(path, "/dev/null", "/dev/null", "/dev/null", "/dev/null", exclude_flags=0, lib=lib)


def child(lib_path, path, reps):
    """The sorted conversion and the collation with the library at lib_path (the parent's lacks the newer entry points)."""
    for name in [k for k in ffi.PROTOTYPES if "markdup" in k or "mark_duplicates" in k]:
        del ffi.PROTOTYPES[name]
    lib = ffi.load_library(lib_path)
    print(json.dumps({"sorted": [round(x, 1) for x in timed(lambda: sort_run(lib, path), reps)[0]],
                      "collate": [round(x, 1) for x in timed(lambda: collate_run(lib, path), reps)[0]]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain-records", type=int, default=60_000_000)
    ap.add_argument("--aligner-records", type=int, default=150_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libngsq.so of the parent commit: the two older commands are timed with both libraries")
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)  # LIB FILE
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.reps)
    from tools.bench_index import bare_scan_ms, write_file
    build.build(verbose=False)
    lib = ffi.load_library()
    tmp = tempfile.TemporaryDirectory(dir=args.dir)
    result = {"reps": args.reps, "bytes_per_record": lib.ngsq_markdup_bytes_per_record(), "files": {}}
    for label, n, aligner in (("plain", args.plain_records, False), ("aligner", args.aligner_records, True)):
        if n <= 0:
            continue
        path = os.path.join(tmp.name, f"{label}.bam")
        t0 = time.perf_counter()
        write_file(lib, path, n, aligner)
        write_s = time.perf_counter() - t0
        os.remove(path + ".bai")
        bare_scan_ms(lib, path)  # warm-up: the page cache, the process's block cache
        scans = [bare_scan_ms(lib, path)[0] for _ in range(args.reps)]
        swall, sreps = timed(lambda: sort_run(lib, path), args.reps)
        f = {"records": n, "bytes": os.path.getsize(path), "write_s": round(write_s, 1), "scan_ms": round(med(scans), 1),
             "scan_all_ms": [round(x, 1) for x in scans],
             "sorted": {"ms": round(med(swall), 1), "all_ms": [round(x, 1) for x in swall], "spread": spread(swall)}}
        for k in ("scan_ms", "keep_ms", "sort_ms", "gather_ms", "deflate_ms", "d2h_ms", "write_ms", "total_ms"):
            f["sorted"][k.replace("scan_ms", "ingest_ms")] = round(med(r[k] for r in sreps), 1)
        mwall, mreps = timed(lambda: host.bam_mark_duplicates(path, "/dev/null", lib=lib), args.reps)
        r0 = mreps[0]
        assert r0["records"] == n
        m = {"ms": round(med(mwall), 1), "all_ms": [round(x, 1) for x in mwall], "spread": spread(mwall)}
        for k in ffi.MARKDUP_METRICS + ("name_collisions", "batches", "sort_passes", "pieces", "blocks", "bam_bytes", "compressed_bytes"):
            m[k] = r0[k] if k in r0 else None
        m["duplication"] = round(r0["duplication"], 6)
        m["resident_gb"] = round(r0["resident_bytes"] / 1e9, 3)
        for k in ("scan_ms", "walk_ms", "ends_ms", "match_ms", "mark_ms", "gather_ms", "deflate_ms", "d2h_ms", "write_ms", "total_ms"):
            m[k.replace("scan_ms", "ingest_ms")] = round(med(r[k] for r in mreps), 1)
        ends = med(r["ends_ms"] for r in mreps)
        m.update({"markdup_over_sorted": round(med(mwall) / med(swall), 3), "markdup_over_scan": round(med(mwall) / med(scans), 3),
                  "added_ms": round(m["ends_ms"] + m["match_ms"] + m["mark_ms"], 1),
                  "ends_qual_gbs": round(n * READ_LEN / ends / 1e6, 1) if ends > 0 else None,
                  "ends_record_gbs": round((r0["bam_bytes"]) / ends / 1e6, 1) if ends > 0 else None})
        f["markdup"] = m
        if args.parent_lib:
            runs = {"parent": {"sorted": [], "collate": []}, "this": {"sorted": [], "collate": []}}
            for _ in range(2):  # alternating, each in a fresh process
                for which, so in (("parent", args.parent_lib), ("this", ffi.LIB_PATH)):
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--child", so, path],
                                         check=True, capture_output=True, text=True, timeout=1800).stdout
                    got = json.loads(out.strip().splitlines()[-1])
                    for k in ("sorted", "collate"):
                        runs[which][k] += got[k]
            f["against_parent"] = {k: {which: {"ms": round(med(runs[which][k]), 1), "all_ms": runs[which][k], "spread": spread(runs[which][k])}
                                       for which in ("parent", "this")} for k in ("sorted", "collate")}
            for k in ("sorted", "collate"):
                f["against_parent"][k]["this_over_parent"] = round(med(runs["this"][k]) / med(runs["parent"][k]), 3)
        result["files"][label] = f
        os.remove(path)
        print(f"[bench_markdup] {label}: {json.dumps(f)}", file=sys.stderr, flush=True)
    tmp.cleanup()
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
