"""`ngs fastq --collate` on the MI355X: what pairing the mates of a BAM by name costs against a bare
device-ingest scan and against plain `ngs fastq` in split mode, on the two files of tools/bench_fastq.py, in one run.

    python tools/bench_fastq_collate.py [--plain-records N] [--aligner-records N] [--reps K] [--parent-lib SO] [--dir D] [--out JSON]

The aligner-style file carries mates with equal names (records 2k and 2k + 1); the plain file's names are all different, so
there the match runs and pairs nothing.  Per file, after one warm-up scan, --reps runs each, in process, every output into
/dev/null, of
  scan_ms     the device ingest alone (tools/bench_index.bare_scan_ms)
  fastq       ngsq_bam_write_fastq in two-file mode with the others' file ("split" of tools/bench_fastq.py)
  collate     ngsq_bam_write_fastq_collated with all four outputs, with the report's split (walk, of which ingest / match /
              format / copy / write) and the share of kept records that paired
  d2h_gbs     pinned device-to-host bandwidth in this process (tools/bench_convert.d2h_gbs)
  expected_ms the phases do not overlap: the walk + the match + text bytes / d2h_gbs
Medians of the repeats, with the repeats.  --parent-lib: a libngsq.so built from the parent commit; plain `ngs fastq` split is
then timed with that library and with this tree's in fresh processes, alternating, on the same file (the check that the plain
command did not slow down: a difference inside the repeats' own spread is no difference).  One JSON line on stdout."""
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


def spread(xs):
    return round((max(xs) - min(xs)) / med(xs), 3) if len(xs) > 1 and med(xs) > 0 else 0.0


def plain_split(lib, path, reps, n):
    wall, rep_list = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        rep = host.bam_to_fastq(path, "/dev/null", "/dev/null", "/dev/null", exclude_flags=0, lib=lib)
        wall.append((time.perf_counter() - t0) * 1e3)
        assert rep["records_scanned"] == n
        rep_list.append(rep)
    return wall, rep_list


def child(lib_path, path, reps, n):
    """Plain split with the library at lib_path (one of another commit may lack the newer entry points): the wall clocks."""
    for name in [k for k in ffi.PROTOTYPES if "collate" in k]:
        del ffi.PROTOTYPES[name]
    lib = ffi.load_library(lib_path)
    plain_split(lib, path, 1, n)  # warm-up
    print(json.dumps([round(x, 1) for x in plain_split(lib, path, reps, n)[0]]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain-records", type=int, default=60_000_000)
    ap.add_argument("--aligner-records", type=int, default=150_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libngsq.so of the parent commit: plain split is timed with both libraries")
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)  # LIB FILE RECORDS
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.reps, int(args.child[2]))
    from tools.bench_convert import d2h_gbs
    from tools.bench_index import bare_scan_ms, write_file
    build.build(verbose=False)
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
        os.remove(path + ".bai")
        bare_scan_ms(lib, path)  # warm-up: the page cache, the process's block cache
        scans = [bare_scan_ms(lib, path)[0] for _ in range(args.reps)]
        plain_split(lib, path, 1, n)
        wall, reps = plain_split(lib, path, args.reps, n)
        f = {"records": n, "bytes": os.path.getsize(path), "write_s": round(write_s, 1), "scan_ms": round(med(scans), 1),
             "scan_all_ms": [round(x, 1) for x in scans],
             "fastq": {"ms": round(med(wall), 1), "all_ms": [round(x, 1) for x in wall], "spread": spread(wall), "text_bytes": reps[0]["text_bytes"],
                       "ingest_ms": round(med(r["scan_ms"] for r in reps), 1), "format_ms": round(med(r["format_ms"] for r in reps), 1),
                       "copy_ms": round(med(r["copy_ms"] for r in reps), 1)}}
        cwall, creps = [], []
        for k in range(args.reps + 1):  # (the first is the warm-up)
            t0 = time.perf_counter()
            rep = host.bam_to_fastq_collated(path, "/dev/null", "/dev/null", "/dev/null", "/dev/null", exclude_flags=0, lib=lib)
            if k:
                cwall.append((time.perf_counter() - t0) * 1e3)
                creps.append(rep)
            assert rep["records_scanned"] == n
        bw = [d2h_gbs() for _ in range(args.reps)]
        r0 = creps[0]
        text = sum(r0["text_bytes"])
        kept = r0["resident_records"]
        walk = med(r["walk_ms"] for r in creps)
        copy_ms = text / (med(bw) * 1e9) * 1e3
        c = {"ms": round(med(cwall), 1), "all_ms": [round(x, 1) for x in cwall], "spread": spread(cwall), "text_bytes": r0["text_bytes"],
             "text_gb": round(text / 1e9, 3), "pairs": r0["pairs"], "singletons": r0["singletons"], "ambiguous": r0["ambiguous"],
             "reads_other": r0["reads_other"], "name_collisions": r0["name_collisions"], "paired_share": round(2 * r0["pairs"] / max(kept, 1), 4),
             "resident_records": kept, "resident_gb": round(r0["resident_bytes"] / 1e9, 3), "sort_passes": r0["sort_passes"], "pieces": r0["pieces"],
             "batches": r0["batches"]}
        for k in ("scan_ms", "walk_ms", "match_ms", "format_ms", "deflate_ms", "copy_ms", "write_ms", "total_ms"):
            c[k.replace("scan_ms", "ingest_ms")] = round(med(r[k] for r in creps), 1)
        c.update({"d2h_gbs": round(med(bw), 2), "text_copy_ms": round(copy_ms, 1),
                  "expected_ms": round(walk + c["match_ms"] + copy_ms, 1), "collate_over_expected": round(med(cwall) / (walk + c["match_ms"] + copy_ms), 3),
                  "collate_over_fastq": round(med(cwall) / med(wall), 3), "match_over_walk": round(c["match_ms"] / walk, 3) if walk > 0 else None})
        f["collate"] = c
        if args.parent_lib:
            runs = {"parent": [], "this": []}
            for _ in range(2):  # alternating, each in a fresh process
                for which, so in (("parent", args.parent_lib), ("this", ffi.LIB_PATH)):
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--child", so, path, str(n)],
                                         check=True, capture_output=True, text=True, timeout=1200).stdout
                    runs[which] += json.loads(out.strip().splitlines()[-1])
            f["plain_fastq_against_parent"] = {k: {"ms": round(med(v), 1), "all_ms": v, "spread": spread(v)} for k, v in runs.items()}
            f["plain_fastq_against_parent"]["this_over_parent"] = round(med(runs["this"]) / med(runs["parent"]), 3)
        result["files"][label] = f
        os.remove(path)
        print(f"[bench_fastq_collate] {label}: {json.dumps(f)}", file=sys.stderr, flush=True)
    tmp.cleanup()
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
