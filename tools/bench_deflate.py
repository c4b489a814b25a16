"""The device DEFLATE encoder on the MI355X: its rate and its size against zlib at both efforts
(section 17.6), `ngs generate` into .fastq.gz with --gzip device against --gzip host, and the sorted BAM conversion of
tools/bench_bam_sort.py's plain file at both efforts.

    python tools/bench_deflate.py [--rate-mb N] [--size-mb N] [--pairs N] [--records N] [--sort-records N] [--reps K] [--genome-scale F]
                                  [--parent-lib SO] [--dir D] [--out JSON]

Every step that uses the GPU is a child process of its own under `timeout`, and the first step that fails ends the run:
  make          the inputs, written into --dir: the FASTQ text of `ngs generate` (read ones of --rate-mb MB), the plain BAM of
                bench.py's file leg (--records records), its SAM text from `ngs convert`, and the BAM's inflated stream
  zlib <input>  host only: the first --size-mb MB of the input through zlib levels 1, 6 and 9 at the encoder's 65280-byte block size
  rate <input> <effort>
                ngsq_bgzf_deflate_device on the first --rate-mb MB of the input at the effort (normal, high): input GB/s of the
                encoder alone (the report's GPU time of the encoder, the CRC, the scan and the pack; the copies and the wall
                clock beside it), the median of --reps runs after a warm-up; and the compressed size of the first --size-mb MB,
                whose ratios to zlib's three sizes are added to it.  Both efforts of an input run one behind the other.  With
                --parent-lib, a build of the parent commit's library runs as `parent_normal` in front of them, the same way: what
                normal effort cost before there was a choice, from the same session
  e2e <where> <effort>
                `ngs generate -n --pairs` into two .fastq.gz files with --gzip host (16 threads of zlib level 6 behind two pipes)
                and with --gzip device at both efforts, wall clock, the median of --reps runs
  sortmake, sort <effort>
                the plain file of tools/bench_bam_sort.py (--sort-records records, shuffled) as that tool makes it, and its
                conversion to a sorted BAM in process into /dev/null at the effort: wall clock and the report's split, the median
                of --reps runs after a warm-up; `parent_normal` as above
One JSON line on stdout."""
from __future__ import annotations

import argparse
import ctypes as C
import gzip
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

INPUTS = ("fastq", "sam", "bam_stream")
EFFORTS = ("normal", "high")
PARENT = "parent_normal"  # the parent commit's library, which has one effort
EFFORT_ENTRY_POINTS = ("ngsq_bgzf_set_effort", "ngsq_bgzf_effort", "ngsq_bgzf_effort_candidates")


def library(args, which):
    """This build's library, or for `parent_normal` the one at --parent-lib: a build from before the effort existed has no entry
    points for it and runs at normal effort, so the calls that set it answer OK without doing anything."""
    if which != PARENT:
        return ffi.load_library()
    raw = C.CDLL(args.parent_lib)
    absent = [n for n in EFFORT_ENTRY_POINTS if not hasattr(raw, n)]
    kept = {n: ffi.PROTOTYPES.pop(n) for n in absent}
    try:
        lib = ffi.load_library(args.parent_lib)
    finally:
        ffi.PROTOTYPES.update(kept)
    for n in absent:
        setattr(lib, n, lambda *a: 0)
    return lib


def effort_of(which):
    return "normal" if which == PARENT else which


def provider(args, d):
    return f"{os.path.join(d, 'ref.fa')}:1000:200:30:150:1"


def step_make(args, d):
    import numpy as np

    import bench
    from ngs_amd.genome_shape import grch38_no_alt
    from tools.bench_index import write_file
    lib = ffi.load_library()
    ngs = build.build_cli(verbose=False)
    names, lens, _ = grch38_no_alt()
    lens = [max(1000, int(x * args.genome_scale)) for x in lens]
    cfg = host.synth_config(1000, read_len=150, genome=lens, seq_model=ffi.SYNTH_SEQ_FROM_REFERENCE, lib=lib)
    bench.write_bench_fasta(np, lib, host, cfg, names, lens, os.path.join(d, "ref.fa"))
    want = args.rate_mb << 20
    pairs = want // 340 + 1
    r = subprocess.run([ngs, "-q", "generate", "-n", str(pairs), "--seed", "1", os.path.join(d, "one.fastq"), os.path.join(d, "two.fastq"), provider(args, d)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    os.rename(os.path.join(d, "one.fastq"), os.path.join(d, "fastq"))
    os.remove(os.path.join(d, "two.fastq"))
    bam = os.path.join(d, "plain.bam")
    write_file(lib, bam, args.records, False)
    os.remove(bam + ".bai")
    r = subprocess.run([ngs, "convert", bam, os.path.join(d, "plain.sam")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    os.rename(os.path.join(d, "plain.sam"), os.path.join(d, "sam"))
    with gzip.open(bam, "rb") as f, open(os.path.join(d, "bam_stream"), "wb") as o:
        o.write(f.read(want))
    return {k: os.path.getsize(os.path.join(d, k)) for k in INPUTS}


def step_zlib(args, d, name):
    from tests import bgzf_model as bm
    part = open(os.path.join(d, name), "rb").read(args.size_mb << 20)
    return {"in_bytes": len(part), "zlib_1": bm.zlib_size(part, 1), "zlib_6": bm.zlib_size(part, 6), "zlib_9": bm.zlib_size(part, 9)}


def step_rate(args, d, name, which):
    lib = library(args, which)
    effort = effort_of(which)
    data = open(os.path.join(d, name), "rb").read(args.rate_mb << 20)
    host.bgzf_deflate(data[:1 << 24], lib=lib, effort=effort)  # warm-up
    reps = [host.bgzf_deflate(data, eof=False, lib=lib, effort=effort)[1] for _ in range(args.reps)]
    med = statistics.median
    gpu = med(r["deflate_ms"] + r["crc_ms"] + r["pack_ms"] for r in reps)
    part = data[:args.size_mb << 20]
    mine = len(host.bgzf_deflate(part, eof=False, lib=lib, effort=effort)[0])
    return {"in_bytes": len(data), "out_bytes": reps[0]["out_bytes"], "blocks": reps[0]["blocks"], "stored_blocks": reps[0]["stored_blocks"],
            "tokens": reps[0]["tokens"], "matches": reps[0]["matches"],
            "encoder_gpu_ms": round(gpu, 2), "input_gbs": round(len(data) / gpu / 1e6, 2),
            "deflate_kernel_ms": round(med(r["deflate_ms"] for r in reps), 2), "crc_ms": round(med(r["crc_ms"] for r in reps), 2),
            "pack_ms": round(med(r["pack_ms"] for r in reps), 2), "copy_ms": round(med(r["copy_ms"] for r in reps), 2),
            "total_ms": round(med(r["total_ms"] for r in reps), 1),
            "all_encoder_gpu_ms": [round(r["deflate_ms"] + r["crc_ms"] + r["pack_ms"], 2) for r in reps],
            "size": {"in_bytes": len(part), "device": mine, "ratio": round(len(part) / mine, 3)}}


def step_sortmake(args, d):
    from tools import bench_bam_sort as bbs
    bbs.step_make(args, d, "plain", args.sort_records)
    p = bbs.paths(d, "plain")
    os.remove(p["shuf.sam"])
    return {"records": args.sort_records, "input_bytes": os.path.getsize(p["shuf.bam"])}


def step_sort(args, d, which):
    from tools import bench_bam_sort as bbs
    lib = library(args, which)
    effort = effort_of(which)
    src = bbs.paths(d, "plain")["shuf.bam"]
    host.bam_to_sorted_bam(src, "/dev/null", lib=lib, effort=effort)  # warm-up: the page cache, the process's block cache
    runs = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        r = host.bam_to_sorted_bam(src, "/dev/null", lib=lib, effort=effort)
        r["wall_ms"] = (time.perf_counter() - t0) * 1e3
        runs.append(r)
    med = statistics.median
    out = {k: runs[0][k] for k in ("records", "bam_bytes", "compressed_bytes", "blocks", "stored_blocks", "pieces")}
    out["wall_ms"] = round(med(r["wall_ms"] for r in runs), 1)
    out["all_ms"] = [round(r["wall_ms"], 1) for r in runs]
    out["split"] = {k: round(med(r[k] for r in runs), 1) for k in ("scan_ms", "keep_ms", "sort_ms", "gather_ms", "deflate_ms", "d2h_ms", "write_ms")}
    return out


def step_e2e(args, d, where, effort):
    ngs = build.build_cli(verbose=False)
    o1, o2 = os.path.join(d, f"{where}_1.fastq.gz"), os.path.join(d, f"{where}_2.fastq.gz")
    flags = ["--gzip", where] + (["--gzip-effort", effort] if where == "device" else [])
    runs = []
    for k in range(args.reps + 1):  # the first run warms the page cache of the FASTA
        t0 = time.perf_counter()
        r = subprocess.run([ngs, "-q", "generate", "-n", str(args.pairs), "--seed", "7", *flags, o1, o2, provider(args, d)],
                           capture_output=True, text=True)
        runs.append((time.perf_counter() - t0) * 1e3)
        assert r.returncode == 0, r.stderr
    size = os.path.getsize(o1) + os.path.getsize(o2)
    os.remove(o1)
    os.remove(o2)
    return {"pairs": args.pairs, "wall_ms": round(statistics.median(runs[1:]), 1), "pairs_per_s": round(args.pairs / statistics.median(runs[1:]) * 1e3, 0),
            "gz_bytes": size, "all_ms": [round(x, 1) for x in runs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate-mb", type=int, default=512)
    ap.add_argument("--size-mb", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=50_000_000)
    ap.add_argument("--records", type=int, default=5_000_000)
    ap.add_argument("--sort-records", type=int, default=60_000_000, help="records of the sorted conversion's file (0: no such step)")
    ap.add_argument("--parent-lib", default=None, help="a libngsq.so built from the parent commit, measured beside this build's")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--genome-scale", type=float, default=1.0, help="shrink every sequence (a quick look on a small box)")
    ap.add_argument("--step-seconds", type=int, default=900, help="time limit of one step")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--step", nargs="+", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        fn = {"make": step_make, "zlib": step_zlib, "rate": step_rate, "e2e": step_e2e, "sortmake": step_sortmake, "sort": step_sort}[args.step[0]]
        print(json.dumps(fn(args, args.dir, *args.step[1:])))
        return
    build.build(verbose=False)
    tmp = tempfile.TemporaryDirectory(dir=args.dir)
    lib = ffi.load_library()
    result = {"reps": args.reps, "block_input": ffi.BGZF_BLOCK_INPUT,
              "candidates": {e: lib.ngsq_bgzf_effort_candidates(host.BGZF_EFFORTS[e]) for e in EFFORTS},  # (K: the chain walked at high effort)
              "zlib": {}, "rate": {}, "e2e": {}, "sort": {}}
    which = ([PARENT] if args.parent_lib else []) + list(EFFORTS)
    steps = [("make",)]
    for k in INPUTS:
        steps += [("zlib", k)] + [("rate", k, w) for w in which]
    if args.pairs > 0:
        steps += [("e2e", "host", "normal")] + [("e2e", "device", e) for e in EFFORTS]
    if args.sort_records > 0:
        steps += [("sortmake",)] + [("sort", w) for w in which]
    ok = True
    for st in steps:
        cmd = ["timeout", "-k", "10", str(args.step_seconds), sys.executable, os.path.abspath(__file__), "--dir", tmp.name, "--rate-mb", str(args.rate_mb),
               "--size-mb", str(args.size_mb), "--pairs", str(args.pairs), "--records", str(args.records), "--reps", str(args.reps),
               "--genome-scale", str(args.genome_scale), "--sort-records", str(args.sort_records),
               *(["--parent-lib", os.path.abspath(args.parent_lib)] if args.parent_lib else []), "--step", *st]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:  # (nothing more is started on the GPU behind a step that failed)
            print(f"[bench_deflate] step {' '.join(st)} ended with {r.returncode}:\n{r.stderr[-4000:]}", file=sys.stderr, flush=True)
            result["failed_step"] = " ".join(st)
            ok = False
            break
        out = json.loads(r.stdout.strip().splitlines()[-1])
        if st[0] == "make":
            result["inputs"] = out
        elif st[0] == "sortmake":
            result["sort"]["file"] = out
        elif st[0] == "rate":
            z = result["zlib"][st[1]]
            out["size"].update({f"device_over_{k}": round(out["size"]["device"] / z[k], 4) for k in ("zlib_1", "zlib_6", "zlib_9")})
            result["rate"].setdefault(st[1], {})[st[2]] = out
        elif st[0] == "e2e":
            result["e2e"][st[1] if st[1] == "host" else f"device_{st[2]}"] = out
        else:
            result[st[0]][st[1]] = out
        print(f"[bench_deflate] {' '.join(st)}: {json.dumps(out)}", file=sys.stderr, flush=True)
    if ok:
        for k, r in result["rate"].items():
            r["high_over_normal"] = {"bytes": round(r["high"]["size"]["device"] / r["normal"]["size"]["device"], 4),
                                     "encoder_gpu_ms": round(r["high"]["encoder_gpu_ms"] / r["normal"]["encoder_gpu_ms"], 3)}
    if ok and args.pairs > 0:
        for e in EFFORTS:
            result["e2e"][f"device_{e}_over_host"] = round(result["e2e"][f"device_{e}"]["wall_ms"] / result["e2e"]["host"]["wall_ms"], 3)
    if ok and args.sort_records > 0:
        result["sort"]["high_over_normal"] = {k: round(result["sort"]["high"][k] / result["sort"]["normal"][k], 4) for k in ("wall_ms", "compressed_bytes")}
    tmp.cleanup()
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
