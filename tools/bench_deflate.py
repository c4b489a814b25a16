"""The device DEFLATE encoder on the MI355X: its rate, its size against zlib, and `ngs generate` into
.fastq.gz with --gzip device against --gzip host.

    python tools/bench_deflate.py [--rate-mb N] [--size-mb N] [--pairs N] [--records N] [--reps K] [--genome-scale F] [--dir D] [--out JSON]

Every step that uses the GPU is a child process of its own under `timeout`, and the first step that fails ends the run:
  make          the inputs, written into --dir: the FASTQ text of `ngs generate` (read ones of --rate-mb MB), the plain BAM of
                bench.py's file leg (--records records), its SAM text from `ngs convert`, and the BAM's inflated stream
  rate <input>  ngsq_bgzf_deflate_device on the first --rate-mb MB of the input: input GB/s of the encoder alone (the report's
                GPU time of the encoder, the CRC, the scan and the pack; the copies and the wall clock beside it), the median of
                --reps runs after a warm-up; and the compressed size of the first --size-mb MB beside zlib level 1 and level 6
                at the same 65280-byte block size, computed on the host in the same process
  e2e <where>   `ngs generate -n --pairs` into two .fastq.gz files with --gzip host (the parent commit's behaviour: 16 threads of
                zlib level 6 behind two pipes) and with --gzip device, wall clock, the median of --reps runs
One JSON line on stdout."""
from __future__ import annotations

import argparse
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


def step_rate(args, d, name):
    from tests import bgzf_model as bm
    lib = ffi.load_library()
    data = open(os.path.join(d, name), "rb").read(args.rate_mb << 20)
    host.bgzf_deflate(data[:1 << 24], lib=lib)  # warm-up
    reps = [host.bgzf_deflate(data, eof=False, lib=lib)[1] for _ in range(args.reps)]
    med = statistics.median
    gpu = med(r["deflate_ms"] + r["crc_ms"] + r["pack_ms"] for r in reps)
    part = data[:args.size_mb << 20]
    mine = len(host.bgzf_deflate(part, eof=False, lib=lib)[0])
    l1, l6 = bm.zlib_size(part, 1), bm.zlib_size(part, 6)
    return {"in_bytes": len(data), "out_bytes": reps[0]["out_bytes"], "blocks": reps[0]["blocks"], "stored_blocks": reps[0]["stored_blocks"],
            "tokens": reps[0]["tokens"], "matches": reps[0]["matches"],
            "encoder_gpu_ms": round(gpu, 2), "input_gbs": round(len(data) / gpu / 1e6, 2),
            "deflate_kernel_ms": round(med(r["deflate_ms"] for r in reps), 2), "crc_ms": round(med(r["crc_ms"] for r in reps), 2),
            "pack_ms": round(med(r["pack_ms"] for r in reps), 2), "copy_ms": round(med(r["copy_ms"] for r in reps), 2),
            "total_ms": round(med(r["total_ms"] for r in reps), 1),
            "size": {"in_bytes": len(part), "device": mine, "zlib_1": l1, "zlib_6": l6, "device_over_zlib_1": round(mine / l1, 4),
                     "device_over_zlib_6": round(mine / l6, 4), "ratio": round(len(part) / mine, 3)}}


def step_e2e(args, d, where):
    ngs = build.build_cli(verbose=False)
    o1, o2 = os.path.join(d, f"{where}_1.fastq.gz"), os.path.join(d, f"{where}_2.fastq.gz")
    runs = []
    for k in range(args.reps + 1):  # the first run warms the page cache of the FASTA
        t0 = time.perf_counter()
        r = subprocess.run([ngs, "-q", "generate", "-n", str(args.pairs), "--seed", "7", "--gzip", where, o1, o2, provider(args, d)],
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--genome-scale", type=float, default=1.0, help="shrink every sequence (a quick look on a small box)")
    ap.add_argument("--step-seconds", type=int, default=900, help="time limit of one step")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--step", nargs="+", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        fn = {"make": step_make, "rate": step_rate, "e2e": step_e2e}[args.step[0]]
        print(json.dumps(fn(args, args.dir, *args.step[1:])))
        return
    build.build(verbose=False)
    tmp = tempfile.TemporaryDirectory(dir=args.dir)
    result = {"reps": args.reps, "block_input": ffi.BGZF_BLOCK_INPUT, "rate": {}, "e2e": {}}
    steps = [("make",)] + [("rate", k) for k in INPUTS] + ([("e2e", "host"), ("e2e", "device")] if args.pairs > 0 else [])
    ok = True
    for st in steps:
        cmd = ["timeout", "-k", "10", str(args.step_seconds), sys.executable, os.path.abspath(__file__), "--dir", tmp.name, "--rate-mb", str(args.rate_mb),
               "--size-mb", str(args.size_mb), "--pairs", str(args.pairs), "--records", str(args.records), "--reps", str(args.reps),
               "--genome-scale", str(args.genome_scale), "--step", *st]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:  # (nothing more is started on the GPU behind a step that failed)
            print(f"[bench_deflate] step {' '.join(st)} ended with {r.returncode}:\n{r.stderr[-4000:]}", file=sys.stderr, flush=True)
            result["failed_step"] = " ".join(st)
            ok = False
            break
        out = json.loads(r.stdout.strip().splitlines()[-1])
        if st[0] == "make":
            result["inputs"] = out
        else:
            result[st[0]][st[1]] = out
        print(f"[bench_deflate] {' '.join(st)}: {json.dumps(out)}", file=sys.stderr, flush=True)
    if ok and args.pairs > 0:
        result["e2e"]["device_over_host"] = round(result["e2e"]["device"]["wall_ms"] / result["e2e"]["host"]["wall_ms"], 3)
    tmp.cleanup()
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
