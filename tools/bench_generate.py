"""`ngs generate` on the MI355X: what drawing and writing read pairs costs against the device-to-host
copy of their text.

    python tools/bench_generate.py [--pairs N] [--gz-pairs N] [--read-len L] [--reps K] [--genome-scale F] [--dir D] [--out JSON]

The FASTA is the GRCh38-shaped, soft-masked stand-in of bench.py's cli_all_facets leg (write_bench_fasta: the 195 sequences of
the no-alt analysis set at full length, 60 bases a line, about half of it lower case), written here by the same function.  One
provider, PATH:1000:200:30:<L>:1.  In process, both files into /dev/null:
  load_s        ngsq_generate_load: the FASTA's text to the device and its letters there (once)
  run_ms        ngsq_generate_write of --pairs pairs, with the report's split: draw (k_gen_draw and the offsets scan), format
                (k_gen_write), copy (device to host, both files), write (write(2), both files)
  d2h_gbs       pinned device-to-host bandwidth in this process (tools/bench_convert.py: copies of the ring piece, one stream)
  bound_ms      text bytes of both files / d2h_gbs: what the run would take if the copies hid everything else
  gz            the same call with --gz-pairs pairs through the two gzip pipes (host deflate, zlib level 6, 8 threads a file)
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
from tools.bench_convert import d2h_gbs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=50_000_000)
    ap.add_argument("--gz-pairs", type=int, default=2_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--genome-scale", type=float, default=1.0, help="shrink every sequence (a quick look on a small box)")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import numpy as np

    import bench
    from ngs_amd.genome_shape import grch38_no_alt
    build.build(verbose=False)
    lib = ffi.load_library()
    names, lens, _ = grch38_no_alt()
    lens = [max(1000, int(x * args.genome_scale)) for x in lens]
    med = statistics.median
    tmp = tempfile.TemporaryDirectory(dir=args.dir)
    fa = os.path.join(tmp.name, "GRCh38_stand_in.fa")
    cfg = host.synth_config(1000, read_len=args.read_len, genome=lens, seq_model=ffi.SYNTH_SEQ_FROM_REFERENCE, lib=lib)
    t0 = time.perf_counter()
    fa_bytes = bench.write_bench_fasta(np, lib, host, cfg, names, lens, fa)
    made_s = time.perf_counter() - t0
    L = args.read_len
    spec = [(fa, 1000, 200.0, 30.0, L, 1)]
    result = {"reps": args.reps, "pairs": args.pairs, "read_length": L, "provider": f"<fasta>:1000:200:30:{L}:1",
              "fasta": "195 sequences, 60 bases per line, soft-masked (half of it lower case), no .fai", "fasta_bytes": fa_bytes,
              "fasta_write_s": round(made_s, 1)}
    null = os.open("/dev/null", os.O_WRONLY)
    with host.Generator(spec, lib=lib) as g:
        t0 = time.perf_counter()
        g.load()
        result["load_s"] = round(time.perf_counter() - t0, 2)
        g.write_fds(null, null, 1, min(args.pairs, 1 << 20))  # warm-up: the rings, the device buffers
        runs, reps = [], []
        for k in range(args.reps):
            t0 = time.perf_counter()
            rep = g.write_fds(null, null, 100 + k, args.pairs)
            runs.append((time.perf_counter() - t0) * 1e3)
            reps.append(rep)
            assert rep["pairs"] == args.pairs
        bw = [d2h_gbs() for _ in range(args.reps)]
        text = reps[0]["text_bytes_one"] + reps[0]["text_bytes_two"]
        bound = text / (med(bw) * 1e9) * 1e3
        attempts = reps[0]["pairs"] + reps[0]["rejected_start"] + reps[0]["rejected_end"] + reps[0]["rejected_base"]
        result.update({
            "text_gb": round(text / 1e9, 3), "text_bytes_per_pair": round(text / args.pairs, 1), "batches": reps[0]["batches"],
            "attempts_per_pair": round(attempts / args.pairs, 4),
            "run_ms": round(med(runs), 1), "pairs_per_s": round(args.pairs / med(runs) * 1e3, 0),
            "draw_gpu_ms": round(med(r["draw_ms"] for r in reps), 1), "format_gpu_ms": round(med(r["format_ms"] for r in reps), 1),
            "copy_gpu_ms": round(med(r["copy_ms"] for r in reps), 1), "write_ms": round(med(r["write_ms"] for r in reps), 1),
            "d2h_gbs": round(med(bw), 2), "bound_ms": round(bound, 1), "run_over_bound": round(med(runs) / bound, 3),
            "text_gbs": round(text / med(runs) / 1e6, 2),
            "all_ms": {"run": [round(x, 1) for x in runs], "d2h_gbs": [round(x, 2) for x in bw]},
        })
        print(f"[bench_generate] plain: {json.dumps(result)}", file=sys.stderr, flush=True)
        if args.gz_pairs > 0:
            gz = []
            for k in range(args.reps):
                pipes = []
                for _ in range(2):
                    p, wfd = C.c_void_p(), C.c_int()
                    assert lib.ngsq_gzip_pipe_open(null, 8, C.byref(p), C.byref(wfd)) == 0
                    pipes.append((p, wfd.value))
                t0 = time.perf_counter()
                rep = g.write_fds(pipes[0][1], pipes[1][1], 100 + k, args.gz_pairs)
                for p, wfd in pipes:
                    os.close(wfd)
                    assert lib.ngsq_gzip_pipe_close(p) == 0
                gz.append((time.perf_counter() - t0) * 1e3)
            gtext = rep["text_bytes_one"] + rep["text_bytes_two"]
            result["gz"] = {"pairs": args.gz_pairs, "run_ms": round(med(gz), 1), "pairs_per_s": round(args.gz_pairs / med(gz) * 1e3, 0),
                            "text_gbs": round(gtext / med(gz) / 1e6, 3), "threads": 16, "zlib_level": 6, "all_ms": [round(x, 1) for x in gz]}
    os.close(null)
    tmp.cleanup()
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
