"""`ngs fastq` on the MI355X: what writing the reads of a BAM back as FASTQ costs against a bare
device-ingest scan, against `ngs convert <BAM> <SAM>` of the same file in the same run, and against the device-to-host copy
of its text; with BGZF outputs, against the encoder alone.

    python tools/bench_fastq.py [--plain-records N] [--aligner-records N] [--reps K] [--deflate-mb M] [--dir D] [--out JSON]

Files: those of tools/bench_convert.py (tools/bench_index.py's writer).  Per file, after one warm-up scan, --reps runs each of
  scan_ms        the device ingest alone (tools/bench_index.bare_scan_ms)
  sam_ms         ngsq_bam_write_sam in process into /dev/null (what tools/bench_convert.py measures as convert_ms)
  fastq_ms       ngsq_bam_write_fastq in process, every output into /dev/null, in one-file mode ("one") and in two-file mode with
                 --other ("split"), with the report's split (ingest / format / deflate / copy / write)
  d2h_gbs        pinned device-to-host bandwidth in this process (tools/bench_convert.d2h_gbs)
  bound_ms       max(scan_ms, text bytes of all outputs / d2h_gbs), as profiles/r08_convert_bench.json states it for convert
  fastq_over_sam fastq_ms / sam_ms, with the spread (max - min) / median of both columns' own repeats beside it
and with every output as BGZF from the device encoder ("split_bgzf"): the bound is the encoder alone, its GPU time on the first
--deflate-mb MiB of the one-file text (ngsq_bgzf_deflate_device: deflate, CRC, scan and pack) scaled to the text of all outputs,
as tools/bench_sam_to_bam.py takes it.  Medians.  One JSON line on stdout."""
from __future__ import annotations

import argparse
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
from tools.bench_index import bare_scan_ms, write_file  # noqa: E402

med = statistics.median


def spread(xs):
    return round((max(xs) - min(xs)) / med(xs), 3) if len(xs) > 1 and med(xs) > 0 else 0.0


def fastq_runs(lib, path, reps, n, split=False, **kw):
    """--reps calls into /dev/null: one output, or (split) read ones, read twos and others.  (wall clocks, reports)"""
    wall, rep_list = [], []
    others = "/dev/null" if split else None
    for _ in range(reps):
        t0 = time.perf_counter()
        rep = host.bam_to_fastq(path, "/dev/null", others, others, lib=lib, **kw)
        wall.append((time.perf_counter() - t0) * 1e3)
        assert rep["records_scanned"] == n
        rep_list.append(rep)
    return wall, rep_list


def column(wall, reps):
    out = {"ms": round(med(wall), 1), "all_ms": [round(x, 1) for x in wall], "spread": spread(wall), "batches": reps[0]["batches"],
           "text_bytes": reps[0]["text_bytes"], "compressed_bytes": reps[0]["compressed_bytes"]}
    for k in ("records_scanned", "excluded", "no_sequence", "reads_one", "reads_two", "reads_other", "dropped_other", "blocks", "stored_blocks"):
        out[k] = reps[0][k]
    for k in ("scan_ms", "format_ms", "deflate_ms", "copy_ms", "write_ms"):
        out[k.replace("scan_ms", "ingest_ms")] = round(med(r[k] for r in reps), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain-records", type=int, default=60_000_000)
    ap.add_argument("--aligner-records", type=int, default=150_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--deflate-mb", type=int, default=256, help="MiB of FASTQ text the encoder-alone run compresses")
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
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
        sam, sam_reps = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            sam_reps.append(host.bam_to_sam(path, "/dev/null", lib=lib))
            sam.append((time.perf_counter() - t0) * 1e3)
        # the synthetic files hold duplicates and secondary records: exclude nothing, so that every record's read is written
        kw = dict(exclude_flags=0)
        one = fastq_runs(lib, path, args.reps, n, **kw)
        split = fastq_runs(lib, path, args.reps, n, split=True, **kw)
        bw = [d2h_gbs() for _ in range(args.reps)]
        f = {"records": n, "bytes": os.path.getsize(path), "write_s": round(write_s, 1), "scan_ms": round(med(scans), 1),
             "scan_all_ms": [round(x, 1) for x in scans], "d2h_gbs": round(med(bw), 2),
             "sam": {"ms": round(med(sam), 1), "all_ms": [round(x, 1) for x in sam], "spread": spread(sam),
                     "text_bytes": sam_reps[0]["header_bytes"] + sam_reps[0]["text_bytes"],
                     "ingest_ms": round(med(r["scan_ms"] for r in sam_reps), 1), "format_ms": round(med(r["format_ms"] for r in sam_reps), 1),
                     "copy_ms": round(med(r["copy_ms"] for r in sam_reps), 1)}}
        for name, (wall, reps) in (("one", one), ("split", split)):
            c = column(wall, reps)
            text = sum(c["text_bytes"])
            copy_bound = text / (med(bw) * 1e9) * 1e3
            c.update({"text_gb": round(text / 1e9, 3), "text_bytes_per_record": round(text / n, 1), "copy_bound_ms": round(copy_bound, 1),
                      "bound_ms": round(max(med(scans), copy_bound), 1), "fastq_over_bound": round(med(wall) / max(med(scans), copy_bound), 3),
                      "fastq_over_sam": round(med(wall) / med(sam), 3), "text_over_sam_text": round(text / f["sam"]["text_bytes"], 3)})
            f[name] = c
        # BGZF from the device encoder: the encoder alone on the head of the one-file text, scaled to all of it
        sample = os.path.join(tmp.name, "sample.fastq")
        per_record = sum(f["one"]["text_bytes"]) / n
        host.bam_to_fastq(path, sample, lib=lib, max_records=max(1, int((args.deflate_mb << 20) / per_record)), **kw)
        data = open(sample, "rb").read()
        os.remove(sample)
        host.bgzf_deflate(data[:1 << 24], eof=False, lib=lib)  # warm-up
        zreps = [host.bgzf_deflate(data, eof=False, lib=lib)[1] for _ in range(args.reps)]
        enc_ms = med(r["deflate_ms"] + r["crc_ms"] + r["pack_ms"] for r in zreps)
        wall, reps = fastq_runs(lib, path, args.reps, n, split=True, bgzf_mask=7, **kw)
        c = column(wall, reps)
        text = sum(c["text_bytes"])
        enc_bound = enc_ms * text / len(data)
        c.update({"text_gb": round(text / 1e9, 3), "compressed_gb": round(sum(c["compressed_bytes"]) / 1e9, 3),
                  "encoder_alone": {"in_bytes": len(data), "out_bytes": zreps[0]["out_bytes"], "gpu_ms": round(enc_ms, 2),
                                    "input_gbs": round(len(data) / enc_ms / 1e6, 2)},
                  "bound_ms": round(max(med(scans), enc_bound), 1), "fastq_over_bound": round(med(wall) / max(med(scans), enc_bound), 3)})
        f["split_bgzf"] = c
        result["files"][label] = f
        os.remove(path)
        print(f"[bench_fastq] {label}: {json.dumps(f)}", file=sys.stderr, flush=True)
    tmp.cleanup()
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
