#!/usr/bin/env python3
"""Randomised sweep of `ngs fastq` (GPU), in the manner of tools/fuzz_parity.py --consumers: random BAM files through
ngsq_bam_write_fastq in process against tests/fastq_model.py, byte for byte per output, count for count, and the planted
record's message.  tests/test_fastq_gpu.py runs a slice of it; the rest is run by hand:
    python tools/fuzz_fastq.py [--seeds 200] [--seed-base 0]
"""
import argparse
import gzip
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from ngs_amd import ffi, host  # noqa: E402
from tests import bamio  # noqa: E402
from tests import fastq_model as fm  # noqa: E402

NAMES = ["chr1", "chr2", "chr3"]
LENS = [300_000, 70_000, 5_000]
FLAG_CYCLE = [0x41, 0x81, 0xC1, 0x01, 0x141, 0x881]      # one, two, both, neither, secondary, supplementary
EOF = bamio.EOF_BLOCK


def read_batch(rng, l_seq, flags, qual_kind):
    """Unplaced records of the given lengths and flags: packed bases drawn from all 16 codes (the pad nibble of an odd length
    too), qual_kind[i] 0: scores of 0..93, 1: QUAL missing, 2: all 93."""
    l_seq = np.asarray(l_seq, dtype=np.uint32)
    n = len(l_seq)
    seq_off = np.zeros(n + 1, np.uint64)
    seq_off[1:] = np.cumsum((l_seq.astype(np.uint64) + 1) // 2)
    kinds = np.asarray(qual_kind)
    qual_off = np.zeros(n + 1, np.uint64)
    qual_off[1:] = np.cumsum(np.where(kinds == 1, 0, l_seq).astype(np.uint64))
    qual = rng.integers(0, 94, int(qual_off[-1])).astype(np.uint8)
    for i in np.flatnonzero(kinds == 2):
        qual[int(qual_off[i]):int(qual_off[i + 1])] = 93
    cols = dict(flag=np.asarray(flags, dtype=np.uint16), mapq=np.zeros(n, np.uint8), ref_id=np.full(n, -1, np.int32), pos=np.full(n, -1, np.int32),
                mate_ref_id=np.full(n, -1, np.int32), tlen=np.zeros(n, np.int32), l_seq=l_seq, n_cigar=np.zeros(n, np.uint16),
                seq=rng.integers(0, 256, int(seq_off[-1])).astype(np.uint8), seq_off=seq_off, qual=qual, qual_off=qual_off,
                cigar=np.zeros(0, np.uint32), cigar_off=np.zeros(n + 1, np.uint64))
    return host.HostBatch(n, cols, 0, 0, 0, 0)


def random_names(rng, n):
    """Names of 0 to 254 bytes, most of them short, printable, without '@' in front."""
    lens = np.where(rng.random(n) < 0.9, rng.integers(1, 40, n), rng.choice([0, 1, 63, 64, 65, 254], n))
    return [bytes(rng.integers(48, 123, int(k)).astype(np.uint8)) for k in lens]


def convert(lib, path, out_dir, *, two_files=False, other=False, tag="o", **kw):
    """host.bam_to_fastq into files of out_dir: ([bytes written per output], report)."""
    p = [os.path.join(out_dir, f"{tag}_{k}.fastq") for k in range(3)]
    for x in p:
        if os.path.exists(x):
            os.unlink(x)
    rep = host.bam_to_fastq(path, p[0], p[1] if two_files else None, p[2] if other else None, lib=lib, **kw)
    return [open(x, "rb").read() if os.path.exists(x) else b"" for x in p], rep


def model(path, *, two_files=False, other=False, exclude_flags=ffi.FASTQ_EXCLUDE_FLAGS, require_flags=0, name_suffix=False,
          default_quality=ffi.FASTQ_DEFAULT_QUALITY, max_records=0, **_ignored):
    """tests/fastq_model.expected_fastq under the wrapper's argument names (max_records 0: all)."""
    return fm.expected_fastq(path, two_files=two_files, other=other, exclude=exclude_flags, require=require_flags, suffix=name_suffix,
                             default_quality=default_quality, max_records=max_records or None)


def first_difference(got, want):
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    lo = max(want.rfind(b"\n@", 0, k + 1), 0)
    return f"byte {k} of {len(got)} / {len(want)}: got {got[lo:k + 60]!r} want {want[lo:k + 60]!r}"


def check(lib, path, out_dir, **kw):
    """Convert and hold every output, the counts and the byte totals to the model.  A BGZF output is gunzipped first and must end
    in the EOF block.  Returns (the outputs' text, report)."""
    want = model(path, **kw)
    assert not isinstance(want, str), want
    got, rep = convert(lib, path, out_dir, **kw)
    mask = kw.get("bgzf_mask", 0)
    for k in range(3):
        if mask >> k & 1:
            assert got[k].endswith(EOF) and rep["compressed_bytes"][k] == len(got[k]), (k, len(got[k]), rep["compressed_bytes"])
            got[k] = gzip.decompress(got[k])
        else:
            assert rep["compressed_bytes"][k] == 0
        assert got[k] == want[k], f"output {k}: " + first_difference(got[k], want[k])
        assert rep["text_bytes"][k] == len(want[k]), (k, rep["text_bytes"], len(want[k]))
    for key, value in want[3].items():
        assert rep[key] == value, (key, rep[key], value)
    return got, rep


def fastq_case(seed, dir):
    """One BAM file for the sweep and the options it is converted with; pure CPU, no library call.  Everything is drawn from
    default_rng(26000 + seed): 1 000 to 4 000 records of 0 to max_len bases in any of the 16 codes, every flag bit of the low
    twelve, QUAL present / missing / all 93, names of 0 to 254 bytes, blocks of 0.7 to 60 kB.  seed % 4 == 1: a score of 94
    to 255 planted in one record, kept or not."""
    rng = np.random.default_rng(26000 + seed)
    n = int(rng.integers(1000, 4001))
    max_len = int(rng.choice([1, 2, 3, 36, 150, 151, 300, 1000]))
    l_seq = rng.integers(0 if rng.random() < 0.5 else 1, max_len + 1, n)
    if rng.random() < 0.4:
        l_seq[:] = max_len
    l_seq[rng.random(n) < 0.03] = 0
    flags = rng.integers(0, 1 << 12, n)
    paired = rng.random(n) < 0.7                               # most records are a clean read one or read two
    flags[paired] = (flags[paired] & ~0xC0) | np.where(rng.random(int(paired.sum())) < 0.5, 0x40, 0x80)
    flags[rng.random(n) < 0.6] &= ~0x900                       # ... and neither secondary nor supplementary
    hb = read_batch(rng, l_seq, flags, rng.choice([0, 0, 0, 1, 2], n))
    planted = None
    if seed % 4 == 1:
        have = np.flatnonzero(np.diff(hb.cols["qual_off"].astype(np.int64)) > 0)
        if len(have):
            at = int(rng.choice(have))
            lo, hi = int(hb.cols["qual_off"][at]), int(hb.cols["qual_off"][at + 1])
            k = lo + int(rng.integers(0, hi - lo))
            if k == lo and hi - lo > 1:
                k += 1                                          # (0xFF in front would be a missing QUAL)
            hb.cols["qual"][k] = int(rng.integers(94, 255))
            planted = at
    path = os.path.join(dir, f"fastq_{seed}.bam")
    bamio.write_bam(path, hb, NAMES, LENS, block_payload=int(rng.choice([700, 4000, 60000])), with_index=False, names=random_names(rng, n),
                    level=int(rng.choice([0, 1, 6])), sort_order="unsorted")
    mode = int(rng.integers(0, 3))                              # one file, two files, two files and others
    n_out = mode + 1
    opts = dict(two_files=mode >= 1, other=mode == 2, exclude_flags=int(rng.choice([2304, 0, 0x4, 0xF00, 0x10])),
                require_flags=int(rng.choice([0, 0, 0x1, 0x40, 0x10])), name_suffix=bool(rng.integers(0, 2)),
                default_quality=int(rng.choice([0, 1, 40, 93])), batch_records=int(rng.choice([63, 64, 65, 257, 2500, 0])),
                max_records=0 if rng.random() < 2 / 3 else int(rng.integers(1, n + 6)), bgzf_mask=int(rng.integers(0, 1 << n_out)) if rng.random() < 0.4 else 0)
    return dict(path=path, n=n, max_len=max_len, planted=planted, opts=opts)


def fastq_sweep(lib, seeds, base=0, verbose=True):
    td = tempfile.mkdtemp(prefix="ngsq_fuzz_fastq_")
    try:
        for seed in range(base, base + seeds):
            case = fastq_case(seed, td)
            want = model(case["path"], **case["opts"])
            if isinstance(want, str):
                try:
                    convert(lib, case["path"], td, **case["opts"])
                except host.NgsqError as e:
                    assert e.code == ffi.ERR_INVALID_ARGUMENT and e.message == want, (seed, e.message, want)
                else:
                    raise AssertionError(f"seed {seed}: no error, the model says {want!r}")
                what = "error ok"
            else:
                _, rep = check(lib, case["path"], td, **case["opts"])
                what = f"{rep['reads_one']} + {rep['reads_two']} + {rep['reads_other']} reads in {rep['batches']} batches"
            if verbose:
                print(f"fastq seed {seed}: n={case['n']} max_len={case['max_len']} planted={case['planted']} {case['opts']}: {what}", flush=True)
            os.unlink(case["path"])
    finally:
        shutil.rmtree(td, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=40)
    ap.add_argument("--seed-base", type=int, default=0, help="first seed (a soak behind an earlier one takes up where that left off)")
    a = ap.parse_args()
    lib = ffi.load_library()
    if lib.ngsq_device_count() < 1:
        raise SystemExit("fuzz_fastq: no HIP device")
    fastq_sweep(lib, a.seeds, a.seed_base)
    print("all seeds ok")


if __name__ == "__main__":
    main()
