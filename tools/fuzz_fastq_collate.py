#!/usr/bin/env python3
"""Randomised sweep of `ngs fastq --collate` (GPU), in the manner of tools/fuzz_fastq.py: random BAM files whose read ones and
read twos share names in every way the rules tell apart (a pair, a lone mate, several ones or twos of one name, an other or an
excluded record of a pair's name), shuffled, through ngsq_bam_write_fastq_collated in process against
tests/fastq_collate_model.py, byte for byte per output, count for count, and the planted record's message.
tests/test_fastq_collate_gpu.py runs a slice of it; the rest is run by hand:
    python tools/fuzz_fastq_collate.py [--seeds 200] [--seed-base 0]
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
from tests import fastq_collate_model as cm  # noqa: E402
from tools.fuzz_fastq import EOF, LENS, NAMES, first_difference, random_names, read_batch  # noqa: E402

OUTPUTS = ("one", "two", "other", "single")


def convert(lib, path, out_dir, *, two_files=False, other=False, singletons=False, tag="c", **kw):
    """host.bam_to_fastq_collated into files of out_dir: ([bytes written per output, four of them], report)."""
    p = [os.path.join(out_dir, f"{tag}_{k}.fastq") for k in OUTPUTS]
    for x in p:
        if os.path.exists(x):
            os.unlink(x)
    rep = host.bam_to_fastq_collated(path, p[0], p[1] if two_files else None, p[2] if other else None, p[3] if singletons else None, lib=lib, **kw)
    return [open(x, "rb").read() if os.path.exists(x) else b"" for x in p], rep


def model(path, *, two_files=False, other=False, singletons=False, exclude_flags=ffi.FASTQ_EXCLUDE_FLAGS, require_flags=0, name_suffix=False,
          default_quality=ffi.FASTQ_DEFAULT_QUALITY, max_records=0, **_ignored):
    """tests/fastq_collate_model.expected_collated under the wrapper's argument names (max_records 0: all).  What cuts the
    work (hash_bits, batch_records, piece_records, memory_budget, bgzf_mask, effort) is ignored: it changes nothing."""
    return cm.expected_collated(path, two_files=two_files, other=other, singletons=singletons, exclude=exclude_flags, require=require_flags,
                                suffix=name_suffix, default_quality=default_quality, max_records=max_records or None)


def check(lib, path, out_dir, **kw):
    """Convert and hold every output, the counts and the byte totals to the model.  A BGZF output is gunzipped first and must end
    in the EOF block.  Returns (the outputs' text, report)."""
    want = model(path, **kw)
    assert not isinstance(want, str), want
    got, rep = convert(lib, path, out_dir, **kw)
    mask = kw.get("bgzf_mask", 0)
    for k in range(4):
        if mask >> k & 1:
            assert got[k].endswith(EOF) and rep["compressed_bytes"][k] == len(got[k]), (k, len(got[k]), rep["compressed_bytes"])
            got[k] = gzip.decompress(got[k])
        else:
            assert rep["compressed_bytes"][k] == 0
        assert got[k] == want[k], f"output {OUTPUTS[k]}: " + first_difference(got[k], want[k])
        assert rep["text_bytes"][k] == len(want[k]), (k, rep["text_bytes"], len(want[k]))
    for key, value in want[4].items():
        assert rep[key] == value, (key, rep[key], value)
    assert rep["resident_records"] == rep["reads_one"] + rep["reads_two"] + rep["reads_other"]
    assert rep["resident_records"] == 2 * rep["pairs"] + rep["singletons"] + rep["reads_other"]
    return got, rep


# what a name's records are: (flags of its records), drawn with these weights
GROUPS = [((0x41, 0x81), 60), ((0x41,), 6), ((0x81,), 6), ((0x41, 0x41, 0x81), 3), ((0x41, 0x81, 0x81), 3), ((0x41, 0x41), 2),
          ((0x41, 0x81, 0x01), 4), ((0x41, 0x81, 0xC1), 3), ((0x41, 0x981), 4), ((0x141, 0x81), 3), ((0x01,), 4), ((0x41, 0x81, 0x41, 0x81), 2)]


def paired_reads(rng, base):
    """(names, flags) of a file: every name of `base` gets the records of one of GROUPS, each reversed at random, and all
    records come in random order, as a coordinate sort leaves mates."""
    weights = np.array([w for _, w in GROUPS], float)
    pick = rng.choice(len(GROUPS), len(base), p=weights / weights.sum())
    names, flags = [], []
    for name, g in zip(base, pick):
        for f in GROUPS[g][0]:
            names.append(name)
            flags.append(f | (0x10 if rng.random() < 0.4 else 0))
    order = rng.permutation(len(names))
    return [names[k] for k in order], np.array(flags)[order]


def collate_case(seed, dir):
    """One BAM file for the sweep and the options it is converted with; pure CPU, no library call.  Everything is drawn from
    default_rng(27000 + seed): 150 to 700 names, each with the records of one of GROUPS, reversed at random, in random order;
    0 to max_len bases; names of 0 to 254 bytes, a tenth of them a neighbour of another name (one byte more, the last byte
    changed).  seed % 4 == 1: a score of 94 to 255 planted in one record, kept or not."""
    rng = np.random.default_rng(27000 + seed)
    n_names = int(rng.integers(150, 701))
    base = list(dict.fromkeys(random_names(rng, n_names)))
    for k in range(0, len(base), 10):                              # neighbours: equal length and a last byte apart, or a prefix
        nb = base[k] + b"x" if rng.random() < 0.5 or not base[k] else base[k][:-1] + bytes([base[k][-1] ^ 1])
        if len(nb) <= 254:
            base.append(nb)
    base = list(dict.fromkeys(base))
    names, flags = paired_reads(rng, base)
    n = len(names)
    max_len = int(rng.choice([1, 2, 3, 36, 150, 151, 300]))
    l_seq = rng.integers(1, max_len + 1, n)
    l_seq[rng.random(n) < 0.02] = 0
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
    path = os.path.join(dir, f"collate_{seed}.bam")
    bamio.write_bam(path, hb, NAMES, LENS, block_payload=int(rng.choice([700, 4000, 60000])), with_index=False, names=names,
                    level=int(rng.choice([0, 1, 6])), sort_order="unsorted")
    two_files = bool(rng.integers(0, 2))
    outs = [True, two_files, two_files and bool(rng.integers(0, 2)), bool(rng.integers(0, 2))]
    mask = sum(1 << k for k in range(4) if outs[k] and rng.random() < 0.5) if rng.random() < 0.4 else 0
    opts = dict(two_files=two_files, other=outs[2], singletons=outs[3], exclude_flags=int(rng.choice([2304, 2304, 0, 0x10])),
                require_flags=int(rng.choice([0, 0, 0, 0, 0x1, 0x40])), name_suffix=bool(rng.integers(0, 2)), default_quality=int(rng.choice([0, 1, 40, 93])),
                hash_bits=int(rng.choice([0, 0, 1, 3, 8, 63])), batch_records=int(rng.choice([63, 64, 65, 257, 0])),
                piece_records=int(rng.choice([1, 3, 64, 100, 0])), max_records=0 if rng.random() < 2 / 3 else int(rng.integers(1, n + 6)), bgzf_mask=mask)
    return dict(path=path, n=n, max_len=max_len, planted=planted, opts=opts)


def collate_sweep(lib, seeds, base=0, verbose=True):
    td = tempfile.mkdtemp(prefix="ngsq_fuzz_collate_")
    try:
        for seed in range(base, base + seeds):
            case = collate_case(seed, td)
            want = model(case["path"], **case["opts"])
            if isinstance(want, str):
                try:
                    got, _ = convert(lib, case["path"], td, **case["opts"])
                except host.NgsqError as e:
                    assert e.code == ffi.ERR_INVALID_ARGUMENT and e.message == want, (seed, e.message, want)
                else:
                    raise AssertionError(f"seed {seed}: no error, the model says {want!r}")
                what = "error ok"
            else:
                _, rep = check(lib, case["path"], td, **case["opts"])
                what = (f"{rep['pairs']} pairs, {rep['singletons']} singletons ({rep['ambiguous']} ambiguous), {rep['reads_other']} others, "
                        f"{rep['name_collisions']} collisions, {rep['pieces']} pieces")
            if verbose:
                print(f"collate seed {seed}: n={case['n']} max_len={case['max_len']} planted={case['planted']} {case['opts']}: {what}", flush=True)
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
        raise SystemExit("fuzz_fastq_collate: no HIP device")
    collate_sweep(lib, a.seeds, a.seed_base)
    print("all seeds ok")


if __name__ == "__main__":
    main()
