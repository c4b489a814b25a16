#!/usr/bin/env python3
"""Randomised sweep of `ngs markdup` (GPU), in the manner of tools/fuzz_fastq_collate.py: random BAM files whose templates are
re-drawn over a small set of sites, so that pairs and fragments share ends, with clip variants that keep the end (S, H, both, on
either strand), mates on two references, reads with unmapped mates, unpaired reads, secondary and supplementary records, names
that repeat, incoming 0x400 bits and missing QUAL, shuffled or coordinate-sorted, through ngsq_bam_mark_duplicates in process
against tests/markdup_model.py: every decompressed byte and every metric.  tests/test_markdup_gpu.py runs a slice of it, and
tests/test_markdup.py holds the model to at least one duplicate pair and one duplicate fragment per seed; the rest is run by hand:
    python tools/fuzz_markdup.py [--seeds 200] [--seed-base 0]
Also here, for the tests: a BAM writer that takes records as plain dictionaries (any CIGAR, any QUAL)."""
import argparse
import gzip
import os
import re
import shutil
import struct
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from ngs_amd import ffi, host  # noqa: E402
from tests import bamio  # noqa: E402
from tests import markdup_model as mm  # noqa: E402

NAMES = ["chr1", "chr2", "chr3"]
LENS = [300_000, 70_000, 5_000]
EOF = bamio.EOF_BLOCK
OPS = "MIDNSHP=X"


def cigar_ops(cigar):
    """"5S95M" or [(5, "S"), (95, "M")] as [(length, code)]."""
    if isinstance(cigar, str):
        cigar = [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    return [(int(n), OPS.index(op) if isinstance(op, str) else int(op)) for n, op in cigar]


def rec(name, flag, ref=0, pos=0, cigar="", qual=b"", l_seq=None, seq=None, mapq=60, mate_ref=-1, mate_pos=-1, tlen=0, aux=b""):
    """A record as the writer takes it.  qual None: QUAL missing, l_seq bases."""
    return dict(name=name, flag=flag, ref=ref, pos=pos, cigar=cigar, qual=qual, l_seq=l_seq, seq=seq, mapq=mapq, mate_ref=mate_ref,
                mate_pos=mate_pos, tlen=tlen, aux=aux)


def record_bytes(r) -> bytes:
    ops = cigar_ops(r["cigar"])
    qual = r["qual"]
    l = r["l_seq"] if qual is None else len(qual)
    q = b"\xff" * l if qual is None else bytes(qual)
    seq = r["seq"] if r["seq"] is not None else bytes((l + 1) // 2)
    assert len(seq) == (l + 1) // 2 and len(ops) <= 65535
    span = sum(n for n, c in ops if c in (0, 2, 3, 7, 8))
    pos = r["pos"]
    bin_ = bamio.reg2bin(pos, pos + max(span, 1)) & 0xFFFF if pos >= 0 else 4680
    nm = r["name"] + b"\0"
    body = struct.pack("<iiBBHHHIiii", r["ref"], pos, len(nm), r["mapq"], bin_, len(ops), r["flag"], l, r["mate_ref"], r["mate_pos"], r["tlen"])
    body += nm + b"".join(struct.pack("<I", n << 4 | c) for n, c in ops) + seq + q + r["aux"]
    return struct.pack("<I", len(body)) + body


def write_bam(path, recs, block_payload=60000, level=1, sort_order="unsorted", ref_names=NAMES, ref_lens=LENS):
    """The records in BGZF blocks of block_payload bytes, cut wherever that falls."""
    text = f"@HD\tVN:1.6\tSO:{sort_order}\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in zip(ref_names, ref_lens))
    s = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(ref_names))
    for n, l in zip(ref_names, ref_lens):
        s += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l)
    s += b"".join(record_bytes(r) for r in recs)
    with open(path, "wb") as f:
        for at in range(0, len(s), block_payload):
            f.write(bamio.bgzf_block(s[at:at + block_payload], level))
        f.write(EOF)
    return str(path)


def convert(lib, path, out_dir, tag="m", **kw):
    """host.bam_mark_duplicates into a file of out_dir: (the file's bytes, report)."""
    out = os.path.join(out_dir, f"{tag}_out.bam")
    if os.path.exists(out):
        os.unlink(out)
    rep = host.bam_mark_duplicates(path, out, lib=lib, **kw)
    return open(out, "rb").read(), rep


def model(path, *, remove=False, max_records=0, **_ignored):
    """tests/markdup_model.expected_markdup under the wrapper's argument names (max_records 0: all).  What cuts the work
    (hash_bits, batch_records, piece_bytes, memory_budget, effort) is ignored: it changes nothing."""
    return mm.expected_markdup(path, remove=remove, max_records=max_records or None)


def first_difference(got, want):
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return f"byte {k} of {len(got)} / {len(want)}: got {got[max(k - 20, 0):k + 20].hex()} want {want[max(k - 20, 0):k + 20].hex()}"


def check(lib, path, out_dir, **kw):
    """Mark and hold the decompressed output and every metric to the model.  Returns (the decompressed bytes, report)."""
    want = model(path, **kw)
    assert not isinstance(want, str), want
    raw, rep = convert(lib, path, out_dir, **kw)
    assert raw.endswith(EOF) and rep["compressed_bytes"] == len(raw), (len(raw), rep["compressed_bytes"])
    got = gzip.decompress(raw)
    assert got == want[0], first_difference(got, want[0])
    assert rep["bam_bytes"] == len(want[0])
    for key, value in want[1].items():
        assert rep[key] == value, (key, rep[key], value)
    return got, rep


SITES = 24


def markdup_case(seed, dir):
    """One BAM file for the sweep and the options it is marked with; pure CPU, no library call.  Everything is drawn from
    default_rng(28000 + seed): 500 to 1500 templates over SITES sites of three references.  A site is an unclipped end (ref, u)
    used on either strand; a read that lands on it keeps the end under a random clip variant (none, S, H, H then S)."""
    rng = np.random.default_rng(28000 + seed)
    sites = [(int(r), int(rng.integers(400, LENS[int(r)] - 400))) for r in rng.choice([0, 0, 0, 1, 2], SITES)]
    recs = []

    def qual(l):
        kind = rng.random()
        if kind < 0.05:
            return None
        if kind < 0.5:                                             # few distinct scores, so that score ties happen
            return bytes([int(rng.choice([10, 14, 15, 30]))]) * l
        return bytes(rng.integers(0, 42, l).astype(np.uint8))

    def placed(name, flag, site, reverse, **kw):
        """A read of 20 to 150 bases whose unclipped end is the site's."""
        ref, u = sites[site]
        l = int(rng.integers(20, 151))
        hard, soft = [(0, 0), (0, 0), (0, 5), (3, 0), (3, 2), (0, 19)][int(rng.integers(0, 6))]
        body = l - soft
        mid = f"{body}M" if rng.random() < 0.7 else f"{body // 2}M2I3D{body - body // 2 - 2}M" if body > 8 else f"{body}M"
        span = body + (1 if "D" in mid else 0)
        clips = (f"{hard}H" if hard else "") + (f"{soft}S" if soft else "")
        if reverse:
            back = (f"{soft}S" if soft else "") + (f"{hard}H" if hard else "")
            pos, cigar, flag = u - hard - soft - span + 1, mid + back, flag | 0x10
        else:
            pos, cigar = u + hard + soft, clips + mid
        q = qual(l)
        return rec(name, flag, ref, pos, cigar, q, l_seq=l, seq=bytes(rng.integers(0, 256, (l + 1) // 2).astype(np.uint8)), **kw)

    n_templates = int(rng.integers(500, 1501))
    for t in range(n_templates):
        name = b"t%d" % t if rng.random() < 0.97 else b"t%d" % int(rng.integers(0, max(t, 1)))     # a few names repeat
        kind = rng.random()
        old = 0x400 if rng.random() < 0.05 else 0
        a, b = int(rng.integers(0, SITES)), int(rng.integers(0, SITES))
        ra, rb = bool(rng.random() < 0.3), bool(rng.random() < 0.7)
        if kind < 0.55:                                            # a pair
            recs += [placed(name, 0x41 | old, a, ra), placed(name, 0x81, b, rb)]
            if rng.random() < 0.1:
                recs.append(placed(name, 0x41 | int(rng.choice([0x100, 0x800])), int(rng.integers(0, SITES)), False))
        elif kind < 0.75:                                          # an unpaired read
            recs.append(placed(name, old, a, ra))
        elif kind < 0.9:                                           # a read whose mate is unmapped, and the mate
            recs.append(placed(name, 0x49 | old, a, ra))
            recs.append(rec(name, 0x85, sites[a][0], sites[a][1], "", qual(30) or b"", l_seq=30))
        elif kind < 0.95:                                          # a read one whose read two is absent
            recs.append(placed(name, 0x41, a, ra))
        else:                                                      # neither one nor two, or both
            recs.append(placed(name, int(rng.choice([0x1, 0xC1])) | old, a, ra))
    order = rng.permutation(len(recs))
    recs = [recs[k] for k in order]
    sorted_order = bool(rng.integers(0, 2))
    if sorted_order:
        recs.sort(key=lambda r: (r["ref"] < 0, r["ref"], r["pos"]))
    path = os.path.join(dir, f"markdup_{seed}.bam")
    write_bam(path, recs, block_payload=int(rng.choice([700, 4000, 60000])), level=int(rng.choice([0, 1, 6])),
              sort_order="coordinate" if sorted_order else "unsorted")
    n = len(recs)
    opts = dict(remove=bool(rng.integers(0, 2)), hash_bits=int(rng.choice([0, 0, 1, 3, 8, 63])), batch_records=int(rng.choice([63, 64, 65, 257, 0])),
                piece_bytes=int(rng.choice([100, 4096, 65536, 0])), max_records=0 if rng.random() < 2 / 3 else int(rng.integers(n // 2, n + 6)),
                effort=str(rng.choice(["normal", "normal", "high"])))
    return dict(path=path, n=n, sorted=sorted_order, opts=opts)


def markdup_sweep(lib, seeds, base=0, verbose=True):
    td = tempfile.mkdtemp(prefix="ngsq_fuzz_markdup_")
    try:
        for seed in range(base, base + seeds):
            case = markdup_case(seed, td)
            _, rep = check(lib, case["path"], td, **case["opts"])
            if verbose:
                print(f"markdup seed {seed}: n={case['n']} sorted={case['sorted']} {case['opts']}: {rep['pairs']} pairs ({rep['duplicate_pairs']} duplicates), "
                      f"{rep['fragments']} fragments ({rep['duplicate_fragments']}), {rep['ambiguous']} ambiguous, {rep['name_collisions']} collisions, "
                      f"{rep['pieces']} pieces", flush=True)
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
        raise SystemExit("fuzz_markdup: no HIP device")
    markdup_sweep(lib, a.seeds, a.seed_base)
    print("all seeds ok")


if __name__ == "__main__":
    main()
