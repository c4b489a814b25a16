"""`ngs index` without a GPU: the test-side model (tests/bai_model.py) pinned on hand-worked cases
and held against the project's other BAI writer (tests/bamio.py) on random sorted files, and the command line's
refusals and messages, which all come before any GPU work."""
import ctypes as C
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

from ngs_amd import build, host
from tests import bai_model as bm
from tests import bamio
from tests.util import random_batch

NAMES = ["chr1", "chr2", "chr3"]
LENS = [300_000, 70_000, 5_000]


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def run(ngs, *args, env=None):
    return subprocess.run([ngs, *args], capture_output=True, text=True, env=env, timeout=120)


def reorder(hb, order):
    """The records of hb in the given order (HostBatch with offsets columns)."""
    recs = [hb.slice(int(i), int(i) + 1) for i in order]
    cols = {k: np.concatenate([r.cols[k] for r in recs]) for k in host.FIXED_COLUMNS}
    for data, off in (("seq", "seq_off"), ("qual", "qual_off"), ("cigar", "cigar_off")):
        cols[data] = np.concatenate([r.cols[data] for r in recs])
        cols[off] = np.concatenate([[0], np.cumsum([len(r.cols[data]) for r in recs])]).astype(np.uint64)
    return host.HostBatch(len(order), cols, 0, 0, 0, 0)


def index_sorted_batch(seed, n, lens=LENS, weird=True, max_len=150, min_len=1):
    """Random records (every flag, every CIGAR op, empty CIGARs, reads beyond LN) in coordinate order: placed records by
    (sequence, position), the unplaced ones (no sequence or no position) behind them.  seed: an integer, or a generator to
    draw from."""
    rng = seed if isinstance(seed, np.random.Generator) else np.random.default_rng(seed)
    hb = random_batch(rng, n, lens, max_len=max_len, min_len=min_len, weird=weird)
    c = hb.cols
    unplaced = (c["ref_id"] < 0) | (c["pos"] < 0)
    order = np.lexsort((np.arange(n), c["pos"], c["ref_id"], unplaced))
    placed_part = order[~unplaced[order]]
    return reorder(hb, np.concatenate([placed_part, order[unplaced[order]]]))


def chain(specs, v=1 << 16):
    """Records (ref, pos, span, flag) with contiguous chunks of 100 bytes each, starting at virtual position v."""
    out = []
    for ref, pos, span, flag in specs:
        out.append(bm.Rec(ref, pos, flag, span, v, v + 100))
        v += 100
    return out


# ---- the model on hand-worked cases ----------------------------------------------------------------------------------

def test_read_ending_exactly_at_16384():
    recs = chain([(0, 16384 - 150, 150, 0), (0, 16384, 10, 0)])
    (bins, lin), = bm.parse(bm.build(recs, 1))[0]
    assert bins[4681] == [(recs[0].v0, recs[0].v1)]            # [16234, 16384): window 0 only, leaf bin 0
    assert bins[4682] == [(recs[1].v0, recs[1].v1)]
    assert lin == [recs[0].v0, recs[1].v0]                      # window 1 belongs to the second read alone
    assert bins[bm.META_BIN] == [(recs[0].v0, recs[1].v1), (2, 0)]


def test_read_spanning_two_windows():
    recs = chain([(0, 16300, 150, 0)])
    (bins, lin), = bm.parse(bm.build(recs, 1))[0]
    assert bm.reg2bin(16300, 16450) == 585
    assert set(bins) == {585, bm.META_BIN}
    assert lin == [recs[0].v0, recs[0].v0]


def test_span0_unmapped_mate_on_a_window_boundary():
    # an unmapped mate placed at its mate's position: no reference bases -> length 1, counted as unmapped
    recs = chain([(0, 100, 150, 0), (0, 16384, 0, 0x4 | 0x1)])
    (bins, lin), = bm.parse(bm.build(recs, 1))[0]
    assert bins[4682] == [(recs[1].v0, recs[1].v1)]
    assert lin == [recs[0].v0, recs[1].v0]
    assert bins[bm.META_BIN][1] == (1, 1)


def test_interleaved_bins_do_not_merge():
    recs = chain([(0, 100, 20000, 0), (0, 200, 100, 0), (0, 300, 20000, 0), (0, 400, 100, 0), (0, 500, 100, 0)])
    (bins, lin), = bm.parse(bm.build(recs, 1))[0]
    assert bins[585] == [(recs[0].v0, recs[0].v1), (recs[2].v0, recs[2].v1)]
    assert bins[4681] == [(recs[1].v0, recs[1].v1), (recs[3].v0, recs[4].v1)]   # adjacent records of a bin: one chunk
    assert lin == [recs[0].v0, recs[0].v0]


def test_a_chunk_merges_only_when_it_starts_where_the_last_ended():
    a, b = bm.Rec(0, 100, 0, 50, 1 << 16, 2 << 16), bm.Rec(0, 120, 0, 50, (2 << 16) + 1, 3 << 16)
    (bins, _), = bm.parse(bm.build([a, b], 1))[0]
    assert bins[4681] == [(a.v0, a.v1), (b.v0, b.v1)]


def test_leading_and_interior_linear_gaps():
    recs = chain([(0, 50_000, 100, 0), (0, 100_000, 100, 0)])
    (bins, lin), = bm.parse(bm.build(recs, 1))[0]
    assert lin == [0, 0, 0, recs[0].v0, recs[0].v0, recs[0].v0, recs[1].v0]


def test_empty_file():
    assert bm.build([], 2) == b"BAI\1" + struct.pack("<i", 2) + struct.pack("<ii", 0, 0) * 2 + struct.pack("<Q", 0)


def test_unplaced_reads():
    recs = chain([(1, 10, 100, 0), (-1, -1, 0, 4), (0, -1, 0, 4), (-1, 5, 0, 4)])
    refs, n_no_coor = bm.parse(bm.build(recs, 2))
    assert n_no_coor == 3
    assert refs[0] == ({}, [])
    assert refs[1][0][bm.META_BIN] == [(recs[0].v0, recs[0].v1), (1, 0)]


def test_order_violations_name_the_record():
    with pytest.raises(bm.Unsorted) as e:
        bm.build(chain([(0, 10, 1, 0), (0, 20, 1, 0), (0, 15, 1, 0)]), 1)
    assert e.value.index == 2
    with pytest.raises(bm.Unsorted) as e:
        bm.build(chain([(1, 10, 1, 0), (0, 20, 1, 0)]), 2)
    assert e.value.index == 1
    with pytest.raises(bm.Unsorted) as e:                       # a placed record behind an unplaced one
        bm.build(chain([(0, 10, 1, 0), (-1, -1, 0, 4), (0, 30, 1, 0)]), 1)
    assert e.value.index == 2


def test_position_behind_a_block_end_is_the_next_member_even_when_empty():
    blocks = [bm.Block(0, 0, 100), bm.Block(50, 100, 0), bm.Block(78, 100, 200)]
    assert bm.pos_after(blocks, 100, 400) == 50 << 16          # the empty member, not the block with the next byte
    assert bm.pos_after(blocks, 150, 400) == 78 << 16 | 50
    assert bm.pos_after(blocks, 300, 400) == 400 << 16          # no member behind: the file size


def test_hand_spec_empty_member_separates_chunk_and_record_id():
    """tests/golden/hand_spec.bam has an empty member between two records: the chunk of the record behind it starts at
    that member (htslib's position behind the previous record), not in the block that holds the record's first byte."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hand_spec.bam")
    blocks, _, _ = bm.read_blocks(path)
    empty = {b.coff << 16 for b in blocks[:-1] if b.isize == 0}
    assert empty
    recs, _, _ = bm.read_records(path)
    assert all(recs[k].v0 == recs[k - 1].v1 for k in range(1, len(recs)))
    assert any(r.v0 in empty for r in recs)


# ---- the limit rule (include/ngsq_index.h; the message of bai.cpp) -----------------------------------------------------------

def test_window_limit_both_sides_of_the_edge():
    # LN 300 000: ceil(300000 / 16384) = 19 windows of the sequence, 64 of slack: windows 0 .. 82 are kept, [0, 83 * 16384)
    assert bm.lin_cap(300_000) == 83 and 83 * 16384 == 1_359_872
    assert bm.lin_cap(16384) == 65 and bm.lin_cap(16385) == 66 and bm.lin_cap(1) == 65
    ok = chain([(0, 100, 50, 0), (0, 1_359_872 - 10, 10, 0), (1, 5, 5, 0)])      # last base 1 359 871: window 82
    (_, lin), (_, lin1) = bm.parse(bm.build(ok, 2, ref_lens=[300_000, 70_000]))[0]
    assert len(lin) == 83 and lin[82] == ok[1].v0 and lin[81] == ok[0].v0 and lin1 == [ok[2].v0]
    with pytest.raises(bm.Limit) as e:
        bm.build(chain([(0, 100, 50, 0), (0, 1_359_872 - 10, 11, 0), (1, 5, 5, 0)]), 2, ref_lens=[300_000, 70_000])
    assert e.value.index == 1 and "record 1 (0-based) cannot be held by a BAI" in str(e.value)
    with pytest.raises(bm.Limit):                                                   # a span of 0 counts as one base
        bm.build(chain([(0, 1_359_872, 0, 0)]), 1, ref_lens=[300_000])
    bm.build(chain([(0, 1_359_871, 0, 0)]), 1, ref_lens=[300_000])
    # an N skip reaches there with a short read: 5M 1359000N 5M from 862 ends at 1 359 872
    bm.build(chain([(0, 862, 5 + 1_359_000 + 5, 0)]), 1, ref_lens=[300_000])
    with pytest.raises(bm.Limit):
        bm.build(chain([(0, 863, 5 + 1_359_000 + 5, 0)]), 1, ref_lens=[300_000])


def test_position_limit_both_sides_of_2_to_the_29():
    # LN 2^29: 32768 windows and no slack beyond the binning scheme's range
    assert bm.lin_cap(1 << 29) == 32768 and bm.lin_cap((1 << 29) - 20_000) == 32768 and bm.lin_cap(1 << 31) == 32768
    ok = chain([(0, (1 << 29) - 7, 7, 0)])
    (bins, lin), = bm.parse(bm.build(ok, 1, ref_lens=[1 << 29]))[0]
    assert len(lin) == 32768 and lin[32767] == ok[0].v0 and lin[32766] == 0 and 4681 + 32767 in bins
    for bad in ([(0, (1 << 29) - 7, 8, 0)], [(0, 1 << 29, 0, 0)], [(0, 10, 1 << 29, 0)]):
        with pytest.raises(bm.Limit) as e:
            bm.build(chain(bad), 1, ref_lens=[1 << 29])
        assert e.value.index == 0
    with pytest.raises(bm.Limit):                                                   # without the lengths the rule still holds
        bm.build(chain([(0, (1 << 29) - 7, 8, 0)]), 1)


def test_sequence_id_limit_and_the_first_record_is_named():
    bm.build(chain([(0, 1, 1, 0), (1, 1, 1, 0)]), 2, ref_lens=[100, 100])
    with pytest.raises(bm.Limit) as e:
        bm.build(chain([(0, 1, 1, 0), (1, 1, 1, 0), (2, 1, 1, 0), (2, 2, 1 << 29, 0)]), 2, ref_lens=[100, 100])
    assert e.value.index == 2
    # an unplaced record is never refused, whatever its fields say
    bm.build(chain([(0, 1, 1, 0), (-1, 1 << 30, 1 << 30, 4), (7, -1, 5, 4)]), 2, ref_lens=[100, 100])
    # an order violation anywhere in the file comes first, as the library reports it
    with pytest.raises(bm.Unsorted) as u:
        bm.build(chain([(0, 10, 1 << 29, 0), (0, 20, 1, 0), (0, 15, 1, 0)]), 1, ref_lens=[100])
    assert u.value.index == 2


# ---- the model against tests/bamio.py's writer -------------------------------------------------------------------------

@pytest.mark.parametrize("seed,n,payload", [(1, 400, 60000), (2, 3000, 4000), (3, 2000, 997), (4, 1, 60000), (5, 800, 300)])
def test_model_equals_bamio_writer_without_the_pseudo_bin(tmp_path, seed, n, payload):
    hb = index_sorted_batch(seed, n)
    path = str(tmp_path / "r.bam")
    bamio.write_bam(path, hb, NAMES, LENS, block_payload=payload, real_index=True)
    want = open(path + ".bai", "rb").read()
    got = bm.expected_bai(path)
    assert bm.strip_meta(got) == want
    refs, n_no_coor = bm.parse(got)
    c = hb.cols
    placed = (c["ref_id"] >= 0) & (c["pos"] >= 0)
    assert n_no_coor == int((~placed).sum())
    for r in range(len(NAMES)):
        sel = placed & (c["ref_id"] == r)
        meta = refs[r][0].get(bm.META_BIN)
        if not sel.any():
            assert meta is None
            continue
        unm = int(((c["flag"] & 4) != 0)[sel].sum())
        assert meta[1] == (int(sel.sum()) - unm, unm)


def test_default_files_of_the_writer_are_unchanged_by_its_new_options(tmp_path):
    """`level`, `empty_members`: a file written with the defaults has the bytes it had before the writer knew them (the
    SHA-256 values were taken from the writer as it was, on test_bamio_files_equal_the_model's recipe)."""
    before = {(11, 5000, 60000): "e07da266c2e6a280a58982b06e70eecbf4dbd0f1d53ef22a7868fc016c333342",
              (13, 3000, 500): "476451355f42ccda718c37978e1288f21dc8a2cee3cb1200a213481cdf7d7f6d"}
    for (seed, n, payload), want in before.items():
        path = str(tmp_path / "r.bam")
        bamio.write_bam(path, index_sorted_batch(seed, n), NAMES, LENS, block_payload=payload, with_index=False)
        assert hashlib.sha256(open(path, "rb").read()).hexdigest() == want


def test_writer_options_change_the_framing_only(tmp_path):
    hb = index_sorted_batch(6, 500)
    plain, opt = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    va = bamio.write_bam(plain, hb, NAMES, LENS, block_payload=900, with_index=False)
    vb = bamio.write_bam(opt, hb, NAMES, LENS, block_payload=900, with_index=False, level=0, empty_members=0.3,
                         rng=np.random.default_rng(6))
    ba, sa, _ = bm.read_blocks(plain)
    bb, sb, _ = bm.read_blocks(opt)
    assert sa == sb and len(bb) > len(ba) + 10 and sum(b.isize == 0 for b in ba) == 1
    ends, p = set(), int(vb[0]) & 0xFFFF
    while p < len(sb):
        p += 4 + struct.unpack_from("<I", sb, p)[0]
        ends.add(p)
    assert all(bb[k].out in ends and bb[k - 1].isize for k in range(1, len(bb) - 1) if bb[k].isize == 0)   # each one behind a record
    # a record's id is the block that holds its first byte, never an empty member in front of it
    empty = {b.coff for b in bb if b.isize == 0}
    assert not {int(v) >> 16 for v in vb} & empty and len(vb) == len(va) == hb.n
    starts = {b.coff: b.out for b in bb}
    assert sorted(ends | {int(vb[0]) & 0xFFFF}) == sorted({starts[int(v) >> 16] + (int(v) & 0xFFFF) for v in vb} | {len(sb)})


def test_model_rejects_the_unsorted_file(tmp_path):
    hb = index_sorted_batch(7, 300, weird=False)
    rev = reorder(hb, np.arange(hb.n)[::-1])
    path = str(tmp_path / "u.bam")
    bamio.write_bam(path, rev, NAMES, LENS, with_index=False)
    with pytest.raises(bm.Unsorted):
        bm.expected_bai(path)


# ---- the command line: everything that is refused before a GPU is touched ---------------------------------------------

def test_help_lists_index(ngs):
    r = run(ngs, "--help")
    assert r.returncode == 0 and "index" in r.stderr + r.stdout
    r = run(ngs, "index", "--help")
    assert r.returncode == 0 and "<BAM/CRAM/FASTA>" in r.stderr + r.stdout


def test_refuses_to_overwrite_an_existing_index(ngs, tmp_path):
    hb = index_sorted_batch(1, 50, weird=False)
    bam = str(tmp_path / "a.bam")
    bamio.write_bam(bam, hb, NAMES, LENS)
    before = open(bam + ".bai", "rb").read()
    r = run(ngs, "index", bam)
    assert r.returncode == 1
    assert (f"Error: refusing to overwrite existing index file: {bam}.bai. Please delete and rerun if you'd like to replace it."
            in r.stderr)
    assert open(bam + ".bai", "rb").read() == before


def header_says_sorted(lib, path):
    """ngsq_bam_sorted_by_coordinate of the file's header: the one answer the library and the command line share."""
    bam = C.c_void_p()
    assert lib.ngsq_bam_open(path.encode(), 0, C.byref(bam)) == 0, lib.ngsq_bam_last_error()
    try:
        return lib.ngsq_bam_sorted_by_coordinate(bam)
    finally:
        lib.ngsq_bam_close(bam)


# ("coordinateX": the field is read as a whole, a header that only CONTAINS SO:coordinate is not sorted)
@pytest.mark.parametrize("order", ["unsorted", "queryname", "unknown", "coordinateX", None])
def test_requires_a_coordinate_sorted_header(ngs, lib, tmp_path, order):
    hb = index_sorted_batch(2, 50, weird=False)
    good = str(tmp_path / "sorted.bam")
    bamio.write_bam(good, hb, NAMES, LENS, with_index=False)
    assert header_says_sorted(lib, good) == 1
    bam = str(tmp_path / "a.bam")
    bamio.write_bam(bam, hb, NAMES, LENS, with_index=False, sort_order=order or "coordinate")
    if order is None:   # no SO field at all
        _, data, _ = bm.read_blocks(bam)
        text_len = struct.unpack_from("<i", data, 4)[0]
        text = data[8:8 + text_len].replace(b"\tSO:coordinate", b"")
        body = data[:4] + struct.pack("<i", len(text)) + text + data[8 + text_len:]
        with open(bam, "wb") as f:
            for k in range(0, len(body), 60000):
                f.write(bamio.bgzf_block(body[k:k + 60000]))
            f.write(bamio.EOF_BLOCK)
    assert header_says_sorted(lib, bam) == 0
    r = run(ngs, "index", bam)
    assert r.returncode == 1 and "Error: the input BAM must be coordinate-sorted to be indexed" in r.stderr
    assert not os.path.exists(bam + ".bai")


def test_format_messages(ngs, tmp_path):
    for name, fmt in (("x.cram", "CRAM"), ("x.fa", "FASTA"), ("x.fasta", "FASTA")):
        p = tmp_path / name
        p.write_bytes(b">chr1\nACGT\n")
        r = run(ngs, "index", str(p))
        assert r.returncode == 1 and f"{fmt} files are indexed by the reference `ngs index` but not by this build" in r.stderr
        assert not os.path.exists(str(p) + ".bai") and not os.path.exists(str(p) + ".fai") and not os.path.exists(str(p) + ".crai")
    for name, fmt in (("x.sam", "SAM"), ("x.vcf", "VCF"), ("x.fq.gz", "Gzipped FASTQ")):
        r = run(ngs, "index", str(tmp_path / name))
        assert r.returncode == 1
        assert (f"Error: {fmt} files are not supported by this command. This may be because we haven't supported this file format "
                "yet or because it does not make sense to index a file of this kind.") in r.stderr
    r = run(ngs, "index", str(tmp_path / "x.unknown"))
    assert r.returncode == 1 and f"Error: Not able to determine bioinformatics file type for path: {tmp_path / 'x.unknown'}" in r.stderr
    r = run(ngs, "index")
    assert r.returncode == 1 and "required arguments" in r.stderr
    r = run(ngs, "-q", "index", "--bogus", "a.bam")
    assert r.returncode == 1 and "unexpected argument '--bogus' found" in r.stderr
