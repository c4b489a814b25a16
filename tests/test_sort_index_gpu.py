"""`ngs convert --gzip device --sort coordinate --write-index` on the GPU.  Every case holds the written
`.bai` byte for byte against two references -- tests/bai_model.expected_bai of the written BAM, and this project's `ngs index`
(host.build_bam_index) of the same file -- and the BAM against the output of the unindexed call.  The cases: the smallest files,
reversed order at the edges of a wave, a block and a sort tile, records that end exactly at and straddle the ends of BGZF blocks
and of pieces, the seams of the index pass's tiles, the span rules, the long-CIGAR placeholder, the limits, the SAM route, the
chain convert --write-index, view through the command line, and a random sweep."""
import gzip
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from ngs_amd import build, ffi, host
from ngs_amd.genome_shape import grch38_no_alt
from tests import bai_model as bm
from tests import bam_sort_model as bsm
from tests import bam_text_model as tm
from tests import bamio
from tests import view_model as vm
from tests.test_bam_sort import stream
from tests.test_bam_sort_gpu import bam_of
from tests.test_convert_gpu import write_long_reads
from tests.test_sam_sort_gpu import shuffled
from tests.test_sam_to_bam import HEAD, NAMES, random_sam
from tests.test_sam_to_bam_gpu import line
from tests.util import random_batch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLOCK = 65280   # input bytes of a BGZF block of the device encoder
LIMIT_TEXT = ("cannot be held by a BAI: its sequence id is out of range, or it reaches beyond position 2^29 or more than 1 Mbp beyond "
              "its @SQ LN")
M, I, D, N, S, EQ, X = 0, 1, 2, 3, 4, 7, 8


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def rec(ref, pos, ops=((10, M),), flag=0, size=None, name=b"r", aux=b""):
    """A whole BAM record without bases: the CIGAR `ops` of (length, operation), its bin from its span.  size: the record's bytes,
    block_size included, reached by the length of its name."""
    span = sum(l for l, op in ops if op in (M, D, N, EQ, X))
    bin_ = bm.reg2bin(pos, pos + max(span, 1)) if ref >= 0 and 0 <= pos and pos + max(span, 1) <= bm.MAX_POS else 4680
    if size is not None:
        name = (name * size)[:size - 4 - 32 - 1 - 4 * len(ops) - len(aux)]
        assert 1 <= len(name) <= 254
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name) + 1, 0, bin_, len(ops), flag, 0, -1, -1, 0) + name + b"\0"
    body += b"".join(struct.pack("<I", l << 4 | op) for l, op in ops) + aux
    out = struct.pack("<I", len(body)) + body
    assert size is None or len(out) == size
    return out


def bam_with(refs, recs, payload=65280):
    text = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n, l) for n, l in refs)
    return tm.bam_file(stream(text, refs, recs), payload)


REFS3 = [(b"chr1", 300_000), (b"chr2", 70_000), (b"chr3", 5_000)]


def held(out: str, bai: bytes, lib, tmp_path):
    """The two references of the index of the BAM at `out`."""
    assert bai == bm.expected_bai(out), "the index differs from tests/bai_model.py"
    other = str(tmp_path / "by_ngs_index.bai")
    if os.path.exists(other):
        os.remove(other)
    rep = host.build_bam_index(out, bai_path=other, lib=lib)
    assert bai == open(other, "rb").read(), "the index differs from `ngs index` of the same file"
    return rep


def indexed(lib, bam: bytes, tmp_path, name="o", tile=0, **kw):
    """Sort without and with the index; the index's bytes, the two reports and the sorted file's path."""
    src, plain, out = str(tmp_path / (name + ".in.bam")), str(tmp_path / (name + ".plain.bam")), str(tmp_path / (name + ".bam"))
    with open(src, "wb") as f:
        f.write(bam)
    if os.path.exists(out + ".bai"):
        os.remove(out + ".bai")
    host.bam_to_sorted_bam(src, plain, lib=lib, **kw)
    rep, irep = host.bam_to_sorted_bam(src, out, lib=lib, bai_path=out + ".bai", index_tile_records=tile, **kw)
    assert open(out, "rb").read() == open(plain, "rb").read(), "the BAM differs from the unindexed call's"
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith(name + ".bam")) == [name + ".bam", name + ".bam.bai"]
    bai = open(out + ".bai", "rb").read()
    by_index = held(out, bai, lib, tmp_path)
    assert {k: irep[k] for k in ("records", "n_no_coor", "runs", "bins")} == {k: by_index[k] for k in ("records", "n_no_coor", "runs", "bins")}
    assert irep["records"] == rep["records"]
    return bai, rep, irep, out


def indexed_sam(lib, sam: bytes, tmp_path, name="s", tile=0, **kw):
    src, plain, out = str(tmp_path / (name + ".sam")), str(tmp_path / (name + ".plain.bam")), str(tmp_path / (name + ".bam"))
    with open(src, "wb") as f:
        f.write(sam)
    if os.path.exists(out + ".bai"):
        os.remove(out + ".bai")
    host.sam_to_sorted_bam(src, plain, lib=lib, **kw)
    rep, irep = host.sam_to_sorted_bam(src, out, lib=lib, bai_path=out + ".bai", index_tile_records=tile, **kw)
    assert open(out, "rb").read() == open(plain, "rb").read(), "the BAM differs from the unindexed call's"
    bai = open(out + ".bai", "rb").read()
    by_index = held(out, bai, lib, tmp_path)
    assert irep["records"] == rep["records"] == by_index["records"] and irep["n_no_coor"] == by_index["n_no_coor"]
    return bai, rep, irep, out


UNPLACED = lambda k: line(f0=f"u{k}", f1="77", f2="*", f3="0", f4="0", f5="*", f6="*", f7="0", f9="NNNN", f10="&&&&")
MIX = [UNPLACED(0), UNPLACED(1), line(f0="a", f2="chr2", f3="40"), line(f0="b", f3="30"), UNPLACED(2), line(f0="zero", f3="0"),
       line(f0="c", f3="1"), line(f0="d", f2="chr3", f3="5000"), UNPLACED(3), line(f0="zero2", f2="chr2", f3="0"), line(f0="e", f3="30"), UNPLACED(4)]


# ---- 1. the smallest files ------------------------------------------------------------------------------------------------------
def test_zero_one_and_two_records(gpu_lib, tmp_path):
    bai, _, irep, _ = indexed(gpu_lib, bam_of(HEAD.encode()), tmp_path)
    assert bai == b"BAI\1" + struct.pack("<i", 3) + struct.pack("<ii", 0, 0) * 3 + struct.pack("<Q", 0)     # n_ref empty sequences, n_no_coor 0
    assert irep["records"] == 0 and irep["runs"] == 0
    bai, _, irep, _ = indexed(gpu_lib, bam_of((HEAD + line(f0="only")).encode()), tmp_path)
    assert irep["records"] == 1 and irep["runs"] == 1 and bm.parse(bai)[1] == 0
    for a, b in (("9", "5"), ("5", "9"), ("5", "5"), ("5", "20000")):
        _, _, irep, _ = indexed(gpu_lib, bam_of((HEAD + line(f0="first", f3=a) + line(f0="second", f3=b)).encode()), tmp_path)
        assert irep["records"] == 2 and irep["runs"] == (2 if b == "20000" else 1)


def test_unplaced_records_only_and_the_mix(gpu_lib, tmp_path):
    bai, _, irep, _ = indexed(gpu_lib, bam_of((HEAD + "".join(UNPLACED(k) for k in range(5))).encode()), tmp_path)
    assert irep["n_no_coor"] == 5 and bm.parse(bai) == ([({}, [])] * 3, 5)
    bai, _, irep, _ = indexed(gpu_lib, bam_of((HEAD + "".join(MIX)).encode()), tmp_path)       # chr1 POS 0 counts in n_no_coor only
    assert irep["records"] == 12 and irep["n_no_coor"] == 7


# ---- 2. reversed order: one past a wave, a block, a tile of the sort --------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 257, 4097])
def test_reversed_order(gpu_lib, tmp_path, n):
    lines = [line(f"XN:i:{k}", f0=f"q{k}", f2=NAMES[k * 3 // n], f3=str(1 + k * 7)) for k in range(n)]
    _, _, irep, _ = indexed(gpu_lib, bam_of((HEAD + "".join(reversed(lines))).encode()), tmp_path)
    assert irep["records"] == n and irep["n_no_coor"] == 0


# ---- 3. the ends of blocks and of pieces --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [120, 119, 121])
def test_records_at_and_across_block_and_piece_ends(gpu_lib, tmp_path, size):
    """65280 = 544 x 120: with records of 120 bytes one ends exactly at every block's end, and with pieces of one or two blocks
    at every piece's end; 119 and 121 bytes and the other piece sizes make records straddle both."""
    n = 544 * 3 + 9
    recs = [rec(k * 3 // n, 10 + (k % (n // 3 + 1)) * 37, size=size, name=b"n%d" % k) for k in range(n)]
    assert size != 120 or BLOCK % len(recs[0]) == 0
    bam = bam_with(REFS3, list(reversed(recs)))
    for piece in (BLOCK, 2 * BLOCK, BLOCK + 1, 65536, 0):
        _, rep, irep, _ = indexed(gpu_lib, bam, tmp_path, piece_bytes=piece)
        assert irep["records"] == n and rep["pieces"] == (1 if piece == 0 else -(-n * size // piece))
    small = bam_with(REFS3, list(reversed(recs[:300])))
    _, rep, _, _ = indexed(gpu_lib, small, tmp_path, piece_bytes=97)
    assert rep["pieces"] == -(-300 * size // 97)


def test_reads_longer_than_a_block_and_than_a_piece(gpu_lib, tmp_path):
    src = str(tmp_path / "l.bam")
    write_long_reads(src)
    data = gzip.decompress(open(src, "rb").read())
    recs = bsm.split(data)[2]
    assert max(len(r) for r in recs) > 2 * 65536
    bam = tm.bam_file(data[:len(data) - sum(len(r) for r in recs)] + b"".join(reversed(recs)), 60000)
    for piece in (65536, 0):                                                      # a read longer than a piece; longer than a block
        _, _, irep, _ = indexed(gpu_lib, bam, tmp_path, piece_bytes=piece)
        assert irep["records"] == len(recs) and irep["n_no_coor"] == 1


# ---- 4. the seams of the index pass's tiles ------------------------------------------------------------------------------------------
def test_tile_seams(gpu_lib, tmp_path):
    """300 records; in sorted order 0-127 lie on chr1, 128-255 on chr2, 256-299 are unplaced: a tile of 64 has the sequence change
    and the first unplaced record exactly at seams, and the run of window 1 (records 55-109) across the seam at 64."""
    recs = [rec(0, k * 300, name=b"a%d" % k) for k in range(128)] + [rec(1, k * 300, name=b"b%d" % k) for k in range(128)]
    recs += [rec(-1, -1, ops=(), flag=4, name=b"u%d" % k) for k in range(44)]
    assert bm.reg2bin(54 * 300, 54 * 300 + 10) != bm.reg2bin(55 * 300, 55 * 300 + 10) == bm.reg2bin(109 * 300, 109 * 300 + 10)
    order = list(range(300))
    random.Random(5).shuffle(order)
    bam = bam_with(REFS3, [recs[k] for k in order])
    want = None
    for tile in (1, 63, 64, 65, 256, 0):
        bai, _, irep, _ = indexed(gpu_lib, bam, tmp_path, tile=tile)
        assert irep["records"] == 300 and irep["n_no_coor"] == 44
        assert want is None or bai == want                                        # (the tile is no part of the result)
        want = bai


# ---- 5. spans -----------------------------------------------------------------------------------------------------------------------
def test_spans_windows_and_bins(gpu_lib, tmp_path):
    refs = [(b"big", 1 << 29), (b"none1", 1000), (b"mid", 100_000), (b"none2", 40_000), (b"short", 5_000)]
    recs = []
    for shift in (14, 17, 20, 23, 26):                                            # a window edge, and a bin edge of every level
        edge = 3 << shift
        recs += [rec(0, edge - 50, ((100, M),)), rec(0, edge - 100, ((100, M),)), rec(0, edge, ((100, M),)), rec(0, edge - 1, ((1, M),)),
                 rec(0, edge - 1, ((2, M),)), rec(0, edge - 30, ((10, M), (5, I), (30, N), (10, EQ), (4, S))), rec(0, edge - 30, ((10, M), (5, D), (10, X), (40, S)))]
    recs += [rec(0, 16383, (), flag=0x4 | 0x1 | 0x40), rec(0, 16384, (), flag=0x4 | 0x1 | 0x40), rec(0, 16383, ((36, S),), flag=0x49)]      # zero span: length 1
    recs += [rec(2, 500, ((50, M),), flag=0x4), rec(2, 500, ((50, M),)), rec(2, 70_000, ((40_000, N), (10, M))), rec(2, 0, ((1, M),))]      # placed, flag 0x4
    recs += [rec(4, 5_000 + 500_000, ((100, M),)), rec(4, 1_064_000, ((900, M),)), rec(4, 4_990, ((20, M),)), rec(4, 20_000, (), flag=0x4)]  # behind LN
    recs += [rec(0, (1 << 29) - 100, ((100, M),)), rec(0, (1 << 29) - 1, ())]    # the last position the BAI holds
    assert (1_064_000 + 900 - 1) >> 14 == bm.lin_cap(5_000) - 1
    random.Random(6).shuffle(recs)
    bai, _, irep, _ = indexed(gpu_lib, bam_with(refs, recs), tmp_path, tile=7)
    parsed, n_no_coor = bm.parse(bai)
    assert n_no_coor == 0 and parsed[1] == ({}, []) and parsed[3] == ({}, []) and parsed[0][0] and parsed[2][0] and parsed[4][0]
    crossing = {bm.reg2bin((3 << shift) - 50, (3 << shift) + 50) for shift in (14, 17, 20, 23, 26)}
    assert crossing == {585, 73, 9, 1, 0} and crossing <= set(parsed[0][0])       # one bin of every level above the windows'
    assert parsed[2][0][bm.META_BIN][1] == (3, 1)                                 # mapped, unmapped


# ---- 6. the long-CIGAR placeholder and every operation ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hand_longcigar.bam", "hand_spec.bam"])
def test_hand_files_in_reversed_order(gpu_lib, tmp_path, name):
    data = gzip.decompress(open(os.path.join(GOLDEN, name), "rb").read())
    recs = bsm.split(data)[2]
    bam = tm.bam_file(data[:len(data) - sum(len(r) for r in recs)] + b"".join(reversed(recs)), 5000)
    for tile in (0, 1):
        _, _, irep, _ = indexed(gpu_lib, bam, tmp_path, tile=tile)
        assert irep["records"] == len(recs)


# ---- 7. limits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["beyond 2^29", "1 Mbp past LN"])
def test_a_record_the_index_cannot_hold_is_refused_before_the_first_byte(gpu_lib, tmp_path, which):
    refs = [(b"big", (1 << 30)), (b"short", 5_000)]
    bad = rec(0, (1 << 29) - 10, ((100, M),)) if which == "beyond 2^29" else rec(1, 1_064_900, ((100, M),))
    last_ok = rec(1, 1_064_000, ((960, M),))
    recs = [bad, rec(0, 7), rec(1, 9), last_ok, rec(-1, -1, (), flag=4), rec(0, 5)]
    at = 2 if which == "beyond 2^29" else 4                                      # its index in the sorted output, not in the input
    src, out = str(tmp_path / "in.bam"), str(tmp_path / "o.bam")
    open(src, "wb").write(bam_with(refs, recs))
    with pytest.raises(host.NgsqError) as e:
        host.bam_to_sorted_bam(src, out, lib=gpu_lib, bai_path=out + ".bai")
    assert e.value.code == ffi.ERR_LIMIT
    assert e.value.message == f"reading BAM record: record {at} (0-based) of the sorted output {LIMIT_TEXT}"
    assert os.path.getsize(out) == 0 and sorted(os.listdir(tmp_path)) == ["in.bam", "o.bam"]
    host.bam_to_sorted_bam(src, out, lib=gpu_lib)                                 # without the index the file is written, and `ngs index` refuses it
    with pytest.raises(host.NgsqError) as e:
        host.build_bam_index(out, lib=gpu_lib)
    assert e.value.code == ffi.ERR_LIMIT and f"record {at} (0-based) {LIMIT_TEXT}" in e.value.message
    indexed(gpu_lib, bam_with(refs, recs[1:]), tmp_path, name="ok")               # the others are held
    # the SAM route: its own prefix, the same rule on @SQ LN
    sam = "@HD\tVN:1.6\n@SQ\tSN:big\tLN:1073741824\n@SQ\tSN:short\tLN:5000\n" + line(f0="ok", f2="short", f3="9") + (
        line(f0="bad", f2="big", f3=str((1 << 29) - 9), f5="100M", f9="*", f10="*") if which == "beyond 2^29"
        else line(f0="bad", f2="short", f3="1064901", f5="100M", f9="*", f10="*")) + line(f0="ok2", f2="big", f3="5")
    ssrc, sout = str(tmp_path / "in.sam"), str(tmp_path / "s.bam")
    open(ssrc, "w").write(sam)
    with pytest.raises(host.NgsqError) as e:
        host.sam_to_sorted_bam(ssrc, sout, lib=gpu_lib, bai_path=sout + ".bai")
    assert e.value.code == ffi.ERR_LIMIT
    assert e.value.message == f"reading SAM record: record {1 if which == 'beyond 2^29' else 2} (0-based) of the sorted output {LIMIT_TEXT}"
    assert os.path.getsize(sout) == 0 and not os.path.exists(sout + ".bai")


def test_an_existing_index_is_refused_by_the_library(gpu_lib, tmp_path):
    src, out = str(tmp_path / "in.bam"), str(tmp_path / "o.bam")
    open(src, "wb").write(bam_of((HEAD + line()).encode()))
    open(out + ".bai", "wb").write(b"kept")
    with pytest.raises(host.NgsqError) as e:
        host.bam_to_sorted_bam(src, out, lib=gpu_lib, bai_path=out + ".bai")
    assert e.value.code == ffi.ERR_INVALID_ARGUMENT
    assert e.value.message == f"refusing to overwrite existing index file: {out}.bai. Please delete and rerun if you'd like to replace it."
    assert open(out + ".bai", "rb").read() == b"kept" and os.path.getsize(out) == 0


# ---- 8. the SAM route ------------------------------------------------------------------------------------------------------------------
def test_sam_route(gpu_lib, tmp_path):
    bai, _, irep, _ = indexed_sam(gpu_lib, HEAD.encode(), tmp_path)
    assert bai == b"BAI\1" + struct.pack("<i", 3) + struct.pack("<ii", 0, 0) * 3 + struct.pack("<Q", 0)
    _, _, irep, _ = indexed_sam(gpu_lib, (HEAD + line(f0="only")).encode(), tmp_path)
    assert irep["records"] == 1 and irep["runs"] == 1
    _, _, irep, _ = indexed_sam(gpu_lib, (HEAD + "".join(MIX)).encode(), tmp_path)
    assert irep["records"] == 12 and irep["n_no_coor"] == 7
    n = 257
    lines = [line(f"XN:i:{k}", f0=f"q{k}", f2=NAMES[k * 3 // n], f3=str(1 + k * 7)) for k in range(n)]
    for tile in (0, 64):
        _, _, irep, _ = indexed_sam(gpu_lib, (HEAD + "".join(reversed(lines))).encode(), tmp_path, tile=tile)
        assert irep["records"] == n
    _, _, irep, _ = indexed_sam(gpu_lib, shuffled(random_sam(97, 1200, tmp_path), 3), tmp_path, piece_bytes=40000, tile=500)
    assert irep["records"] == 1200


def test_sam_route_records_at_block_and_piece_ends(gpu_lib, tmp_path):
    n = 544 * 2 + 5
    lines = [line(f0=("n%d" % k).ljust(73, "x"), f2=NAMES[k * 3 // n], f3=str(1 + k * 11)) for k in range(n)]
    one = tm.bam_records((HEAD + lines[0]).encode())[0]
    assert len(one) == 120 and BLOCK % 120 == 0
    sam = (HEAD + "".join(reversed(lines))).encode()
    for piece in (BLOCK, 2 * BLOCK, 65536):
        _, rep, irep, _ = indexed_sam(gpu_lib, sam, tmp_path, piece_bytes=piece)
        assert irep["records"] == n and rep["pieces"] == -(-n * 120 // piece)


# ---- 9. the chain, through the command line -----------------------------------------------------------------------------------------
def test_chain_convert_with_index_then_view(gpu_lib, ngs, tmp_path):
    def run(*args):
        return subprocess.run([ngs, *args], capture_output=True, timeout=600)
    names, lens, _ = grch38_no_alt()
    rng = np.random.default_rng(98)
    hb = random_batch(rng, 6000, lens, max_len=160)                               # (its records come in random order)
    aux = [bamio.aligner_aux(rng, int(hb.cols["l_seq"][i])) for i in range(hb.n)]
    qn = [bamio.aligner_name(rng) for _ in range(hb.n)]
    src, out = str(tmp_path / "in.bam"), str(tmp_path / "sorted.bam")
    bamio.write_bam(src, hb, names, lens, block_payload=7000, with_index=False, sort_order="unsorted", names=qn, aux=aux)
    r = run("convert", "-v", "--gzip", "device", "--sort", "coordinate", "--write-index", src, out)
    assert r.returncode == 0, r.stderr
    assert b"[ngs] convert: index of 6000 records (" in r.stderr
    assert gzip.decompress(open(out, "rb").read()) == bsm.bam_stream(open(src, "rb").read())
    bai = open(out + ".bai", "rb").read()
    held(out, bai, gpu_lib, tmp_path)
    query = "chr1:1000000-200000000"
    r = run("view", "-m", "records-only", out, query)                             # no `ngs index` in between
    assert r.returncode == 0, r.stderr
    assert r.stdout == vm.expected_view(out, query, "records-only", bai) and r.stdout.count(b"\n") > 10
    r = run("index", out)
    assert r.returncode == 1 and b"refusing to overwrite existing index file: " in r.stderr
    assert open(out + ".bai", "rb").read() == bai
    # -n: the index is of what was written
    short = str(tmp_path / "short.bam")
    r = run("convert", "--gzip", "device", "--sort", "coordinate", "--write-index", "-n", "500", src, short)
    assert r.returncode == 0, r.stderr
    assert gzip.decompress(open(short, "rb").read()) == bsm.bam_stream(open(src, "rb").read(), 500)
    assert held(short, open(short + ".bai", "rb").read(), gpu_lib, tmp_path)["records"] == 500


# ---- 10. a random sweep -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_mixes(gpu_lib, tmp_path, seed):
    rng = np.random.default_rng(9700 + seed)
    n = int(rng.integers(200, 3000))
    lens = [300_000, 70_000, 5_000]
    hb = random_batch(rng, n, lens, max_len=int(rng.integers(1, 400)))
    aux = [bamio.aligner_aux(rng, int(hb.cols["l_seq"][i])) if rng.random() < 0.7 else b"" for i in range(hb.n)]
    qn = [b"r" * int(rng.integers(1, 40)) + b"%d" % i for i in range(hb.n)]
    src = str(tmp_path / "r.bam")
    bamio.write_bam(src, hb, NAMES, lens, block_payload=int(rng.integers(500, 60000)), with_index=False, sort_order="unknown", names=qn, aux=aux,
                    level=int(rng.integers(0, 7)))
    bam = open(src, "rb").read()
    for _ in range(2):
        batch = int(rng.choice([0, 1, 63, 64, 65, int(rng.integers(2, n + 2))]))
        piece = int(rng.choice([0, 777, 4096, 65280, 65536, int(rng.integers(100, 200000))]))
        tile = int(rng.choice([0, 1, 63, 64, 65, 256, int(rng.integers(2, n + 2))]))
        _, _, irep, _ = indexed(gpu_lib, bam, tmp_path, tile=tile, batch_records=batch, piece_bytes=piece)
        assert irep["records"] == n
