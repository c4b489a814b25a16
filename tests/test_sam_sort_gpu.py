"""`ngs convert --gzip device --sort coordinate <SAM> <BAM>` on the GPU.  Every case holds the decompressed
output to the test-side model's stream (tests/sort_model.py) byte for byte, with the BGZF container checks of
tests/test_sam_to_bam_gpu.py.  The cases: the smallest files, reversed order at the edges of a wave and of a block, unplaced
records, two reference digits and the top position digit, every alignment of the gather's source and destination, a record
larger than a piece, floats, chunk and piece sizes, `-n`, the refusals, and the chain convert, index, convert back, view
through the command line."""
import gzip
import os
import random
import re
import struct
import subprocess

import pytest

from ngs_amd import build, host
from tests import bai_model as bm
from tests import bamio
from tests import bam_text_model as tm
from tests import sort_model as som
from tests import view_model as vm
from tests.test_sam_to_bam import GOOD, HEAD, NAMES, hand_spec_text, random_sam
from tests.test_sam_to_bam_gpu import blocks_of, line

pytestmark = pytest.mark.gpu

EOF = bamio.EOF_BLOCK
PER_RECORD = 48   # bytes the budget counts per record beside its own (include/ngsq_samtext.h)


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def convert(lib, sam: bytes, tmp_path, name="o", **kw):
    src, out = str(tmp_path / (name + ".sam")), str(tmp_path / (name + ".bam"))
    with open(src, "wb") as f:
        f.write(sam)
    rep = host.sam_to_sorted_bam(src, out, lib=lib, **kw)
    return open(out, "rb").read(), rep, out


def check(lib, sam: bytes, tmp_path, want=None, **kw):
    """Convert and hold the output to the model (want: its stream, when the caller has it already); the file's bytes, the
    report and the path."""
    raw, rep, out = convert(lib, sam, tmp_path, **kw)
    if want is None:
        want = som.bam_stream(sam, kw.get("max_records", 0))
    got = gzip.decompress(raw)
    if got != want:
        k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"stream differs at byte {k} of {len(got)} / {len(want)}: got {got[max(k - 8, 0):k + 24].hex()} want {want[max(k - 8, 0):k + 24].hex()}")
    bl = blocks_of(raw)
    assert raw.endswith(EOF) and all(b <= 65536 for b, _ in bl) and all(i > 0 for _, i in bl[:-1]) and bl[-1] == (28, 0)
    assert rep["bam_bytes"] == len(want) and rep["compressed_bytes"] == len(raw) and rep["blocks"] == len(bl) - 1
    assert rep["passes_run"] + rep["passes_skipped"] == 8
    return raw, rep, out


def shuffled(sam: bytes, seed: int) -> bytes:
    header, body = tm.split_header(sam)
    lines = tm.body_lines(body)
    random.Random(seed).shuffle(lines)
    return header + b"".join(x + b"\n" for x in lines)


# ---- 1. the smallest files, reversed order --------------------------------------------------------------------------------
def test_zero_one_and_two_records(gpu_lib, tmp_path):
    raw, rep, _ = check(gpu_lib, b"", tmp_path)
    assert gzip.decompress(raw) == b"BAM\1" + struct.pack("<i", len(som.NEW_HD)) + som.NEW_HD + struct.pack("<i", 0)
    assert rep["records"] == 0 and rep["pieces"] == 0 and len(blocks_of(raw)) == 2
    raw, rep, _ = check(gpu_lib, HEAD.encode(), tmp_path)
    assert rep["records"] == 0 and b"@HD\tVN:1.6\tSO:coordinate\n@SQ" in gzip.decompress(raw)
    _, rep, _ = check(gpu_lib, (HEAD + line(f0="only")).encode(), tmp_path)
    assert rep["records"] == 1 and rep["pieces"] == 1 and rep["passes_run"] == 0
    for a, b in (("9", "5"), ("5", "9"), ("5", "5")):
        _, rep, _ = check(gpu_lib, (HEAD + line(f0="first", f3=a) + line(f0="second", f3=b)).encode(), tmp_path)
        assert rep["records"] == 2


@pytest.mark.parametrize("n", [65, 257])
def test_reversed_order(gpu_lib, tmp_path, n):
    body = "".join(line(f"XN:i:{k}", f0=f"q{k}", f2=NAMES[k * 3 // n], f3=str(1 + k * 7)) for k in range(n))
    lines = body.splitlines(keepends=True)
    sam = (HEAD + "".join(reversed(lines))).encode()
    raw, rep, out = check(gpu_lib, sam, tmp_path)
    assert rep["records"] == n
    assert gzip.decompress(raw).endswith(b"".join(tm.bam_records((HEAD + body).encode())))     # (the text was written in order)
    assert host.build_bam_index(out, lib=gpu_lib)["records"] == n


# ---- 2. unplaced records, wide keys ---------------------------------------------------------------------------------------
def test_unplaced_records_go_last_in_input_order(gpu_lib, tmp_path):
    un = lambda k: line(f0=f"u{k}", f1="77", f2="*", f3="0", f4="0", f5="*", f6="*", f7="0", f9="NNNN", f10="&&&&")
    body = [un(0), un(1), line(f0="a", f2="chr2", f3="40"), line(f0="b", f3="30"), un(2), line(f0="zero", f3="0"),      # chr1 POS 0
            line(f0="c", f3="1"), line(f0="d", f2="chr3", f3="5000"), un(3), line(f0="zero2", f2="chr2", f3="0"), line(f0="e", f3="30"), un(4)]
    raw, rep, out = check(gpu_lib, (HEAD + "".join(body)).encode(), tmp_path)
    names = [x.split(b"\t")[0].decode() for x in som.sorted_lines((HEAD + "".join(body)).encode())]
    assert names == ["c", "b", "e", "a", "d", "u0", "u1", "u2", "zero", "u3", "zero2", "u4"]
    irep = host.build_bam_index(out, lib=gpu_lib)
    assert irep["records"] == 12 and irep["n_no_coor"] == 7


def test_two_reference_digits_and_the_top_position_digit(gpu_lib, tmp_path):
    rng = random.Random(81)
    top = 2 ** 31 - 1
    head = "@HD\tVN:1.6\tSO:unsorted\n" + "".join(f"@SQ\tSN:contig{k}\tLN:{top}\n" for k in range(300))
    pos = [1, 2, 255, 256, 257, 65535, 65536, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 2, top] + [rng.randrange(1, top + 1) for _ in range(60)]
    body = [line(f0=f"c{r}p{p}", f2=f"contig{r}", f3=str(p), f5="*", f6="*", f7="0") for r in (0, 1, 255, 256, 257, 299) for p in pos]
    rng.shuffle(body)
    _, rep, _ = check(gpu_lib, (head + "".join(body)).encode(), tmp_path)
    assert rep["passes_run"] == 6                                               # four position digits, two reference digits


# ---- 3. the gather's alignments, a record larger than a piece, floats ------------------------------------------------------
def test_every_residue_of_source_and_destination_offsets(gpu_lib, tmp_path):
    rng = random.Random(82)
    body = []
    for k in range(400):
        tags = [[], ["XA:A:k"], ["XZ:Z:" + "z" * (k % 5)], ["XI:i:7", "XS:i:300"]][k % 4]
        body.append(line(*tags, f0="n" * (1 + k % 8), f3=str(rng.randrange(1, 60000))))
    sam = (HEAD + "".join(body)).encode()
    recs = tm.bam_records(sam)
    residues = lambda rs: {sum(len(r) for r in rs[:k]) % 8 for k in range(len(rs))}
    assert residues(recs) == set(range(8)) and residues(som.sorted_records(sam)) == set(range(8))
    for piece in (0, 4096, 1000):
        _, rep, _ = check(gpu_lib, sam, tmp_path, piece_bytes=piece)
        assert rep["pieces"] == (1 if piece == 0 else -(-sum(len(r) for r in recs) // piece))


def test_a_long_cigar_record_moves_whole(gpu_lib, tmp_path):
    ops = "".join("%d%s" % (1 + k % 3, "MID"[k % 3]) for k in range(70_000))
    l_seq = sum(1 + k % 3 for k in range(70_000) if k % 3 < 2)
    spec = hand_spec_text()
    header, body = tm.split_header(spec)
    lines = [x + b"\n" for x in tm.body_lines(body)]
    lines.append(line("NM:i:0", f0="long", f3="200", f5=ops, f9="A" * l_seq, f10="*").encode())
    lines += [line(f0=f"s{k}", f3=str(50 + 40 * k)).encode() for k in range(20)]
    random.Random(83).shuffle(lines)
    sam = header + b"".join(lines)
    raw, _, _ = check(gpu_lib, sam, tmp_path, piece_bytes=4096)                 # the record spans some 70 pieces
    assert b"NMC\0CGBI" + struct.pack("<I", 70_000) in gzip.decompress(raw)
    check(gpu_lib, sam, tmp_path)


def test_lines_with_floats(gpu_lib, tmp_path):
    body = [line(f"XF:f:{k}.5", "XB:B:f,1.5,-2.25,1e-3", f0=f"f{k}", f3=str(1000 - 3 * k)) if k % 3 == 0 else line(f0=f"p{k}", f3=str(1000 - 3 * k))
            for k in range(200)]
    check(gpu_lib, (HEAD + "".join(body)).encode(), tmp_path, chunk_bytes=3000)


# ---- 4. one stream whatever the chunks and pieces; -n ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text2000(tmp_path_factory):
    big = line(f0="big", f3="150000", f5="*", f9="ACGT" * 2500, f10="*").encode()               # a 10 KB record: larger than a piece of 4096
    sam = shuffled(random_sam(84, 2000, tmp_path_factory.mktemp("src")) + big, 85)
    return sam, som.bam_stream(sam)


def test_chunks_and_pieces_do_not_change_the_stream(gpu_lib, tmp_path, text2000):
    sam, want = text2000
    _, one, _ = check(gpu_lib, sam, tmp_path, want=want)
    assert one["chunks"] == 1 and one["pieces"] == 1 and one["records"] == 2001
    _, many, _ = check(gpu_lib, sam, tmp_path, want=want, chunk_bytes=len(sam) // 6)
    assert many["chunks"] >= 5
    _, cut, _ = check(gpu_lib, sam, tmp_path, want=want, piece_bytes=4096, chunk_bytes=len(sam) // 6)
    records = len(want) - len(tm.header_stream(som.sorted_header(tm.split_header(sam)[0]), tm.references(tm.split_header(sam)[0])))
    assert cut["pieces"] == -(-records // 4096) and cut["resident_bytes"] == records + 2001 * PER_RECORD
    again, _, _ = convert(gpu_lib, sam, tmp_path, name="again", piece_bytes=4096, chunk_bytes=len(sam) // 6)
    assert again == open(tmp_path / "o.bam", "rb").read()


def test_max_records_sorts_the_first_records_of_the_text(gpu_lib, ngs, tmp_path, text2000):
    sam, _ = text2000
    for n in (1, 64, 2000):                                                       # (2001 records: n - 1 is 2000)
        _, rep, _ = check(gpu_lib, sam, tmp_path, max_records=n, chunk_bytes=len(sam) // 6)
        assert rep["records"] == n
    src = str(tmp_path / "o.sam")
    for n, want in (("0", 1), ("3", 3)):                                          # the command line: max(N, 1)
        r = subprocess.run([ngs, "convert", "--gzip", "device", "--sort", "coordinate", "-n", n, src, str(tmp_path / "n.bam")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert gzip.decompress(open(tmp_path / "n.bam", "rb").read()) == som.bam_stream(sam, want)


def test_chunk_edges_and_max_records_of_the_shared_parser(gpu_lib, tmp_path):
    """The cases of test_chunk_edges and test_num_records_and_empty_files of tests/test_sam_to_bam_gpu.py through the sorted
    path, which runs the same chunk parser: chunk ends on every byte of the lines, a line one byte longer than a chunk, a last
    line without its newline, a fault in a later chunk, `max_records` on and beside the chunk ends."""
    sam = shuffled(random_sam(43, 300, tmp_path), 88)
    header, body = tm.split_header(sam)
    lines = tm.body_lines(body)
    longest = max(len(x) for x in lines)
    want = som.bam_stream(sam)
    for chunk in (longest, longest + 1, 1000):
        _, rep, _ = check(gpu_lib, sam, tmp_path, want=want, chunk_bytes=chunk)
        assert rep["chunks"] > 10 and rep["records"] == 300
    with pytest.raises(host.NgsqError) as e:
        convert(gpu_lib, sam, tmp_path, chunk_bytes=longest - 1)
    k = next(i for i, x in enumerate(lines) if len(x) == longest)
    assert e.value.message == f"reading SAM record: record {k}: line longer than {longest - 1} bytes"
    assert os.path.getsize(tmp_path / "o.bam") == 0
    check(gpu_lib, sam[:-1], tmp_path, chunk_bytes=1000)                          # a last line without its newline
    # a faulty line in a chunk other than the first
    good = ["\t".join(GOOD[:3] + [str(900 - k)] + GOOD[4:]) + "\n" for k in range(500)]
    good[300] = line(f4="x")
    with pytest.raises(host.NgsqError) as e:
        convert(gpu_lib, (HEAD + "".join(good)).encode(), tmp_path, chunk_bytes=2000)
    assert e.value.message == f"reading SAM record: record 300: {tm.ERROR_TEXT[tm.E_MAPQ]}"
    assert os.path.getsize(tmp_path / "o.bam") == 0
    # max_records; the records behind which the host cuts its chunks: up to chunk + 1 bytes from the last cut, cut at their last newline
    chunk, ends, at = 2000, [], 0
    while at < len(body):
        at += body[at:at + chunk + 1].rfind(b"\n") + 1
        ends.append(body[:at].count(b"\n"))
    assert len(ends) > 10 and ends[-1] == 300 and ends[0] > 1
    for n, chunks in ((1, 1), (ends[0] - 1, 1), (ends[0], 1), (ends[0] + 1, 2), (ends[4], 5), (ends[4] + 1, 6), (300, len(ends)), (10 ** 6, len(ends))):
        _, rep, _ = check(gpu_lib, sam, tmp_path, max_records=n, chunk_bytes=chunk)
        assert rep["records"] == min(n, 300) and rep["text_bytes"] == sum(len(x) + 1 for x in lines[:n])
        assert rep["chunks"] == chunks, (n, rep["chunks"], chunks)               # (nothing is read or launched behind the last record)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def test_a_faulty_line_keeps_its_message_and_index(gpu_lib, tmp_path):
    good = ["\t".join(GOOD[:3] + [str(900 - k)] + GOOD[4:]) + "\n" for k in range(500)]
    good[3] = line(f4="x")
    for chunk in (0, 2000):
        with pytest.raises(host.NgsqError) as e:
            convert(gpu_lib, (HEAD + "".join(good)).encode(), tmp_path, chunk_bytes=chunk)
        assert e.value.message == f"reading SAM record: record 3: {tm.ERROR_TEXT[tm.E_MAPQ]}"
        assert os.path.getsize(tmp_path / "o.bam") == 0                           # found before the first block is written


def test_records_beyond_the_budget_are_refused(gpu_lib, tmp_path):
    sam = (HEAD + "".join(line(f0=f"q{k}", f3=str(60000 - k), f5="*", f9="ACGT" * 100, f10="*") for k in range(4000))).encode()
    recs = tm.bam_records(sam)
    total = sum(len(r) for r in recs)
    assert total > 1 << 20
    with pytest.raises(host.NgsqError) as e:
        convert(gpu_lib, sam, tmp_path, max_resident_bytes=1 << 20)
    assert e.value.code == host.ffi.ERR_LIMIT
    assert e.value.message == (f"reading SAM record: --sort coordinate holds the records in device memory: {total + len(recs) * PER_RECORD} bytes needed, "
                               f"{1 << 20} allowed")
    with pytest.raises(host.NgsqError) as e:                                      # in chunks: as soon as the running total shows it
        convert(gpu_lib, sam, tmp_path, max_resident_bytes=1 << 20, chunk_bytes=100_000)
    m = re.fullmatch(r"reading SAM record: --sort coordinate holds the records in device memory: (\d+) bytes needed, 1048576 allowed", e.value.message)
    assert m and 1 << 20 < int(m.group(1)) < (1 << 20) + 2 * 100_000
    assert os.path.getsize(tmp_path / "o.bam") == 0
    check(gpu_lib, sam, tmp_path, max_resident_bytes=total + len(recs) * PER_RECORD)       # exactly the budget: converted


def test_a_failed_write_ends_the_call_with_its_message(gpu_lib, tmp_path):
    """/dev/full refuses every write: with one piece the error is read at the end of the run, with many the piece loop meets a
    writer that has failed.  faulthandler ends the process if the call hangs (the suite has no in-process time limit)."""
    import faulthandler
    sam = HEAD.encode() + b"".join(line(f0=f"q{k}", f3=str(500 - k)).encode() for k in range(300))
    src = str(tmp_path / "w.sam")
    open(src, "wb").write(sam)
    faulthandler.dump_traceback_later(120, exit=True)
    try:
        for piece in (0, 2000):
            with pytest.raises(host.NgsqError) as e:
                host.sam_to_sorted_bam(src, "/dev/full", piece_bytes=piece, lib=gpu_lib)
            assert "writing BAM record: No space left on device (os error 28)" in str(e.value), piece
    finally:
        faulthandler.cancel_dump_traceback_later()


# ---- 6. the chain, through the command line -----------------------------------------------------------------------------------
def test_chain_convert_index_convert_back_view(gpu_lib, ngs, tmp_path):
    def run(*args):
        return subprocess.run([ngs, *args], capture_output=True, timeout=600)
    header, body = tm.split_header(shuffled(random_sam(86, 6000, tmp_path), 87))
    sam = header.replace(b"\tSO:coordinate", b"") + body                         # the text does not claim an order
    src, out, plain = str(tmp_path / "in.sam"), str(tmp_path / "sorted.bam"), str(tmp_path / "plain.bam")
    open(src, "wb").write(sam)
    r = run("convert", "--gzip", "device", "--sort", "coordinate", src, out)
    assert r.returncode == 0, r.stderr
    assert gzip.decompress(open(out, "rb").read()) == som.bam_stream(sam)
    r = run("index", out)
    assert r.returncode == 0, r.stderr
    bai = open(out + ".bai", "rb").read()
    assert bai == bm.expected_bai(out)
    lines = som.sorted_lines(sam)
    r = run("convert", out, str(tmp_path / "back.sam"))
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "back.sam", "rb").read() == som.sorted_header(tm.split_header(sam)[0]) + b"".join(x + b"\n" for x in lines)
    query = "chr1:100000-160000"
    r = run("view", "-m", "records-only", out, query)
    assert r.returncode == 0, r.stderr
    ref_id, s, e = vm.parse_query(query, NAMES)
    keep = vm.selected(out, ref_id, s, e, vm.query_chunks(bai, ref_id, s, e))
    assert len(keep) > 100 and r.stdout == b"".join(lines[i] + b"\n" for i in keep)
    # the same records in the order of the text, under a header that claims coordinate order: `ngs index` finds them unsorted
    lie = str(tmp_path / "lie.sam")
    open(lie, "wb").write(som.sorted_header(tm.split_header(sam)[0]) + body)
    r = run("convert", "--gzip", "device", lie, plain)
    assert r.returncode == 0, r.stderr
    r = run("index", plain)
    assert r.returncode == 1 and b"out of coordinate order" in r.stderr and not os.path.exists(plain + ".bai")
