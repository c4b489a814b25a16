"""`ngs convert --gzip device --sort coordinate <BAM> <BAM>` on the GPU.  Every case holds the decompressed
output to the test-side model's stream (tests/bam_sort_model.py) byte for byte, with the BGZF container checks of
tests/test_sam_sort_gpu.py.  The cases: the smallest files, reversed order at the edges of a wave, a block and a sort tile,
unplaced records, every alignment of a batch's source range and of the gather, ingest chunks that cut records and more than one
slab, wide keys, idempotence, `-n` and `-v`, the refusals, the chain convert, index, view, convert back through the command
line, and a random sweep."""
import ctypes as C
import gzip
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from ngs_amd import build, ffi, host
from ngs_amd.genome_shape import grch38_no_alt
from tests import bam_sort_model as bsm
from tests import bam_text_model as tm
from tests import bamio
from tests import sam_model as sm
from tests import view_model as vm
from tests.test_convert_gpu import write_long_reads
from tests.test_sam_to_bam import HEAD, NAMES, random_sam
from tests.test_sam_to_bam_gpu import blocks_of, line
from tests.util import random_batch

pytestmark = pytest.mark.gpu

EOF = bamio.EOF_BLOCK
PER_RECORD = 48   # bytes the budget counts per record beside its own (include/ngsq_bamsort.h)
CTX = "reading BAM record: "


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def bam_of(sam: bytes, payload: int = 65280) -> bytes:
    """A BAM file of the SAM text, its records in the order of the text (tests/bam_text_model.py, zlib's blocks)."""
    return tm.bam_file(tm.bam_stream(sam), payload)


def convert(lib, bam: bytes, tmp_path, name="o", **kw):
    src, out = str(tmp_path / (name + ".in.bam")), str(tmp_path / (name + ".bam"))
    with open(src, "wb") as f:
        f.write(bam)
    rep = host.bam_to_sorted_bam(src, out, lib=lib, **kw)
    return open(out, "rb").read(), rep, out


def check(lib, bam: bytes, tmp_path, want=None, **kw):
    """Convert and hold the output to the model (want: its stream, when the caller has it already); the file's bytes, the
    report and the path."""
    raw, rep, out = convert(lib, bam, tmp_path, **kw)
    if want is None:
        want = bsm.bam_stream(bam, kw.get("max_records", 0))
    got = gzip.decompress(raw)
    if got != want:
        k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"stream differs at byte {k} of {len(got)} / {len(want)}: got {got[max(k - 8, 0):k + 24].hex()} want {want[max(k - 8, 0):k + 24].hex()}")
    bl = blocks_of(raw)
    assert raw.endswith(EOF) and all(b <= 65536 for b, _ in bl) and all(i > 0 for _, i in bl[:-1]) and bl[-1] == (28, 0)
    assert rep["bam_bytes"] == len(want) and rep["compressed_bytes"] == len(raw) and rep["blocks"] == len(bl) - 1
    assert rep["passes_run"] + rep["passes_skipped"] == 8
    return raw, rep, out


def names_of(raw: bytes):
    return [r[36:r.index(b"\0", 36)].decode() for r in bsm.split(gzip.decompress(raw))[2]]


# ---- 1. the smallest files ------------------------------------------------------------------------------------------------------
def test_zero_one_and_two_records(gpu_lib, tmp_path):
    raw, rep, _ = check(gpu_lib, bam_of(HEAD.encode()), tmp_path)
    assert rep["records"] == 0 and rep["pieces"] == 0 and rep["slabs"] == 0 and len(blocks_of(raw)) == 2          # header, EOF
    assert b"@HD\tVN:1.6\tSO:coordinate\n@SQ" in gzip.decompress(raw)
    _, rep, _ = check(gpu_lib, bam_of((HEAD + line(f0="only")).encode()), tmp_path)
    assert rep["records"] == 1 and rep["pieces"] == 1 and rep["passes_run"] == 0 and rep["batches"] == 1 and rep["slabs"] == 1
    for a, b, first in (("9", "5", "second"), ("5", "9", "first"), ("5", "5", "first")):
        raw, rep, _ = check(gpu_lib, bam_of((HEAD + line(f0="first", f3=a) + line(f0="second", f3=b)).encode()), tmp_path)
        assert rep["records"] == 2 and names_of(raw)[0] == first


# ---- 2. reversed order: one past a wave, a block, a tile of the sort --------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 257, 4097])
def test_reversed_order(gpu_lib, tmp_path, n):
    assert n != 4097 or n == gpu_lib.ngsq_sort_tile_keys() + 1
    lines = [line(f"XN:i:{k}", f0=f"q{k}", f2=NAMES[k * 3 // n], f3=str(1 + k * 7)) for k in range(n)]
    raw, rep, out = check(gpu_lib, bam_of((HEAD + "".join(reversed(lines))).encode()), tmp_path)
    assert rep["records"] == n
    assert gzip.decompress(raw).endswith(b"".join(tm.bam_records((HEAD + "".join(lines)).encode())))
    assert host.build_bam_index(out, lib=gpu_lib)["records"] == n


# ---- 3. unplaced records ------------------------------------------------------------------------------------------------------
def test_unplaced_records_go_last_in_input_order(gpu_lib, tmp_path):
    un = lambda k: line(f0=f"u{k}", f1="77", f2="*", f3="0", f4="0", f5="*", f6="*", f7="0", f9="NNNN", f10="&&&&")
    body = [un(0), un(1), line(f0="a", f2="chr2", f3="40"), line(f0="b", f3="30"), un(2), line(f0="zero", f3="0"),      # chr1 POS 0: refID 0, pos -1
            line(f0="c", f3="1"), line(f0="d", f2="chr3", f3="5000"), un(3), line(f0="zero2", f2="chr2", f3="0"), line(f0="e", f3="30"), un(4)]
    bam = bam_of((HEAD + "".join(body)).encode())
    recs = bsm.split(gzip.decompress(bam))[2]
    assert {struct.unpack_from("<ii", r, 4) for r in recs} >= {(-1, -1), (0, -1), (1, -1), (0, 0)}
    raw, rep, out = check(gpu_lib, bam, tmp_path)
    assert names_of(raw) == ["c", "b", "e", "a", "d", "u0", "u1", "u2", "zero", "u3", "zero2", "u4"]
    irep = host.build_bam_index(out, lib=gpu_lib)
    assert irep["records"] == 12 and irep["n_no_coor"] == 7
    assert rep["passes_run"] >= 4                                                 # the unplaced records' hi brings the upper digits in


# ---- 4. alignment ---------------------------------------------------------------------------------------------------------------
def alignment_file():
    rng = random.Random(92)
    body = []
    for k in range(400):
        tags = [[], ["XA:A:k"], ["XZ:Z:" + "z" * (k % 5)], ["XI:i:7", "XS:i:300"], ["XB:B:c,1,2,3"]][k % 5]
        body.append(line(*tags, f0="n" * (1 + (k * 3) % 8), f3=str(rng.randrange(1, 60000))))
    return bam_of((HEAD + "".join(body)).encode())


def batch_start_residues(bam: bytes, batch: int):
    """The offsets modulo 16, in the decompressed input, of the first record of every batch of `batch` records: the residue of a
    batch's source range in the ingest's view, whose first chunk begins on a 16-byte boundary."""
    text, table, recs = bsm.split(gzip.decompress(bam))
    at, out = 8 + len(text) + len(table), set()
    for k, r in enumerate(recs):
        if k % batch == 0:
            out.add(at % 16)
        at += len(r)
    return out


def test_every_residue_of_a_batch_and_of_the_gather(gpu_lib, tmp_path):
    bam = alignment_file()
    recs = bsm.split(gzip.decompress(bam))[2]
    total = sum(len(r) for r in recs)
    assert len(recs) == 400 and batch_start_residues(bam, 1) == set(range(16)) and len(batch_start_residues(bam, 7)) >= 12
    residues8 = lambda rs: {sum(len(r) for r in rs[:k]) % 8 for k in range(len(rs))}
    assert residues8(bsm.sorted_records(recs)) == set(range(8))
    want = bsm.bam_stream(bam)
    for batch in (1, 7, 64, 65, 0):
        _, rep, _ = check(gpu_lib, bam, tmp_path, want=want, batch_records=batch)
        assert rep["batches"] == (1 if batch == 0 else -(-400 // batch)) and rep["records"] == 400
        assert rep["resident_bytes"] == total + 400 * PER_RECORD                  # (the padding is the slab's, not the budget's)
    for piece, batch in ((0, 7), (4096, 1), (1000, 7), (1000, 65)):
        _, rep, _ = check(gpu_lib, bam, tmp_path, want=want, piece_bytes=piece, batch_records=batch)
        assert rep["pieces"] == (1 if piece == 0 else -(-total // piece))


# ---- 5. ingest chunks that cut records, more than one slab, a record larger than a piece -----------------------------------------
def test_chunks_and_slabs(gpu_lib, tmp_path, monkeypatch):
    """1 MiB ingest buffers (as tests/test_convert_gpu.py's test of several chunks): every chunk's end cuts a 100 kb read, the
    next batch begins in the bytes carried in front of its chunk, and the slabs, sized from the ingest's buffers, are several."""
    src = str(tmp_path / "l.bam")
    write_long_reads(src)
    text, table, recs = bsm.split(gzip.decompress(open(src, "rb").read()))
    stream = gzip.decompress(open(src, "rb").read())
    bam = tm.bam_file(stream[:len(stream) - sum(len(r) for r in recs)] + b"".join(reversed(recs)), 60000)        # the file is in order: turn it round
    assert max(len(r) for r in recs) > 65536 and sum(len(r) for r in recs) > 3 << 20
    monkeypatch.setenv("NGSQ_INGEST_RAW_MB", "1")
    want = bsm.bam_stream(bam)
    _, rep, out = check(gpu_lib, bam, tmp_path, want=want, piece_bytes=65536)
    assert rep["slabs"] >= 2 and rep["batches"] >= 3 and rep["records"] == len(recs)
    assert rep["pieces"] == -(-sum(len(r) for r in recs) // 65536)
    _, one, _ = check(gpu_lib, bam, tmp_path, want=want, batch_records=1)
    assert one["batches"] == len(recs) and one["slabs"] >= 2
    monkeypatch.delenv("NGSQ_INGEST_RAW_MB")
    _, rep, _ = check(gpu_lib, bam, tmp_path, want=want)
    assert rep["slabs"] == 1 and rep["batches"] == 1
    assert host.build_bam_index(out, lib=gpu_lib)["records"] == len(recs)


# ---- 6. wide keys -----------------------------------------------------------------------------------------------------------------
def test_two_reference_digits_and_the_top_position_digit(gpu_lib, tmp_path):
    rng = random.Random(81)
    top = 2 ** 31 - 1                                                             # POS: pos is one less, the largest a record holds
    head = "@HD\tVN:1.6\tSO:unsorted\n" + "".join(f"@SQ\tSN:contig{k}\tLN:{top}\n" for k in range(300))
    pos = [1, 2, 255, 256, 257, 65535, 65536, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 2, top] + [rng.randrange(1, top + 1) for _ in range(60)]
    body = [line(f0=f"c{r}p{p}", f2=f"contig{r}", f3=str(p), f5="*", f6="*", f7="0") for r in (0, 1, 255, 256, 257, 299) for p in pos]
    rng.shuffle(body)
    _, rep, _ = check(gpu_lib, bam_of((head + "".join(body)).encode()), tmp_path)
    assert rep["passes_run"] == 6                                                 # four position digits, two reference digits


# ---- 7. idempotence ---------------------------------------------------------------------------------------------------------------
def test_sorting_the_output_again_changes_nothing(gpu_lib, tmp_path):
    bam = bam_of(random_sam(93, 1500, tmp_path), 7000)
    raw, _, _ = check(gpu_lib, bam, tmp_path)
    again, rep, _ = check(gpu_lib, raw, tmp_path, name="again")
    assert gzip.decompress(again) == gzip.decompress(raw)
    assert bsm.split(gzip.decompress(again))[2] == bsm.split(gzip.decompress(raw))[2]      # sorted input: its own records, in order
    assert rep["records"] == 1500


# ---- 8. -n and -v through the command line -----------------------------------------------------------------------------------------
def test_num_records_and_the_report_line(gpu_lib, ngs, tmp_path):
    bam = bam_of(random_sam(94, 300, tmp_path), 7000)
    src, out = str(tmp_path / "in.bam"), str(tmp_path / "n.bam")
    open(src, "wb").write(bam)
    for n, want in (("0", 1), ("1", 1), ("5", 5)):                                # the command line: max(N, 1)
        r = subprocess.run([ngs, "convert", "--gzip", "device", "--sort", "coordinate", "-n", n, src, out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert gzip.decompress(open(out, "rb").read()) == bsm.bam_stream(bam, want)
        assert "[ngs] convert" not in r.stderr
    r = subprocess.run([ngs, "convert", "-v", "--gzip", "device", "--sort", "coordinate", src, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "[ngs] convert: 300 records in 1 batches and 1 slabs sorted in " in r.stderr and " of 8 passes, " in r.stderr
    assert gzip.decompress(open(out, "rb").read()) == bsm.bam_stream(bam)
    for n in (1, 64, 299):                                                        # the library: the first n records, sorted
        _, rep, _ = check(gpu_lib, bam, tmp_path, max_records=n, batch_records=50)
        assert rep["records"] == n


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------
def ingest_message(lib, path, tmp_path):
    """What the device ingest says about the file: the message of BAM to SAM, which passes it on as it is."""
    with pytest.raises(host.NgsqError) as e:
        host.bam_to_sam(path, str(tmp_path / "refused.sam"), lib=lib)
    return e.value.message


@pytest.fixture(scope="module")
def stream4000():
    """The decompressed stream of 4000 records of some 450 bytes in descending order: more than 1 MiB."""
    return tm.bam_stream((HEAD + "".join(line(f0=f"q{k}", f3=str(60000 - k), f5="*", f9="ACGT" * 100, f10="*") for k in range(4000))).encode())


def test_records_beyond_the_budget_are_refused(gpu_lib, tmp_path, stream4000):
    bam = tm.bam_file(stream4000)
    recs = bsm.split(stream4000)[2]
    total = sum(len(r) for r in recs)
    assert total > 1 << 20
    with pytest.raises(host.NgsqError) as e:
        convert(gpu_lib, bam, tmp_path, max_resident_bytes=1 << 20)
    assert e.value.code == ffi.ERR_LIMIT
    assert e.value.message == (f"{CTX}--sort coordinate holds the records in device memory: {total + len(recs) * PER_RECORD} bytes needed, "
                               f"{1 << 20} allowed")
    assert os.path.getsize(tmp_path / "o.bam") == 0
    with pytest.raises(host.NgsqError) as e:                                      # in batches: as soon as the running total shows it
        convert(gpu_lib, bam, tmp_path, max_resident_bytes=1 << 20, batch_records=500)
    need = next(sum(len(r) for r in recs[:k]) + k * PER_RECORD for k in range(500, 4001, 500) if sum(len(r) for r in recs[:k]) + k * PER_RECORD > 1 << 20)
    assert e.value.message == f"{CTX}--sort coordinate holds the records in device memory: {need} bytes needed, {1 << 20} allowed"
    assert os.path.getsize(tmp_path / "o.bam") == 0
    check(gpu_lib, bam, tmp_path, max_resident_bytes=total + len(recs) * PER_RECORD)       # exactly the budget: converted


def test_files_the_ingest_refuses_leave_the_output_empty(gpu_lib, tmp_path, stream4000):
    """Malformed files, refused by the ingest's own checks (the block framing on the host, the CRC of a stored block).  Both faults
    lie behind the first MiB of the file, which the reader inflates on the host when it opens it."""
    good = b"".join(bamio.bgzf_block(stream4000[k:k + 3000], level=0) for k in range(0, len(stream4000), 3000)) + EOF      # stored blocks
    at = len(good) * 3 // 4
    assert at > (1 << 20) + 65536
    cut = good[:at + 7]                                                           # ends in the middle of a block
    flipped = bytearray(good)
    p = 0
    while p + struct.unpack_from("<H", good, p + 16)[0] + 1 <= at:                # the block that holds byte `at`
        p += struct.unpack_from("<H", good, p + 16)[0] + 1
    assert (at + 7 - p) % 3031 not in (0, 3030) and good[p + 18:p + 23] == b"\x01\xb8\x0b\x47\xf4"    # a last stored block of 3000 bytes
    flipped[p + 18 + 5 + 100] ^= 0x20                                             # a payload byte of it: only its CRC notices
    for name, data in (("cut", cut), ("flipped", bytes(flipped))):
        src = str(tmp_path / (name + ".in.bam"))
        open(src, "wb").write(data)
        said = ingest_message(gpu_lib, src, tmp_path)
        assert ("truncated" in said) if name == "cut" else ("CRC" in said or "crc" in said), said
        with pytest.raises(host.NgsqError) as e:
            host.bam_to_sorted_bam(src, str(tmp_path / (name + ".bam")), lib=gpu_lib)
        assert e.value.message == CTX + said
        assert os.path.getsize(tmp_path / (name + ".bam")) == 0
    check(gpu_lib, good, tmp_path)                                                # the file itself converts


def test_a_reader_that_has_handed_out_records_is_refused(gpu_lib, tmp_path):
    src = str(tmp_path / "in.bam")
    open(src, "wb").write(bam_of((HEAD + line() + line(f3="3")).encode()))
    with host._reader_and_plain_context(gpu_lib, src, 0) as (bam, ctx):
        b = ffi.Batch()
        assert gpu_lib.ngsq_bam_next_batch_device(bam, ctx, 1, C.byref(b)) == ffi.OK and b.n_records == 1
        fd = os.open(str(tmp_path / "o.bam"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
        try:
            rep = ffi.BamSortReport()
            assert gpu_lib.ngsq_bam_write_sorted_bam(bam, ctx, fd, 0, 0, 0, 0, C.byref(rep)) == ffi.ERR_STATE
        finally:
            os.close(fd)
        assert "a sorted BAM file is written from a reader no record has been read from" in gpu_lib.ngsq_bam_last_error().decode()
    assert os.path.getsize(tmp_path / "o.bam") == 0


# ---- 10. the chain, through the command line ------------------------------------------------------------------------------------------
def test_chain_convert_index_view_convert_back(gpu_lib, ngs, tmp_path):
    def run(*args):
        return subprocess.run([ngs, *args], capture_output=True, timeout=600)
    names, lens, _ = grch38_no_alt()
    rng = np.random.default_rng(95)
    hb = random_batch(rng, 6000, lens, max_len=160)                               # (its records come in random order)
    aux = [bamio.aligner_aux(rng, int(hb.cols["l_seq"][i])) for i in range(hb.n)]
    qn = [bamio.aligner_name(rng) for _ in range(hb.n)]
    src, out, model = str(tmp_path / "in.bam"), str(tmp_path / "sorted.bam"), str(tmp_path / "model.bam")
    bamio.write_bam(src, hb, names, lens, block_payload=7000, with_index=False, sort_order="unsorted", names=qn, aux=aux)
    want = bsm.bam_stream(open(src, "rb").read())
    open(model, "wb").write(tm.bam_file(want))
    r = run("convert", "--gzip", "device", "--sort", "coordinate", src, out)
    assert r.returncode == 0, r.stderr
    assert gzip.decompress(open(out, "rb").read()) == want
    r = run("index", out)
    assert r.returncode == 0, r.stderr
    bai = open(out + ".bai", "rb").read()
    query = "chr1:1000000-200000000"
    r = run("view", "-m", "records-only", out, query)
    assert r.returncode == 0, r.stderr
    assert r.stdout == vm.expected_view(out, query, "records-only", bai) and r.stdout.count(b"\n") > 10
    r = run("convert", out, str(tmp_path / "back.sam"))
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "back.sam", "rb").read() == sm.expected_sam(model)


# ---- 11. a random sweep -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_mixes(gpu_lib, tmp_path, seed):
    rng = np.random.default_rng(9600 + seed)
    n = int(rng.integers(200, 3000))
    lens = [300_000, 70_000, 5_000]
    hb = random_batch(rng, n, lens, max_len=int(rng.integers(1, 400)))
    aux = [bamio.aligner_aux(rng, int(hb.cols["l_seq"][i])) if rng.random() < 0.7 else b"" for i in range(hb.n)]
    qn = [b"r" * int(rng.integers(1, 40)) + b"%d" % i for i in range(hb.n)]
    src = str(tmp_path / "r.bam")
    bamio.write_bam(src, hb, NAMES, lens, block_payload=int(rng.integers(500, 60000)), with_index=False, sort_order="unknown", names=qn, aux=aux,
                    level=int(rng.integers(0, 7)))
    bam = open(src, "rb").read()
    want = bsm.bam_stream(bam)
    for _ in range(3):
        batch, piece = int(rng.choice([0, 1, 63, 64, 65, int(rng.integers(2, n + 2))])), int(rng.choice([0, 777, 4096, 65536, int(rng.integers(100, 200000))]))
        _, rep, out = check(gpu_lib, bam, tmp_path, want=want, batch_records=batch, piece_bytes=piece)
        assert rep["records"] == n
    assert host.build_bam_index(out, lib=gpu_lib)["records"] == n
