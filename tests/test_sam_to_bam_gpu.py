"""`ngs convert --gzip device <SAM> <BAM>` on the GPU.  Two checks throughout: the decompressed output
equals the test-side model's stream (tests/bam_text_model.py) byte for byte, and the text model of the other direction
(tests/sam_model.py) reads the output back as the input text.  The cases: the hand-worked files, the BGZF container, the
edges of the kernels' own steps (a wave takes 64 items at a time), chunk ends on every byte of a line, reference tables of
195 and 5000 names, floats of random bit patterns, every refusal with its index, `-n`, the command line, a randomised slice."""
import gzip
import json
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from ngs_amd import build, host
from ngs_amd.genome_shape import grch38_no_alt
from tests import bamio
from tests import bam_text_model as tm
from tests import sam_model as sm
from tests.test_sam_to_bam import GOOD, HEAD, faulty_lines, hand_spec_text, random_sam

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EOF = bamio.EOF_BLOCK


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def blocks_of(raw: bytes):
    """(BSIZE, ISIZE) of every BGZF block of the file."""
    out, p = [], 0
    while p < len(raw):
        assert raw[p:p + 4] == b"\x1f\x8b\x08\x04" and raw[p + 12:p + 16] == b"BC\x02\x00"
        bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
        out.append((bsize, struct.unpack_from("<I", raw, p + bsize - 4)[0]))
        p += bsize
    assert p == len(raw)
    return out


def convert(lib, sam: bytes, tmp_path, name="o", **kw):
    src, out = str(tmp_path / (name + ".sam")), str(tmp_path / (name + ".bam"))
    with open(src, "wb") as f:
        f.write(sam)
    rep = host.sam_to_bam(src, out, lib=lib, **kw)
    raw = open(out, "rb").read()
    return raw, rep, out


def check(lib, sam: bytes, tmp_path, text_back=True, **kw):
    """Convert, hold the output to the model and to the text model of the other direction; the file's bytes and the report."""
    raw, rep, out = convert(lib, sam, tmp_path, **kw)
    want = tm.bam_stream(sam, kw.get("max_records", 0))
    got = gzip.decompress(raw)
    if got != want:
        k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"stream differs at byte {k} of {len(got)} / {len(want)}: got {got[k - 8:k + 24].hex()} want {want[k - 8:k + 24].hex()}")
    bl = blocks_of(raw)
    assert raw.endswith(EOF) and all(b <= 65536 for b, _ in bl) and all(i > 0 for _, i in bl[:-1]) and bl[-1] == (28, 0)
    assert rep["bam_bytes"] == len(want) and rep["compressed_bytes"] == len(raw) and rep["blocks"] == len(bl) - 1
    if text_back and not kw.get("max_records"):
        assert sm.expected_sam(out) == sam
    return raw, rep, out


def line(*tags, **kw):
    f = list(GOOD)
    for k, v in kw.items():
        f[int(k[1:])] = v
    return "\t".join(f + list(tags)) + "\n"


# ---- 1. hand files ----------------------------------------------------------------------------------------------------------
def test_hand_text(gpu_lib, tmp_path):
    sam = open(os.path.join(GOLDEN, "hand_text.sam"), "rb").read()
    raw, rep, _ = check(gpu_lib, sam, tmp_path, text_back=False)   # (its lower-case SEQ and explicit RNEXT do not print back as written)
    want = json.load(open(os.path.join(GOLDEN, "hand_text_records.json")))
    assert gzip.decompress(raw).endswith(bytes.fromhex("".join(want["records"])))
    assert rep["records"] == 4 and rep["header_bytes"] == len(want["header_text"])


def test_a_failed_write_ends_the_call_with_its_message(gpu_lib, tmp_path):
    """/dev/full refuses every write.  In one chunk the error is read at the end of the run; in chunks of 200 bytes (five jobs:
    the header's and one per record) the wait for the copies of job k - 2 may meet a writer that has already failed (when
    the chunk loop has not seen the failure first), and the call still returns.  The suite has no in-process time limit of
    its own (only subprocess timeouts), so faulthandler ends the process if the call hangs."""
    import faulthandler
    src = os.path.join(GOLDEN, "hand_text.sam")
    _, rep, _ = convert(gpu_lib, open(src, "rb").read(), tmp_path, chunk_bytes=200)
    assert rep["chunks"] == 4   # (with the header's job: five jobs)
    faulthandler.dump_traceback_later(120, exit=True)
    try:
        for chunk in (0, 200):
            with pytest.raises(host.NgsqError) as e:
                host.sam_to_bam(src, "/dev/full", chunk_bytes=chunk, lib=gpu_lib)
            assert "writing BAM record: No space left on device (os error 28)" in str(e.value), chunk
    finally:
        faulthandler.cancel_dump_traceback_later()


def test_hand_spec_and_long_cigar(gpu_lib, tmp_path):
    check(gpu_lib, hand_spec_text(), tmp_path, chunk_bytes=1 << 16)
    check(gpu_lib, sm.expected_sam(os.path.join(GOLDEN, "hand_longcigar.bam")), tmp_path)
    ops = "".join("%d%s" % (1 + k % 3, "MID"[k % 3]) for k in range(70_000))
    l_seq = sum(1 + k % 3 for k in range(70_000) if k % 3 < 2)
    sam = (HEAD + line() + line("NM:i:0", f0="long", f5=ops, f9="A" * l_seq, f10="*") + line()).encode()
    raw, _, _ = check(gpu_lib, sam, tmp_path)
    assert b"NMC\0CGBI" + struct.pack("<I", 70_000) in gzip.decompress(raw)


# ---- 2. container -----------------------------------------------------------------------------------------------------------
def test_container_and_exact_block_fills(gpu_lib, tmp_path):
    body = "".join(line(f"XN:i:{k}", f0=f"q{k}", f3=str(5 + k)) for k in range(400))
    sam = (HEAD.replace("VN:1.6", "VN:1.6\tSO:coordinate") + body).encode()          # (the index is built of sorted files)
    raw, _, out = check(gpu_lib, sam, tmp_path)
    d = zlib.decompressobj(31)
    assert d.decompress(raw[:blocks_of(raw)[0][0]]).startswith(b"BAM\1")
    rep = host.build_bam_index(out, lib=gpu_lib)
    assert rep["records"] == 400
    # a Z tag sized with the model pads one chunk's record bytes to exactly one and exactly two blocks
    base = len(b"".join(tm.bam_records((HEAD + line() + line("ZP:Z:")).encode())))
    for fill in (65280, 2 * 65280):
        sam = (HEAD + line() + line("ZP:Z:" + "p" * (fill - base))).encode()
        assert len(b"".join(tm.bam_records(sam))) == fill
        raw, rep, _ = check(gpu_lib, sam, tmp_path)
        assert [i for _, i in blocks_of(raw)[1:-1]] == [65280] * (fill // 65280)


# ---- 3. wave edges ----------------------------------------------------------------------------------------------------------
def test_wave_edges(gpu_lib, tmp_path):
    rng = np.random.default_rng(41)
    lines = []
    for n in (63, 64, 65, 127, 128, 129, 193):
        cig = "".join("%d%s" % (rng.integers(1, 300), "MIDNSHP=X"[k % 9]) for k in range(n))
        tags = [f"XZ:Z:{'z' * n}", f"XH:H:{'A9' * n}"]
        for sub, lo, hi in (("c", -128, 128), ("C", 0, 256), ("s", -32768, 32768), ("S", 0, 65536), ("i", -2 ** 31, 2 ** 31), ("I", 0, 2 ** 32)):
            tags.append(f"B{sub}:B:{sub}," + ",".join(str(int(x)) for x in rng.integers(lo, hi, n)))
        tags.append("Bf:B:f," + ",".join(sm.fmt_f32(x) for x in rng.standard_normal(n).astype(np.float32)))
        lines.append(line(*tags, f0=f"n{n}", f5=cig))
    for L in (1, 2, 63, 64, 65, 129):
        seq = "".join(rng.choice(list("ACGTN"), L))
        lines.append(line(f0=f"s{L}", f5="*", f9=seq, f10="".join(chr(int(c)) for c in rng.integers(33, 127, L))))
        lines.append(line(f0=f"a{L}", f5="*", f9=seq, f10="*"))
    lines.append(line(f0="s0", f5="*", f9="*", f10="*"))
    fixed = len("\t".join(GOOD)) - len(GOOD[0])                                # the 11th tab at bytes 63, 64, 65 of a piece
    for at in (63, 64, 65, 127, 128):
        lines.append(line("XN:i:1", f0="p" * (at - fixed)))
        assert lines[-1].split("XN")[0].rindex("\t") == at
    lines.append(line(f0="q" * 254))
    L = 100_000
    lines.append(line(f0="long", f5=f"{L}M", f9="".join(rng.choice(list("ACGT"), L)), f10="".join(chr(int(c)) for c in rng.integers(33, 127, L))))
    # the extremes of every fixed field
    lines.append(line(f1="65535", f3="2147483647", f4="255", f7="2147483647", f8="2147483647", f5="268435455M"))
    lines.append(line(f1="0", f2="*", f3="0", f4="0", f6="*", f7="0", f8="-2147483648", f5="*"))
    check(gpu_lib, (HEAD + "".join(lines)).encode(), tmp_path)


# ---- 4. chunk edges ---------------------------------------------------------------------------------------------------------
def test_chunk_edges(gpu_lib, tmp_path):
    sam = random_sam(43, 300, tmp_path)
    longest = max(len(x) for x in sam.split(b"\n"))
    streams = set()
    for chunk in (longest, longest + 1, longest + 37, 1000, 4097):              # chunk ends wander over every byte of the lines
        raw, rep, _ = check(gpu_lib, sam, tmp_path, chunk_bytes=chunk)
        assert rep["chunks"] > 10
        streams.add(gzip.decompress(raw))
    assert len(streams) == 1
    with pytest.raises(host.NgsqError) as e:
        convert(gpu_lib, sam, tmp_path, chunk_bytes=longest - 1)
    k = next(i for i, x in enumerate(tm.body_lines(tm.split_header(sam)[1])) if len(x) == longest)
    assert e.value.message == f"reading SAM record: record {k}: line longer than {longest - 1} bytes"
    check(gpu_lib, sam[:-1], tmp_path, text_back=False, chunk_bytes=1000)        # a last line without its newline
    head = "@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:contig{k}\tLN:{1000 + k}\n" for k in range(300))
    check(gpu_lib, (head + line(f2="contig299", f6="contig0")).encode(), tmp_path, chunk_bytes=256)   # a header longer than a chunk


# ---- 5. references ----------------------------------------------------------------------------------------------------------
def test_reference_tables(gpu_lib, tmp_path):
    names, lens, _ = grch38_no_alt()
    head = "@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in zip(names, lens))
    mate = lambda k, j: "=" if k == j else names[j]                              # (the text model prints a mate on the same sequence as `=`)
    body = "".join(line(f2=names[k], f6=mate(k, j)) for k, j in ((0, 194), (194, 0), (97, 97), (0, 0), (97, 96)))
    check(gpu_lib, (head + body).encode(), tmp_path)
    names = [f"scaffold_{k:04d}" for k in range(5000)] + ["tig0", "tig1", "tigA", "tigB"]      # the last differ in their last byte only
    head = "@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:{n}\tLN:{1000 + k}\n" for k, n in enumerate(names))
    body = "".join(line(f2=names[k], f6=mate(k, (k * 7) % len(names))) for k in list(range(0, 5004, 13)) + [5000, 5001, 5002, 5003])
    raw, _, _ = check(gpu_lib, (head + body).encode(), tmp_path)
    with pytest.raises(host.NgsqError) as e:
        convert(gpu_lib, (head + line() + line(f2="tigC")).encode(), tmp_path)
    assert "record 0: reference sequence name not in the header" in e.value.message        # (GOOD's chr1 is not in this header)


# ---- 6. floats --------------------------------------------------------------------------------------------------------------
def test_floats(gpu_lib, tmp_path):
    rng = np.random.default_rng(44)
    bits = rng.integers(0, 2 ** 32, 20_000, dtype=np.uint64).astype(np.uint32)
    special = np.array([0, 0x80000000, 1, 0x80000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x3F800001], np.uint32)
    texts = [sm.fmt_f32(x) for x in np.concatenate([special, bits]).view(np.float32)]
    texts = [t for t in texts if t != "NaN"]                                     # (a NaN's payload is not in its text)
    lines = [line(f"XF:f:{t}", f0=f"f{k}") for k, t in enumerate(texts[:6000])]  # more float lines than one turn of the float kernels' grid
    lines += [line("XB:B:f," + ",".join(texts[k:k + 100])) for k in range(6000, len(texts), 100)]
    lines.append(line("XE:f:1e5", "Xe:f:-2.5E-3", "Xn:f:nan", "Xi:f:-Infinity", "Xp:f:+.5", "XG:B:f,1e39,1e-46,7.1e-46,3.4028235e38,1.00000005960464477539063"))
    raw, _, _ = check(gpu_lib, (HEAD + "".join(lines)).encode(), tmp_path, text_back=False, chunk_bytes=1 << 20)
    sam = (HEAD + "".join(lines[:-1])).encode()
    check(gpu_lib, sam, tmp_path)                                                # printed patterns read back as the same text


# ---- 7. errors --------------------------------------------------------------------------------------------------------------
def test_every_fault_ends_the_call_with_its_message_and_index(gpu_lib, tmp_path):
    good = "\t".join(GOOD) + "\n"
    for fields, code in faulty_lines():
        sam = (HEAD + good * 5 + "\t".join(fields) + "\n" + good).encode("latin-1")
        with pytest.raises(host.NgsqError) as e:
            convert(gpu_lib, sam, tmp_path)
        assert e.value.message == f"reading SAM record: record 5: {tm.ERROR_TEXT[code]}", fields


def test_the_leftmost_fault_and_the_first_faulty_record(gpu_lib, tmp_path):
    good = "\t".join(GOOD) + "\n"
    two = line("XA:H:ABC", "XB:i:x", f10="III")                                 # QUAL length, then two faulty tags
    for sam, chunk, want in (
            (HEAD + good + two, 0, (1, tm.E_QUAL_LEN)),
            (HEAD + good + line("XA:H:ABC", "XB:i:x"), 0, (1, tm.E_HEX)),
            (HEAD + good * 3 + line(f4="x") + good + line(f1="x"), 0, (3, tm.E_MAPQ)),       # two faulty records in one chunk
            (HEAD + good * 3 + line(f4="x") + good * 40 + line(f1="x"), 200, (3, tm.E_MAPQ)),  # ... in different chunks
            (HEAD + good * 3 + line("XF:f:1.2.3") + good + line(f1="x"), 0, (3, tm.E_NUMBER)),
            # a bad float in front of a tag whose fault has a smaller code: the walk ends at the float
            (HEAD + good + line("XF:f:1.2.3", "XA"), 0, (1, tm.E_NUMBER)),
            (HEAD + good + line("XF:f:1.2.3", "XA:q:1"), 0, (1, tm.E_NUMBER)),
            (HEAD + good + line("XB:B:f,1,x", "XA"), 0, (1, tm.E_NUMBER)),
            (HEAD + good + line("XB:B:f,1,x", "XC:B:q,1"), 0, (1, tm.E_NUMBER)),
            (HEAD + good + line("XB:B:f,1," + "0" * 49, "XA:q:1"), 0, (1, tm.E_FLOAT_LONG)),
            # a good float in front of a faulty tag, and behind a faulty field: the float kernels report the line's faults
            (HEAD + good + line("XF:f:1.5", "XA"), 0, (1, tm.E_TAG_FORM)),
            (HEAD + good + line("XB:B:f,1,2", "XA:q:1"), 0, (1, tm.E_TAG_TYPE)),
            (HEAD + good + line("XF:f:1.5", f4="x"), 0, (1, tm.E_MAPQ)),
            (HEAD + good + line("XA", "XF:f:1.2.3"), 0, (1, tm.E_TAG_FORM))):
        with pytest.raises(host.NgsqError) as e:
            convert(gpu_lib, sam.encode(), tmp_path, chunk_bytes=chunk)
        assert e.value.message == f"reading SAM record: record {want[0]}: {tm.ERROR_TEXT[want[1]]}"
        with pytest.raises(tm.TextError) as m:
            tm.bam_stream(sam.encode())
        assert (m.value.index, m.value.code) == want


# ---- 8. -n, empty files -----------------------------------------------------------------------------------------------------
def test_num_records_and_empty_files(gpu_lib, ngs, tmp_path):
    sam = random_sam(45, 200, tmp_path)
    lines = tm.body_lines(tm.split_header(sam)[1])
    chunk = 2000
    # the records behind which the host cuts its chunks: up to chunk + 1 bytes from the last cut, cut at their last newline
    body, ends, at = tm.split_header(sam)[1], [], 0
    while at < len(body):
        at += body[at:at + chunk + 1].rfind(b"\n") + 1
        ends.append(body[:at].count(b"\n"))
    assert len(ends) > 10 and ends[-1] == 200 and ends[0] > 1
    # 1; inside the first and a later chunk; on the last record of the first and of a later chunk; the file's last; beyond
    for n, chunks in ((1, 1), (ends[0] - 1, 1), (ends[0], 1), (ends[0] + 1, 2), (ends[4], 5), (ends[4] + 1, 6), (200, len(ends)), (10 ** 6, len(ends))):
        raw, rep, _ = check(gpu_lib, sam, tmp_path, max_records=n, chunk_bytes=chunk)
        assert rep["records"] == min(n, 200) and rep["text_bytes"] == sum(len(x) + 1 for x in lines[:n])
        assert rep["chunks"] == chunks, (n, rep["chunks"], chunks)           # (nothing is read or launched behind the last record)
    src = str(tmp_path / "o.sam")
    for n, want in (("0", 1), ("1", 1), ("3", 3), ("500", 200)):                  # the command line: max(N, 1)
        r = subprocess.run([ngs, "convert", "--gzip", "device", "-n", n, src, str(tmp_path / "n.bam")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert gzip.decompress(open(tmp_path / "n.bam", "rb").read()) == tm.bam_stream(sam, want)
    raw, rep, _ = check(gpu_lib, b"", tmp_path)
    assert gzip.decompress(raw) == b"BAM\1" + struct.pack("<ii", 0, 0) and rep["records"] == 0 and len(blocks_of(raw)) == 2
    check(gpu_lib, HEAD.encode(), tmp_path)


# ---- 9. 10. 11. the command line, a randomised slice, determinism -----------------------------------------------------------
def test_cli_sweep_and_determinism(gpu_lib, ngs, tmp_path):
    sam = random_sam(46, 6000, tmp_path)
    raw, rep, out = check(gpu_lib, sam, tmp_path, chunk_bytes=60_000)
    assert rep["chunks"] >= 20
    again, _, _ = convert(gpu_lib, sam, tmp_path, name="again", chunk_bytes=60_000)
    assert again == raw
    r = subprocess.run([ngs, "convert", "--gzip", "device", "-c", "best", str(tmp_path / "o.sam"), str(tmp_path / "cli.bam")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lib_default, _, _ = convert(gpu_lib, sam, tmp_path, name="dflt")
    assert open(tmp_path / "cli.bam", "rb").read() == lib_default
    r = subprocess.run([ngs, "convert", str(tmp_path / "cli.bam"), str(tmp_path / "back.sam")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "back.sam", "rb").read() == sam                       # both directions of the command
