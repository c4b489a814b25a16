"""`ngs convert <BAM> <SAM>` without a GPU: the test-side model (tests/sam_model.py) pinned on the
hand-worked golden text and on records of known columns, the float and `-n` rules, and the command line's surface and
refusals, which all come before any GPU work."""
import os
import struct
import subprocess

import numpy as np
import pytest

from ngs_amd import build
from tests import bamio
from tests import sam_model as sm
from tests.util import random_batch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["chr1", "chr2", "chr3"]
LENS = [300_000, 70_000, 5_000]


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def run(ngs, *args, cwd=None):
    return subprocess.run([ngs, *args], capture_output=True, text=True, timeout=120, cwd=cwd)


def test_model_equals_the_hand_worked_golden():
    want = open(os.path.join(GOLDEN, "hand_spec.sam"), "rb").read()
    assert sm.expected_sam(os.path.join(GOLDEN, "hand_spec.bam")) == want
    assert sm.count_records(os.path.join(GOLDEN, "hand_spec.bam")) == 8


def test_model_resolves_the_long_cigar():
    text = sm.expected_sam(os.path.join(GOLDEN, "hand_longcigar.bam")).decode()
    line = text.splitlines()[-1].split("\t")
    assert line[5] == "10M5D20M" and line[11:] == ["NM:i:0"]          # the CG tag is the CIGAR, not a tag


def parse_line(line: bytes, names):
    """The columns a SAM line says (the inverse of section 13.1), and its tags."""
    f = line.split(b"\t")
    ref = -1 if f[2] == b"*" else names.index(f[2].decode())
    mate = -1 if f[6] == b"*" else ref if f[6] == b"=" else names.index(f[6].decode())
    ops = []
    if f[5] != b"*":
        num = b""
        for ch in f[5]:
            if 48 <= ch <= 57:
                num += bytes([ch])
            else:
                ops.append(int(num) << 4 | sm.CIGAR_OPS.index(chr(ch)))
                num = b""
    seq = b"" if f[9] == b"*" else f[9]
    qual = None if f[10] == b"*" else [c - 33 for c in f[10]]
    return dict(name=f[0], flag=int(f[1]), ref_id=ref, pos=int(f[3]) - 1, mapq=int(f[4]), cigar=ops, mate_ref_id=mate,
                next_pos=int(f[7]) - 1, tlen=int(f[8]), seq=seq, qual=qual, tags=f[11:])


def test_records_of_known_columns_parse_back():
    """bamio writes records from known columns; the model's text, read back, gives those columns."""
    import tempfile
    rng = np.random.default_rng(5)
    hb = random_batch(rng, 3000, LENS, max_len=160)
    names = [bamio.aligner_name(rng) for _ in range(hb.n)]
    aux = [bamio.aligner_aux(rng, int(hb.cols["l_seq"][i])) for i in range(hb.n)]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "k.bam")
        bamio.write_bam(path, hb, NAMES, LENS, block_payload=5000, with_index=False, names=names, aux=aux)
        text = sm.expected_sam(path)
    lines = text.split(b"\n")[:-1]
    head = [x for x in lines if x.startswith(b"@")]
    body = [x for x in lines if not x.startswith(b"@")]
    assert head == [b"@HD\tVN:1.6\tSO:coordinate"] + [b"@SQ\tSN:%s\tLN:%d" % (n.encode(), ln) for n, ln in zip(NAMES, LENS)]
    assert len(body) == hb.n
    c = hb.cols
    for i, line in enumerate(body):
        r = parse_line(line, NAMES)
        assert r["name"] == names[i]
        for k in ("flag", "ref_id", "pos", "mapq", "mate_ref_id", "tlen"):
            assert r[k] == int(c[k][i]), (i, k)
        assert r["next_pos"] == -1                                     # (bamio writes next_pos -1)
        assert r["cigar"] == [int(x) for x in c["cigar"][int(c["cigar_off"][i]):int(c["cigar_off"][i + 1])]]
        L = int(c["l_seq"][i])
        packed = c["seq"][int(c["seq_off"][i]):int(c["seq_off"][i + 1])]
        codes = [(int(packed[k >> 1]) >> (0 if k & 1 else 4)) & 15 for k in range(L)]
        assert r["seq"] == "".join(sm.SEQ_CODES[x] for x in codes).encode()
        q = c["qual"][int(c["qual_off"][i]):int(c["qual_off"][i + 1])]
        assert r["qual"] == (None if len(q) != L or L == 0 else [int(x) for x in q])
        tags = [t[:2] for t in r["tags"]]
        assert tags[:1] in ([b"NM"], [b"MC"]) and b"RG" in tags


@pytest.mark.parametrize("x,text", [
    (1.0, "1"), (3.5, "3.5"), (0.1, "0.1"), (-1.5, "-1.5"), (0.25, "0.25"), (1e10, "10000000000"),
    (1e20, "100000000000000000000"), (1e-45, "0.000000000000000000000000000000000000000000001"),
    (3.4028234663852886e38, "340282350000000000000000000000000000000"), (16777216.0, "16777216"), (2097152.25, "2097152.2"),
    (2097152.75, "2097152.8"), (float("nan"), "NaN"), (float("inf"), "inf"), (float("-inf"), "-inf"), (0.0, "0"), (-0.0, "-0"),
    (1e9, "1000000000"), (123456.79, "123456.79"), (5e-324, "0")])
def test_float_rule(x, text):
    assert sm.fmt_f32(x) == text


def test_float_text_reads_back_and_is_short():
    rng = np.random.default_rng(6)
    bits = rng.integers(0, 2 ** 32, 20_000, dtype=np.uint64).astype(np.uint32)
    for f in bits.view(np.float32):
        t = sm.fmt_f32(f)
        assert "e" not in t and not t.endswith(".0")
        if np.isfinite(f):
            assert np.float32(t) == f or (f == 0 and float(t) == 0)
            assert len(t) <= 48


def reference_counter(n_records, num_records):
    """src/convert/bam.rs:50-66 with utils/display.rs:58-63: write, inc, break when count >= limit."""
    written = 0
    for _ in range(n_records):
        written += 1
        if num_records is not None and written >= num_records:
            break
    return written


@pytest.mark.parametrize("total", [0, 1, 2, 999, 1000])
@pytest.mark.parametrize("num", [None, 0, 1, 2, 500, 999, 1000, 1001, 10 ** 6])
def test_num_records_arithmetic(total, num):
    assert sm.records_written(total, num) == reference_counter(total, num)


def test_convert_help_shows_the_reference_surface(ngs):
    r = run(ngs, "convert", "--help")
    assert r.returncode == 0
    h = r.stderr + r.stdout
    for s in ("<FROM>", "<TO>", "-n, --num-records <USIZE>", "-r, --reference-fasta <REFERENCE_FASTA>",
              "-c, --compression-strategy <COMPRESSION_STRATEGY>", "[default: balanced]", "best, balanced, fastest", "--device <N>"):
        assert s in h, s
    r = run(ngs, "--help")
    assert "convert" in r.stderr + r.stdout


@pytest.fixture(scope="module")
def small_bam(tmp_path_factory):
    d = tmp_path_factory.mktemp("c")
    hb = random_batch(np.random.default_rng(7), 20, LENS)
    path = str(d / "in.bam")
    bamio.write_bam(path, hb, NAMES, LENS, with_index=False)
    return path


def refusals(src_bam, d):
    """(arguments, message): every refusal of the command line."""
    sam, gff = os.path.join(d, "x.sam"), os.path.join(d, "x.gff")
    for p in (sam, gff):
        open(p, "w").close()
    return [
        (["x.unknown", os.path.join(d, "o.sam")], "failed to detect from input filetype: x.unknown: Failed parsing of bioinformatics file format."),
        ([src_bam, os.path.join(d, "o.txt")], f"failed to deteect to input filetype: {os.path.join(d, 'o.txt')}: Failed parsing of bioinformatics file format."),
        ([src_bam, os.path.join(d, "o.fastq")], "Conversion from BAM to FASTQ is not currently supported"),
        ([src_bam, os.path.join(d, "o.bam")], "Conversion from BAM to BAM is not currently supported"),
        ([sam, os.path.join(d, "o.sam")], "Conversion from SAM to SAM is not currently supported"),
        ([sam, os.path.join(d, "o.bam")], "Conversion from SAM to BAM is done by the reference `ngs convert` but not by this build, which converts BAM to SAM only"),
        ([gff, os.path.join(d, "o.gff.bgz")], "Conversion from GFF to Block-gzipped GFF is done by the reference `ngs convert` but not by this build, which converts BAM to SAM only"),
        ([src_bam, os.path.join(d, "o.cram")], "--reference-fasta is a required argument when converting to/from a CRAM file"),
        ([sam, os.path.join(d, "o.cram")], "--reference-fasta is a required argument when converting to/from a CRAM file"),
        (["x.cram", os.path.join(d, "o.sam")], "--reference-fasta is a required argument when converting to/from a CRAM file"),
        (["x.cram", os.path.join(d, "o.bam")], "--reference-fasta is a required argument when converting to/from a CRAM file"),
        (["-r", "ref.fa", src_bam, os.path.join(d, "o.cram")], "Conversion from BAM to CRAM is done by the reference `ngs convert` but not by this build, which converts BAM to SAM only"),
        (["-r", "ref.fa", "x.cram", os.path.join(d, "o.sam")], "Conversion from CRAM to SAM is done by the reference `ngs convert` but not by this build, which converts BAM to SAM only"),
        ([os.path.join(d, "missing.bam"), os.path.join(d, "o.sam")], "opening BAM input file: "),
    ]


def test_every_refusal_prints_its_message_and_creates_nothing(ngs, small_bam, tmp_path):
    for args, msg in refusals(small_bam, str(tmp_path)):
        before = set(os.listdir(tmp_path))
        r = run(ngs, "convert", *args)
        assert r.returncode == 1, (args, r.stderr)
        assert "Error: " + msg in r.stderr, (args, r.stderr)
        assert set(os.listdir(tmp_path)) == before, args               # no <TO>


def test_output_that_cannot_be_created(ngs, small_bam, tmp_path):
    r = run(ngs, "convert", small_bam, str(tmp_path / "no_such_dir" / "o.sam"))
    assert r.returncode == 1
    assert "Error: creating SAM output file: No such file or directory (os error 2)" in r.stderr


def test_argument_errors(ngs, small_bam, tmp_path):
    r = run(ngs, "convert", small_bam)
    assert r.returncode == 1 and "required arguments" in r.stderr and "<TO>" in r.stderr
    r = run(ngs, "convert", "-c", "quick", small_bam, str(tmp_path / "o.sam"))
    assert r.returncode == 1 and "possible values: best, balanced, fastest" in r.stderr
    r = run(ngs, "convert", "-n", "ten", small_bam, str(tmp_path / "o.sam"))
    assert r.returncode == 1 and "--num-records <USIZE>" in r.stderr
    assert not os.path.exists(tmp_path / "o.sam")


def test_model_refuses_each_error_class():
    """One planted record of each kind: the model's SamError names its index and kind (the GPU tests hold the library to it)."""
    import tempfile
    from tests.util import batch_from_records
    good = dict(flag=0, mapq=60, ref_id=0, pos=5, mate_ref_id=0, tlen=0, cigar="4M", seq="ACGT", qual=[30, 31, 32, 33])
    cases = [({}, b"XXq\x01", sm.E_TAG_TYPE), ({}, b"XZZabc", sm.E_STR_NUL), ({}, b"XBBq" + struct.pack("<I", 1) + b"\0", sm.E_B_SUB),
             ({}, b"XBBi" + struct.pack("<I", 9) + b"\0" * 8, sm.E_OVERRUN), ({"qual": [1, 2, 94, 3]}, b"", sm.E_QUAL),
             ({"cigar": [32, 41]}, b"", sm.E_CIGAR_OP), ({"ref_id": 3}, b"", sm.E_REF)]
    with tempfile.TemporaryDirectory() as d:
        for over, aux, code in cases:
            recs = [dict(good), dict(good), dict(good, **over)]
            path = os.path.join(d, "e.bam")
            bamio.write_bam(path, batch_from_records(recs), NAMES, LENS, with_index=False, aux=[b"", b"", aux])
            with pytest.raises(sm.SamError) as e:
                sm.expected_sam(path)
            assert (e.value.index, e.value.code) == (2, code)
            assert e.value.message == f"writing SAM record: record 2: {sm.ERROR_TEXT[code]}"
            assert sm.expected_sam(path, 2).count(b"\n") == 4 + 2
