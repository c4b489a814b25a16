"""`ngs convert --gzip device <SAM> <BAM>` without a GPU: the test-side model (tests/bam_text_model.py)
pinned on a hand-worked fixture and on the text round trip through tests/sam_model.py, the float rule held against exact
fractions (the model's, and the library's own parser on the host), every refusal of the model, and the command line's surface
and refusals, which all come before any GPU work.

The tests named test_model_*, and test_an_empty_file_and_a_header_alone, run the model alone: they pin the yardstick the GPU
tests (tests/test_sam_to_bam_gpu.py) hold the library to, not the feature, and pass without it.  The float, fixture-generator
and command-line tests call the library or the command."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from ngs_amd import build, host
from tests import bamio
from tests import bam_text_model as tm
from tests import sam_model as sm
from tests.util import random_batch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["chr1", "chr2", "chr3"]
LENS = [300_000, 70_000, 5_000]
HEAD = "@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in zip(NAMES, LENS))
REFUSAL = "Error: Conversion from SAM to BAM is done by the reference `ngs convert` but not by this build, which converts BAM to SAM only"


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def run(ngs, *args):
    return subprocess.run([ngs, *args], capture_output=True, text=True, timeout=120)


def test_model_equals_the_hand_worked_fixture():
    sam = open(os.path.join(GOLDEN, "hand_text.sam"), "rb").read()
    want = json.load(open(os.path.join(GOLDEN, "hand_text_records.json")))
    assert [r.hex() for r in tm.bam_records(sam)] == want["records"]
    header, _ = tm.split_header(sam)
    assert header.decode() == want["header_text"]
    assert [(n.decode(), l) for n, l in tm.references(header)] == [tuple(x) for x in want["references"]]
    stream = tm.bam_stream(sam)
    assert stream.startswith(b"BAM\1" + struct.pack("<i", len(header)) + header + struct.pack("<i", 3) + struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", 1000))
    assert stream.endswith(bytes.fromhex(want["records"][-1]))


def test_the_fixture_is_what_its_generator_writes(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_hand_text_sam", os.path.join(GOLDEN, "make_hand_text_sam.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    text = m.HEADER + "".join("\t".join(f) + "\n" for f, _ in m.TABLE)
    assert open(os.path.join(GOLDEN, "hand_text.sam"), "rb").read() == text.encode()
    assert json.load(open(os.path.join(GOLDEN, "hand_text_records.json")))["records"] == [r.hex() for _, r in m.TABLE]


def round_trip(sam: bytes, tmp_path):
    path = str(tmp_path / "rt.bam")
    with open(path, "wb") as f:
        f.write(tm.bam_file(tm.bam_stream(sam), 5000))
    return sm.expected_sam(path)


def random_sam(seed, n, tmp_path):
    """The SAM text of n random records with aligner tags and names (no tab or newline in any Z value)."""
    rng = np.random.default_rng(seed)
    hb = random_batch(rng, n, LENS, max_len=160)
    aux = [bamio.aligner_aux(rng, int(hb.cols["l_seq"][i])) for i in range(hb.n)]
    names = [bamio.aligner_name(rng) for _ in range(hb.n)]
    path = str(tmp_path / "src.bam")
    bamio.write_bam(path, hb, NAMES, LENS, block_payload=7000, with_index=False, names=names, aux=aux)
    text = sm.expected_sam(path)
    import re
    body = [x for x in text.split(b"\n")[:-1] if not x.startswith(b"@")]                # no Z value holds a tab or a newline:
    assert len(body) == n and all(re.match(rb"..:[AifZHB]:", t) for x in body for t in x.split(b"\t")[11:])   # every piece is a tag
    return text


def hand_spec_text():
    """tests/golden/hand_spec.sam with the one tab inside its XZ:Z value made a space: section 13.1 copies Z bytes as they
    are, so that value reads as two fields in SAM text (the ambiguity section 18.1 names); every other byte is the file's."""
    sam = open(os.path.join(GOLDEN, "hand_spec.sam"), "rb").read()
    assert sam.count(b"with spaces \t and a tab") == 1
    return sam.replace(b"with spaces \t and a tab", b"with spaces   and a tab")


def test_model_text_round_trip(tmp_path):
    for sam in (hand_spec_text(), sm.expected_sam(os.path.join(GOLDEN, "hand_longcigar.bam")),
                random_sam(31, 1500, tmp_path)):
        assert round_trip(sam, tmp_path) == sam


def test_model_moves_a_long_cigar_to_its_cg_tag(tmp_path):
    """More than 65535 operations: <l_seq>S<span>N in the record and a CG:B,I tag behind the line's own tags, which the text
    model reads back as the CIGAR."""
    ops = "".join("%d%s" % (1 + k % 3, "MID"[k % 3]) for k in range(70_000))
    l_seq = sum(1 + k % 3 for k in range(70_000) if k % 3 < 2)
    span = sum(1 + k % 3 for k in range(70_000) if k % 3 != 1)
    sam = (HEAD + "\t".join(["long", "0", "chr1", "51", "30", ops, "*", "0", "0", "A" * l_seq, "*", "NM:i:0"]) + "\n").encode()
    rec = tm.bam_records(sam)[0]
    assert struct.unpack_from("<H", rec, 16)[0] == 2
    assert struct.unpack_from("<II", rec, 36 + 5) == (l_seq << 4 | 4, span << 4 | 3)
    assert rec[-(8 + 4 * 70_000):][:8] == b"CGBI" + struct.pack("<I", 70_000) and b"NMC\0CGBI" in rec
    assert round_trip(sam, tmp_path) == sam


def test_float_rule_reads_back_every_printed_pattern(lib):
    """fmt_f32 prints the shortest text that reads back: the model (exact fractions) and the library's parser return the bits."""
    rng = np.random.default_rng(8)
    bits = rng.integers(0, 2 ** 32, 10_000, dtype=np.uint64).astype(np.uint32)
    for u, f in zip(bits.tolist(), bits.view(np.float32)):
        t = sm.fmt_f32(f).encode()
        want = u if not np.isnan(f) else 0x7FC00000
        assert tm.parse_f32(t) == want, t
        assert host.sam_parse_f32(t, lib) == want, t


@pytest.mark.parametrize("text,bits", [
    # 1 + 2^-24 is the midpoint of 1 and its successor: a tie goes to the even mantissa, a digit above it goes up
    ("1.000000059604644775390625", 0x3F800000), ("1.00000005960464477539062", 0x3F800000), ("1.00000005960464477539063", 0x3F800001),
    ("1.000000178813934326171875", 0x3F800002), ("1.00000017881393432617187", 0x3F800001),
    # the largest float, the midpoint to 2^128 (a tie, to the even side: infinity) and one digit under it
    ("340282346638528859811704183484516925440", 0x7F7FFFFF), ("340282356779733661637539395458142568448", 0x7F800000),
    ("340282356779733661637539395458142568447", 0x7F7FFFFF), ("1e39", 0x7F800000), ("-1e39", 0xFF800000),
    # the smallest denormal 2^-149 = 1.4e-45 and half of it (a tie, to zero)
    ("1e-45", 1), ("7.1e-46", 1), ("7e-46", 0), ("-1e-46", 0x80000000), ("1.17549435e-38", 0x00800000), ("1.1754942e-38", 0x007FFFFF),
    ("0", 0), ("-0", 0x80000000), ("+1.5", 0x3FC00000), (".5", 0x3F000000), ("5.", 0x40A00000), ("1E5", 0x47C35000), ("1e-5", 0x3727C5AC),
    ("inf", 0x7F800000), ("-Infinity", 0xFF800000), ("+INF", 0x7F800000), ("NaN", 0x7FC00000), ("-nan", 0xFFC00000),
    ("1e99999999999", 0x7F800000), ("1e-99999999999", 0), ("0e99999", 0)])
def test_float_cases(lib, text, bits):
    assert tm.parse_f32(text.encode()) == bits
    assert host.sam_parse_f32(text, lib) == bits


@pytest.mark.parametrize("text", ["", "+", ".", "e5", "1e", "1e+", "1.2.3", "0x10", "1 ", "in", "infinit", "nane", "1" * 49])
def test_texts_that_are_no_float(lib, text):
    assert len(text) > 48 or tm.parse_f32(text.encode()) is None
    with pytest.raises(host.NgsqError):
        host.sam_parse_f32(text, lib)


GOOD = ["r", "0", "chr1", "5", "60", "4M", "=", "9", "0", "ACGT", "IIII"]


def faulty_lines():
    """(fields, code): one line of each kind of fault of section 18.1."""
    def g(**kw):
        f = list(GOOD)
        for k, v in kw.items():
            f[int(k[1:])] = v
        return f
    return [
        (GOOD[:10], tm.E_FIELDS), (g(f0=""), tm.E_QNAME_EMPTY), (g(f0="q" * 255), tm.E_QNAME_LONG), (g(f1="x"), tm.E_FLAG), (g(f1="65536"), tm.E_FLAG),
        (g(f2="chr9"), tm.E_RNAME), (g(f3="-1"), tm.E_POS), (g(f3="2147483648"), tm.E_POS), (g(f4="256"), tm.E_MAPQ), (g(f4=""), tm.E_MAPQ),
        (g(f5="M"), tm.E_CIGAR_DIGITS), (g(f5="4M3"), tm.E_CIGAR_DIGITS), (g(f5="4Q"), tm.E_CIGAR_OP), (g(f5="268435456M"), tm.E_CIGAR_LEN),
        (g(f6="chrX"), tm.E_RNEXT), (g(f7="1e3"), tm.E_PNEXT), (g(f8="2147483648"), tm.E_TLEN), (g(f8="-2147483649"), tm.E_TLEN), (g(f8="+5"), tm.E_TLEN),
        (g(f9="ACXT"), tm.E_SEQ), (g(f9="*"), tm.E_QUAL_NO_SEQ), (g(f10="III"), tm.E_QUAL_LEN), (g(f10="II I"), tm.E_QUAL_CHAR), (g(f10="II\x7fI"), tm.E_QUAL_CHAR),
        (GOOD + ["XA:i"], tm.E_TAG_FORM), (GOOD + ["XAi:5"], tm.E_TAG_FORM), (GOOD + ["XA:A:ab"], tm.E_TAG_FORM), (GOOD + [""], tm.E_TAG_FORM),
        (GOOD + ["XA:q:1"], tm.E_TAG_TYPE), (GOOD + ["XA:c:1"], tm.E_TAG_TYPE), (GOOD + ["XA:B:q,1"], tm.E_B_SUB),
        (GOOD + ["XA:i:1x"], tm.E_NUMBER), (GOOD + ["XA:i:4294967296"], tm.E_NUMBER), (GOOD + ["XA:i:-2147483649"], tm.E_NUMBER), (GOOD + ["XA:i:"], tm.E_NUMBER),
        (GOOD + ["XA:f:1.2.3"], tm.E_NUMBER), (GOOD + ["XA:B:c,128"], tm.E_NUMBER), (GOOD + ["XA:B:C,-1"], tm.E_NUMBER), (GOOD + ["XA:B:S,1,,2"], tm.E_NUMBER),
        (GOOD + ["XA:B:c1"], tm.E_NUMBER), (GOOD + ["XA:B:f,1,x"], tm.E_NUMBER), (GOOD + ["XA:H:ABC"], tm.E_HEX), (GOOD + ["XA:H:AG"], tm.E_HEX),
        (GOOD + ["XA:f:" + "1" * 49], tm.E_FLOAT_LONG), (GOOD + ["XA:B:f,1," + "0" * 49], tm.E_FLOAT_LONG),
    ]


def test_model_refuses_each_fault_with_its_message():
    good = "\t".join(GOOD) + "\n"
    for fields, code in faulty_lines():
        sam = (HEAD + good + good + "\t".join(fields) + "\n" + good).encode("latin-1")
        with pytest.raises(tm.TextError) as e:
            tm.bam_stream(sam)
        assert (e.value.index, e.value.code) == (2, code), fields
        assert e.value.message == f"reading SAM record: record 2: {tm.ERROR_TEXT[code]}"
        assert len(tm.bam_records(sam, 2)) == 2
    # two faults in one line: the one further left; two faulty tags: the first
    assert tm.record("\t".join(["r", "x", "chr1", "5", "60", "4M", "=", "9", "0", "ACGT", "III"]).encode(), {b"chr1": 0})[1] == tm.E_FLAG
    assert tm.record("\t".join(GOOD + ["XA:H:ABC", "XB:i:x"]).encode(), {b"chr1": 0})[1] == tm.E_HEX
    assert tm.record("\t".join(GOOD + ["XB:i:x", "XA"]).encode(), {b"chr1": 0})[1] == tm.E_NUMBER


HEADER_REFUSALS = [
    ("@SQ\tLN:5\n", "@SQ line 1 has no SN"), ("@SQ\tSN:a\tLN:5\n@SQ\tSN:b\n", "@SQ line 2 (b) has no LN"),
    ("@SQ\tSN:a\tLN:0\n", "@SQ line 1 (a): LN 0 is outside 1..2147483647"), ("@SQ\tSN:a\tLN:2147483648\n", "@SQ line 1 (a): LN 2147483648 is outside 1..2147483647"),
    ("@SQ\tSN:a\tLN:5x\n", "@SQ line 1 (a): LN 5x is outside 1..2147483647"),
    ("@SQ\tSN:a\tLN:5\n@SQ\tSN:a\tLN:6\n", "@SQ line 2: the sequence name a stands in more than one @SQ line")]


def test_model_refuses_each_header():
    for text, msg in HEADER_REFUSALS:
        with pytest.raises(tm.HeaderError) as e:
            tm.bam_stream(text.encode())
        assert str(e.value) == "opening SAM input file: " + msg


def test_an_empty_file_and_a_header_alone():
    assert tm.bam_stream(b"") == b"BAM\1" + struct.pack("<ii", 0, 0)
    assert tm.bam_stream(HEAD.encode()).endswith(b"chr3\0" + struct.pack("<i", 5000))
    assert len(tm.bam_records((HEAD + "\t".join(GOOD)).encode())) == 1          # a last line without its newline is a line


# ---- the command line ---------------------------------------------------------------------------------------------------
def test_help_names_the_flag_and_the_direction(ngs):
    r = run(ngs, "convert", "--help")
    h = r.stderr + r.stdout
    assert r.returncode == 0
    for s in ("--gzip <WHERE>", "[possible values: host, device]", "SAM to BAM"):
        assert s in h, s


def test_gzip_values(ngs, tmp_path):
    sam = tmp_path / "x.sam"
    sam.write_text(HEAD)
    for v in ("gpu", "", "Device"):
        r = run(ngs, "convert", "--gzip", v, str(sam), str(tmp_path / "o.bam"))
        assert r.returncode == 1 and f"Error: invalid value '{v}' for '--gzip <WHERE>' [possible values: host, device]" in r.stderr
    for args in (["--gzip", "host"], []):                                        # today's refusal, unchanged
        r = run(ngs, "convert", *args, str(sam), str(tmp_path / "o.bam"))
        assert r.returncode == 1 and REFUSAL in r.stderr
    r = run(ngs, "convert", "--gzip", "device", "-c", "quick", str(sam), str(tmp_path / "o.bam"))
    assert r.returncode == 1 and "possible values: best, balanced, fastest" in r.stderr
    # with BAM to SAM the flag takes no part: the refusals of that direction stay
    r = run(ngs, "convert", "--gzip", "device", str(tmp_path / "missing.bam"), str(tmp_path / "o.sam"))
    assert r.returncode == 1 and "Error: opening BAM input file: " in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["x.sam"]


def test_input_and_output_refusals_come_before_any_gpu_work(ngs, tmp_path):
    r = run(ngs, "convert", "--gzip", "device", str(tmp_path / "missing.sam"), str(tmp_path / "o.bam"))
    assert r.returncode == 1 and "Error: opening SAM input file: No such file or directory (os error 2)" in r.stderr
    assert os.listdir(tmp_path) == []
    sam = tmp_path / "x.sam"
    sam.write_text(HEAD)
    r = run(ngs, "convert", "--gzip", "device", str(sam), str(tmp_path / "no_such_dir" / "o.bam"))
    assert r.returncode == 1 and "Error: opening BAM output file: No such file or directory (os error 2)" in r.stderr
    for k, (text, msg) in enumerate(HEADER_REFUSALS):
        bad = tmp_path / f"h{k}.sam"
        bad.write_text(text)
        r = run(ngs, "convert", "--gzip", "device", str(bad), str(tmp_path / "o.bam"))
        assert r.returncode == 1 and "Error: opening SAM input file: " + msg in r.stderr, (text, r.stderr)
        with pytest.raises(host.NgsqError) as e:
            host.sam_to_bam(str(bad), str(tmp_path / "o.bam"))
        assert e.value.message == "opening SAM input file: " + msg
    assert not os.path.exists(tmp_path / "o.bam")
