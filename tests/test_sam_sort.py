"""`ngs convert --gzip device --sort coordinate <SAM> <BAM>` without a GPU: the test-side model
(tests/sort_model.py) held to cases worked by hand, the library's header rewrite (ngsq_sam_sorted_header, host only) held to
the model, and the command line's surface and refusals, which all come before any GPU work."""
import os
import struct
import subprocess

import pytest

from ngs_amd import build, ffi, host
from tests import bam_text_model as tm
from tests import sort_model as som
from tests.test_sam_to_bam import HEAD, REFUSAL

GOOD = ["r", "0", "chr1", "5", "60", "4M", "=", "9", "0", "ACGT", "IIII"]


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def run(ngs, *args):
    return subprocess.run([ngs, *args], capture_output=True, text=True, timeout=120)


def line(name, rname, pos, *tags):
    f = list(GOOD)
    f[0], f[2], f[3] = name, rname, str(pos)
    if rname == "*":
        f[6] = "*"
    return "\t".join(f + list(tags)) + "\n"


def rec(ref_id, pos):
    return struct.pack("<iii", 32, ref_id, pos) + b"\0" * 24


# ---- the model against hand-worked cases ------------------------------------------------------------------------------------
def test_model_key_rule():
    assert som.key(rec(0, 0)) == 1                                      # chr1 POS 1
    assert som.key(rec(2, 99)) == 2 << 32 | 100
    assert som.key(rec(299, 2 ** 31 - 2)) == 299 << 32 | 0x7FFFFFFF     # POS 2^31 - 1: the top position digit
    assert som.key(rec(-1, -1)) == 0xFFFFFFFF << 32                     # RNAME * POS 0
    assert som.key(rec(0, -1)) == 0xFFFFFFFF << 32                      # chr1 POS 0: no position, so last
    assert som.key(rec(-1, 6)) == 0xFFFFFFFF << 32 | 7                  # RNAME * with a POS: last too
    assert som.key(rec(0, -1)) > som.key(rec(2 ** 31 - 1, 2 ** 31 - 2))  # behind every placed record
    # through the text: the fields of the line decide
    recs = tm.bam_records((HEAD + line("a", "chr1", 0) + line("b", "*", 0) + line("c", "chr3", 5000)).encode())
    assert [som.key(r) for r in recs] == [0xFFFFFFFF << 32, 0xFFFFFFFF << 32, 2 << 32 | 5000]


def test_model_order_is_stable():
    assert som.order([]) == [] and som.order([7]) == [0]
    assert som.order([5, 3, 5, 3, 1]) == [4, 1, 3, 0, 2]
    assert som.order([9, 9, 9]) == [0, 1, 2]


HAND = [("u0", "*", 0), ("c2p9", "chr2", 9), ("c1p7", "chr1", 7), ("c1p0", "chr1", 0), ("c1p7b", "chr1", 7), ("c3p1", "chr3", 1),
        ("u1", "*", 0), ("c1p1", "chr1", 1), ("c2p9b", "chr2", 9), ("c1p300000", "chr1", 300000), ("c2p1", "chr2", 1), ("c1p7c", "chr1", 7)]
HAND_ORDER = ["c1p1", "c1p7", "c1p7b", "c1p7c", "c1p300000", "c2p1", "c2p9", "c2p9b", "c3p1", "u0", "c1p0", "u1"]


def hand_text():
    return (HEAD + "".join(line(n, r, p, f"XI:i:{k}") for k, (n, r, p) in enumerate(HAND))).encode()


def test_model_stream_of_a_dozen_hand_written_lines():
    sam = hand_text()
    by_name = {r[36:36 + r[12] - 1].decode(): r for r in tm.bam_records(sam)}
    header = HEAD.replace("@HD\tVN:1.6\n", "@HD\tVN:1.6\tSO:coordinate\n").encode()
    want = tm.header_stream(header, [(b"chr1", 300_000), (b"chr2", 70_000), (b"chr3", 5_000)]) + b"".join(by_name[n] for n in HAND_ORDER)
    assert som.bam_stream(sam) == want
    assert [x.split(b"\t")[0].decode() for x in som.sorted_lines(sam)] == HAND_ORDER
    # max_records: the first records of the text, sorted
    assert [x.split(b"\t")[0].decode() for x in som.sorted_lines(sam, 4)] == ["c1p7", "c2p9", "u0", "c1p0"]
    assert som.bam_stream(sam, 4).endswith(by_name["c1p7"] + by_name["c2p9"] + by_name["u0"] + by_name["c1p0"])
    # a faulty line is the model's refusal, with the index in the text
    with pytest.raises(tm.TextError) as e:
        som.bam_stream(sam + line("bad", "chr9", 1).encode())
    assert (e.value.index, e.value.code) == (12, tm.E_RNAME)


SQ = "@SQ\tSN:chr1\tLN:1000\n"
HEADERS = [
    # (header text, the sorted file's, worked by hand)
    ("@HD\tVN:1.6\tSO:unsorted\n" + SQ, "@HD\tVN:1.6\tSO:coordinate\n" + SQ),
    ("@HD\tVN:1.6\tSO:queryname\tSS:queryname:natural\n" + SQ, "@HD\tVN:1.6\tSO:coordinate\n" + SQ),
    ("@HD\tVN:1.6\tSO:coordinate\tSS:coordinate:x\n" + SQ, "@HD\tVN:1.6\tSO:coordinate\tSS:coordinate:x\n" + SQ),
    ("@HD\tVN:1.6\n" + SQ, "@HD\tVN:1.6\tSO:coordinate\n" + SQ),
    ("@HD\tVN:1.6\tGO:query\n" + SQ + "@CO\tSO:unsorted\n", "@HD\tVN:1.6\tGO:query\tSO:coordinate\n" + SQ + "@CO\tSO:unsorted\n"),
    ("@HD\tSS:queryname:natural\tVN:1.6\tSO:unknown\tSO:unsorted\n", "@HD\tVN:1.6\tSO:coordinate\tSO:unsorted\n"),
    (SQ + "@HD\tVN:1.5\tSO:unsorted\n@CO\tx\n", SQ + "@HD\tVN:1.5\tSO:coordinate\n@CO\tx\n"),       # @HD not first
    (SQ + "@CO\tnothing\n", "@HD\tVN:1.6\tSO:coordinate\n" + SQ + "@CO\tnothing\n"),              # no @HD
    ("", "@HD\tVN:1.6\tSO:coordinate\n"),                                                         # an empty header
    ("@HD\tVN:1.6", "@HD\tVN:1.6\tSO:coordinate"),                                                 # a last line without its newline
    ("@HD", "@HD\tSO:coordinate"),
]


def test_model_sorted_header():
    for text, want in HEADERS:
        assert som.sorted_header(text.encode()) == want.encode(), text


def test_library_sorted_header_equals_the_model(lib):
    for text, want in HEADERS:
        assert host.sam_sorted_header(text.encode(), lib=lib) == want.encode(), text
        assert host.sam_sorted_header(text.encode(), cap=len(want) + 7, lib=lib) == want.encode()
    long = ("@HD\tVN:1.6\tSO:unsorted\n" + "".join(f"@SQ\tSN:contig{k}\tLN:{1000 + k}\n" for k in range(3000))).encode()
    assert host.sam_sorted_header(long, lib=lib) == som.sorted_header(long)


def test_library_sorted_header_with_a_cap_that_is_too_small(lib):
    import ctypes as C
    text = b"@HD\tVN:1.6\n" + SQ.encode()
    want = som.sorted_header(text)
    for cap in (0, 1, len(text), len(want) - 1):
        out = C.create_string_buffer(b"\xAA" * (len(want) + 8))
        n = C.c_size_t(0)
        rc = lib.ngsq_sam_sorted_header(text, len(text), out, cap, C.byref(n))
        assert rc == ffi.ERR_BUFFER_TOO_SMALL and n.value == len(want), cap
        assert out.raw[:len(want) + 8] == b"\xAA" * (len(want) + 8)               # nothing was written
        with pytest.raises(host.NgsqError):
            host.sam_sorted_header(text, cap=cap, lib=lib)
    n = C.c_size_t(0)
    out = C.create_string_buffer(len(want))
    assert lib.ngsq_sam_sorted_header(text, len(text), out, len(want), C.byref(n)) == ffi.OK and out.raw == want


def test_sorted_header_on_hostile_input_under_sanitizers(tmp_path):
    """tests/c/sorted_header_drive.c: fields cut short at the end of the text, every prefix and tail of a header, bytes that are
    no text, every buffer of its exact size.  The code under test and the driver are compiled with -fsanitize=address,undefined
    into one program that runs here, on the CPU."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
    src = os.path.join(root, "ngs_amd", "csrc", "samsort_header.cpp")
    drv = os.path.join(root, "tests", "c", "sorted_header_drive.c")
    o1, o2, exe = str(tmp_path / "sh.o"), str(tmp_path / "drive.o"), str(tmp_path / "sorted_header_drive")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *san, "-c", src, "-o", o1], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", *san, "-c", drv, "-o", o2], check=True)
    subprocess.run(["g++", *san, o1, o2, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["cases", "ok", "prefixes", "ok", "hostile", "ok"]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


# ---- the command line -------------------------------------------------------------------------------------------------------
def test_help_names_the_flag(ngs):
    r = run(ngs, "convert", "--help")
    h = r.stderr + r.stdout
    assert r.returncode == 0
    for s in ("--sort <ORDER>", "[possible values: none, coordinate]", "--gzip <WHERE>", "[possible values: host, device]", "SAM to BAM",
              "-n, --num-records <USIZE>", "[default: balanced] [possible values: best, balanced, fastest]"):
        assert s in h, s


def test_sort_values_and_refusals(ngs, tmp_path):
    sam = tmp_path / "x.sam"
    sam.write_text(HEAD)
    for v in ("bogus", "", "Coordinate", "queryname"):
        for gz in ([], ["--gzip", "device"]):
            r = run(ngs, "convert", *gz, "--sort", v, str(sam), str(tmp_path / "o.bam"))
            assert r.returncode == 1 and f"Error: invalid value '{v}' for '--sort <ORDER>' [possible values: none, coordinate]" in r.stderr
    # without --gzip device the direction is not converted: today's refusal, word for word
    for args in (["--sort", "coordinate"], ["--sort", "none"], ["--sort", "coordinate", "--gzip", "host"]):
        r = run(ngs, "convert", *args, str(sam), str(tmp_path / "o.bam"))
        assert r.returncode == 1 and REFUSAL in r.stderr, args
    # refusals of the input come before any GPU work, as without the flag
    r = run(ngs, "convert", "--gzip", "device", "--sort", "coordinate", str(tmp_path / "missing.sam"), str(tmp_path / "o.bam"))
    assert r.returncode == 1 and "Error: opening SAM input file: No such file or directory (os error 2)" in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["x.sam"]


def test_with_bam_to_sam_the_flag_takes_no_part(ngs, tmp_path):
    plain = run(ngs, "convert", str(tmp_path / "x.bam"), str(tmp_path / "o.sam"))
    for v in ("coordinate", "none"):
        r = run(ngs, "convert", "--sort", v, str(tmp_path / "x.bam"), str(tmp_path / "o.sam"))
        assert (r.returncode, r.stdout, r.stderr) == (plain.returncode, plain.stdout, plain.stderr)
    assert plain.returncode == 1 and "Error: opening BAM input file: " in plain.stderr
    r = run(ngs, "convert", "--sort", "bogus", str(tmp_path / "x.bam"), str(tmp_path / "o.sam"))       # validated all the same
    assert r.returncode == 1 and "invalid value 'bogus' for '--sort <ORDER>'" in r.stderr
    assert os.listdir(tmp_path) == []
