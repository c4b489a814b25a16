"""`ngs view <BAM> [QUERY]` without a GPU: the test-side model (tests/view_model.py) pinned on the
hand-assembled files against lines worked out by hand, the region grammar, the library's chunk query against the model's on
files of several hundred blocks, the command line's refusals and its header-only mode (which needs no GPU), and the host side
of the query under the sanitizers, driven by a stand-alone C program."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from ngs_amd import build, ffi, host
from tests import bai_model as bm
from tests import bamio
from tests import view_model as vm
from tests.test_index import LENS, NAMES, index_sorted_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def run(ngs, *args):
    return subprocess.run([ngs, *args], capture_output=True, timeout=120)


def indexed_copy(name, d):
    """A hand file beside the index `ngs index` gives it (bai_model): the committed .bai of the hand files holds no bins."""
    path = os.path.join(str(d), name)
    shutil.copy(os.path.join(GOLDEN, name), path)
    with open(path + ".bai", "wb") as f:
        f.write(bm.expected_bai(path))
    return path


def write_indexed(path, hb, **kw):
    """hb (coordinate order) as a BAM file with the model's index beside it."""
    kw.setdefault("with_index", False)
    bamio.write_bam(path, hb, NAMES, LENS, **kw)
    with open(path + ".bai", "wb") as f:
        f.write(bm.expected_bai(path))
    return path


# ---- the model on the hand files ----------------------------------------------------------------------------------------
# hand_spec.sam, by hand: r1 chr1 100..149, r2 301..330 (20S30M), r3 321..458 (10M2I5M3D10M100N5M1X4=: 10+5+3+10+100+5+1+4),
# r4 5001..5040 (5H40M5H), r5 5011..5050, r6 99991..100000, r7 chr2 11..130, r8 unplaced
HAND_REGIONS = [
    ("chr1", ["r1/all_tags", "r2", "r3", "r4", "r5", "r6/straddles"]),
    ("chr2", ["r7"]),
    ("chr1:149-300", ["r1/all_tags"]),                  # r1's last base; r2 starts one behind the interval
    ("chr1:150-300", []),
    ("chr1:150-301", ["r2"]),
    ("chr1:331-331", ["r3"]),                           # one behind r2's end
    ("chr1:440-458", ["r3"]),                           # reached by r3's N and what follows it
    ("chr1:459-5000", []),
    ("chr1:459-5001", ["r4"]),
    ("chr1:5041", ["r5", "r6/straddles"]),              # an open interval
    ("chr1:100000-100000", ["r6/straddles"]),
    ("chr1:100001", []),                                # past the sequence's end
    ("chr2:1-10", []),
    ("chr2:130-200", ["r7"]),
    ("chr2:131", []),
]


@pytest.mark.parametrize("query,want", HAND_REGIONS)
def test_model_on_hand_spec(tmp_path, query, want):
    path = indexed_copy("hand_spec.bam", tmp_path)
    lines = open(os.path.join(GOLDEN, "hand_spec.sam"), "rb").read().split(b"\n")
    by_name = {ln.split(b"\t")[0].decode(): ln + b"\n" for ln in lines if ln and not ln.startswith(b"@")}
    head = b"".join(ln + b"\n" for ln in lines if ln.startswith(b"@"))
    body = b"".join(by_name[n] for n in want)
    assert vm.expected_view(path, query, "records-only") == body
    assert vm.expected_view(path, query, "full") == head + body
    assert vm.expected_view(path, query, "header-only") == head


def test_model_without_a_query_is_the_whole_file():
    path = os.path.join(GOLDEN, "hand_spec.bam")
    assert vm.expected_view(path) == open(os.path.join(GOLDEN, "hand_spec.sam"), "rb").read()
    assert vm.expected_view(path, None, "records-only").count(b"\n") == 8


def test_model_with_the_committed_index_without_bins_selects_nothing():
    """tests/golden/hand_spec.bam.bai holds no bins: no chunk, no record -- the index decides, not the file."""
    path = os.path.join(GOLDEN, "hand_spec.bam")
    assert vm.expected_view(path, "chr1", "records-only") == b""
    assert vm.expected_view(path, "chr1:100-200", "full") == vm.header_bytes(path)


def test_model_selects_the_long_cigar_record_by_its_resolved_span(tmp_path):
    """hand_longcigar.bam: pos 1000 (0-based), CIGAR field 30S35N, CG tag 10M5D20M: 1001..1035 either way, and the line shows the
    resolved CIGAR."""
    path = indexed_copy("hand_longcigar.bam", tmp_path)
    got = vm.expected_view(path, "chr1:1035-2000", "records-only")
    assert got.count(b"\n") == 1 and got.split(b"\t")[5] == b"10M5D20M"
    assert vm.expected_view(path, "chr1:1036-2000", "records-only") == b""
    assert vm.expected_view(path, "chr1:1-1000", "records-only") == b""
    assert vm.expected_view(path, "chr1:1-1001", "records-only") == got


GRAMMAR = [
    ("chr1", (0, 1, vm.END_MAX)),
    ("chr1:5", (0, 5, vm.END_MAX)),
    ("chr1:5-9", (0, 5, 9)),
    ("chr1:0", "querying BAM file"),                 # 0 is no start: the name is "chr1:0"
    ("chr1:9-5", "querying BAM file"),
    ("HLA-A*01:01", (2, 1, vm.END_MAX)),             # "01" reads as a start: the name is HLA-A*01
    ("HLA-A*01:01:5-9", (1, 5, 9)),
    ("", "parsing query"),
]
GRAMMAR_NAMES = ["chr1", "HLA-A*01:01", "HLA-A*01"]


@pytest.mark.parametrize("query,want", GRAMMAR)
def test_grammar_model(query, want):
    if isinstance(want, str):
        with pytest.raises(vm.ViewError) as e:
            vm.parse_query(query, GRAMMAR_NAMES)
        assert e.value.context == want
    else:
        assert vm.parse_query(query, GRAMMAR_NAMES) == want


@pytest.fixture(scope="module")
def grammar_bam(tmp_path_factory):
    d = tmp_path_factory.mktemp("g")
    hb = index_sorted_batch(3, 40, lens=[5000, 5000, 5000], weird=False)
    path = str(d / "g.bam")
    bamio.write_bam(path, hb, GRAMMAR_NAMES, [5000, 5000, 5000], with_index=False)
    with open(path + ".bai", "wb") as f:
        f.write(bm.expected_bai(path))
    return path


@pytest.mark.parametrize("query,want", GRAMMAR)
def test_grammar_library(lib, grammar_bam, query, want):
    if isinstance(want, str):
        with pytest.raises(host.NgsqError) as e:
            host.bam_query_chunks(grammar_bam, query, lib=lib)
        assert want + ": " in str(e.value)
    else:
        assert host.bam_query_chunks(grammar_bam, query, lib=lib)[:3] == want


def test_reg2bins_holds_reg2bin():
    rng = np.random.default_rng(5)
    for _ in range(2000):
        beg = int(rng.integers(0, 1 << 29))
        end = min(1 << 29, beg + 1 + int(rng.choice([0, 1, 100, 16383, 16384, 1 << 17, 1 << 26])))
        bins = vm.reg2bins(beg, end)
        assert len(set(bins)) == len(bins) and bm.META_BIN not in bins
        for _ in range(4):                                              # every record overlapping it lies in one of them
            b0 = int(rng.integers(max(0, beg - 70000), end))
            e0 = max(b0 + 1, min(1 << 29, int(rng.integers(beg + 1, end + 70000))))
            assert bm.reg2bin(b0, e0) in bins


# ---- the library's chunk query against the model's ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many_blocks(tmp_path_factory):
    d = tmp_path_factory.mktemp("q")
    hb = index_sorted_batch(31, 12000, max_len=200)
    path = write_indexed(str(d / "q.bam"), hb, block_payload=5000)
    assert len(bm.read_blocks(path)[0]) > 300
    return path


def region_queries(rng, n):
    out = ["chr1", "chr2", "chr3", "chr1:1-1", "chr1:16384-16385", "chr1:16385-16385", "chr1:300000", "chr1:300001", "chr3:4999-9000",
           "chr1:299000-100000000", "chr2:1-536870912", "chr2:536870912", "chr2:536870913"]
    for _ in range(n):
        r = int(rng.integers(0, 3))
        s = int(rng.integers(1, LENS[r] + 500))
        e = s + int(rng.choice([0, 1, 50, 2000, 16384, 100000]))
        out.append(f"{NAMES[r]}:{s}-{e}" if rng.random() < 0.8 else f"{NAMES[r]}:{s}")
    return out


def test_library_chunks_equal_the_models(lib, many_blocks):
    bai = open(many_blocks + ".bai", "rb").read()
    seen = 0
    for q in region_queries(np.random.default_rng(32), 150):
        ref, s, e = vm.parse_query(q, NAMES)
        want = vm.query_chunks(bai, ref, s, e)
        got = host.bam_query_chunks(many_blocks, q, lib=lib)
        assert got[:3] == (ref, s, e), q
        assert got[3] == want, q
        seen += len(want) > 1
    assert seen > 10                                                     # (queries of several merged chunks are among them)


def test_library_chunks_other_index_path_and_errors(lib, many_blocks, tmp_path):
    other = str(tmp_path / "elsewhere.bai")
    shutil.copy(many_blocks + ".bai", other)
    assert host.bam_query_chunks(many_blocks, "chr2:100-900", bai_path=other, lib=lib) == host.bam_query_chunks(many_blocks, "chr2:100-900", lib=lib)
    bai = open(other, "rb").read()
    for bad in (bai[:len(bai) // 2], b"BAI\2" + bai[4:], bai + b"xx", b""):
        open(other, "wb").write(bad)
        with pytest.raises(host.NgsqError, match="reading BAM index: "):
            host.bam_query_chunks(many_blocks, "chr1", bai_path=other, lib=lib)
    with pytest.raises(host.NgsqError, match="reading BAM index: "):
        host.bam_query_chunks(many_blocks, "chr1", bai_path=str(tmp_path / "missing.bai"), lib=lib)
    with pytest.raises(host.NgsqError, match="querying BAM file: "):
        host.bam_query_chunks(many_blocks, "chrX:5", lib=lib)
    with pytest.raises(host.NgsqError, match="parsing query: "):
        host.bam_query_chunks(many_blocks, "", lib=lib)


# ---- the command line -------------------------------------------------------------------------------------------------------
NOT_HERE = " files are viewed by the reference `ngs view` but not by this build, which views BAM files only"
NOT_AT_ALL = (" files are not supported by this command. This may be because we haven't supported this file format yet or because "
              "it does not make sense to view a file of this kind. If you believe this format should be supported, please search "
              "for and upvote the related issue on Github (or file a new one).")


def refusals(d):
    return [
        (["x.sam"], "SAM" + NOT_HERE),
        (["x.cram"], "--reference-fasta is a required argument when converting to/from a CRAM file"),
        (["-r", "ref.fa", "x.cram"], "CRAM" + NOT_HERE),
        (["x.gff"], "GFF" + NOT_HERE),
        (["x.gff3"], "GFF" + NOT_HERE),
        (["x.gff.gz"], "Gzipped GFF" + NOT_HERE),
        (["x.gtf"], "GTF" + NOT_HERE),
        (["x.gtf.gz"], "Gzipped GTF" + NOT_HERE),
        (["x.fastq"], "FASTQ" + NOT_AT_ALL),
        (["x.fa.gz"], "Gzipped FASTA" + NOT_AT_ALL),
        (["x.vcf"], "VCF" + NOT_AT_ALL),
        (["x.bed"], "BED" + NOT_AT_ALL),
        (["x.gff.bgz"], "Block-gzipped GFF" + NOT_AT_ALL),
        (["x.ubam"], "Unaligned BAM" + NOT_AT_ALL),
        (["x.unknown"], "Not able to determine bioinformatics file type for path: x.unknown"),
        (["noextension"], "Not able to determine bioinformatics file type for path: noextension"),
        ([os.path.join(d, "missing.bam")], "opening BAM input file: "),
        ([os.path.join(d, "missing.bam"), "chr1"], "opening BAM input file: "),
        ([], "the following required arguments were not provided: <FILE>"),
        (["a.bam", "chr1", "more"], "unexpected argument 'more' found"),
        (["-m", "both", "a.bam"], "invalid value 'both' for '--mode <MODE>' [possible values: full, header-only, records-only]"),
        (["a.bam", "--mode"], "a value is required for '--mode <MODE>' but none was supplied"),
        (["--nope", "a.bam"], "unexpected argument '--nope' found"),
    ]


def test_every_refusal_prints_its_message_and_writes_nothing(ngs, tmp_path):
    for args, msg in refusals(str(tmp_path)):
        r = run(ngs, "view", *args)
        assert r.returncode == 1, (args, r.stderr)
        assert ("Error: " + msg).encode() in r.stderr, (args, r.stderr)
        assert r.stdout == b"", args


def test_help_shows_the_reference_surface(ngs):
    r = run(ngs, "view", "--help")
    assert r.returncode == 0
    h = (r.stderr + r.stdout).decode()
    for s in ("<FILE>", "[QUERY]", "-r, --reference-fasta <REFERENCE_FASTA>", "-m, --mode <MODE>", "[default: full]",
              "full, header-only, records-only", "--device <N>"):
        assert s in h, s
    r = run(ngs, "nosuchcommand")
    assert r.returncode == 1 and b"`view`" in r.stderr


@pytest.mark.parametrize("name", ["hand_spec.bam", "hand_longcigar.bam"])
def test_header_only_byte_for_byte_without_a_gpu(ngs, lib, tmp_path, name):
    path = os.path.join(GOLDEN, name)
    want = vm.expected_view(path, None, "header-only")
    assert want.startswith(b"@HD\t") and want == vm.header_bytes(path)
    for args in (["-m", "header-only", path], ["--mode", "header-only", path, "chr1:5-9"], ["-q", "-m", "header-only", path, "not a region"]):
        r = run(ngs, "view", *args)                       # (view/bam.rs:39-42: the query is never looked at)
        assert r.returncode == 0, r.stderr
        assert r.stdout == want
    out = str(tmp_path / "h.txt")
    rep = host.bam_view(path, out, mode="header-only", lib=lib)
    assert open(out, "rb").read() == want and rep["header_bytes"] == len(want) and rep["records_written"] == 0


def test_header_without_a_final_newline_gets_none(ngs, lib, tmp_path):
    """The header text exactly as the file holds it: `ngs convert` adds the newline a text lacks, `ngs view` does not."""
    import struct
    text = b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:100"
    head = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", 100)
    path = str(tmp_path / "n.bam")
    open(path, "wb").write(bamio.bgzf_block(head) + bamio.EOF_BLOCK)
    assert vm.expected_view(path, None, "header-only") == text
    r = run(ngs, "view", "-m", "header-only", path)
    assert r.returncode == 0 and r.stdout == text


def test_records_need_the_device_before_the_first_byte(ngs, lib, tmp_path):
    """full and records-only acquire the device before anything is written: on a box without one, exit 1 and an empty stdout
    (with one, the view itself)."""
    path = indexed_copy("hand_spec.bam", tmp_path)
    gpu = lib.ngsq_device_count() > 0
    for mode, query in (("full", None), ("records-only", None), ("full", "chr1:100-200")):
        r = run(ngs, "view", "-m", mode, path, *([query] if query else []))
        if gpu:
            assert r.returncode == 0 and r.stdout == vm.expected_view(path, query, mode), (mode, query, r.stderr)
        else:
            assert r.returncode == 1 and r.stdout == b"" and b"Error: " in r.stderr, (mode, query)


def test_library_refuses_bad_arguments(lib, tmp_path):
    bam = ffi.C.c_void_p()
    path = os.path.join(GOLDEN, "hand_spec.bam")
    assert lib.ngsq_bam_open(path.encode(), 1, ffi.C.byref(bam)) == 0
    try:
        fd = os.open(str(tmp_path / "o"), os.O_WRONLY | os.O_CREAT, 0o666)
        assert lib.ngsq_bam_view(bam, None, fd, None, None, ffi.VIEW_FULL, 0, 0, None) != 0          # records without a context
        assert lib.ngsq_bam_view(bam, None, fd, None, None, 3, 0, 0, None) != 0                      # no such mode
        assert lib.ngsq_bam_view(bam, None, -1, None, None, ffi.VIEW_HEADER_ONLY, 0, 0, None) != 0
        assert lib.ngsq_bam_view(bam, None, fd, None, None, ffi.VIEW_HEADER_ONLY, 0, 0, None) == 0
        os.close(fd)
        fd = os.open("/dev/full", os.O_WRONLY)
        assert lib.ngsq_bam_view(bam, None, fd, None, None, ffi.VIEW_HEADER_ONLY, 0, 0, None) != 0
        assert lib.ngsq_bam_last_error().decode().startswith("writing BAM header to stream: No space left on device (os error 28)")
        os.close(fd)
    finally:
        lib.ngsq_bam_close(bam)


# ---- the host side of the query under the sanitizers ----------------------------------------------------------------------
def test_query_parser_and_chunk_query_on_hostile_input_under_sanitizers(tmp_path):
    """tests/c/view_query_drive.c: the grammar table, a truncated BAI at every length, bins with zero chunks, a linear index
    shorter than the window, counts that lie, random bytes.  The code under test and the driver are compiled with
    -fsanitize=address,undefined into one program that runs here, on the CPU."""
    src = os.path.join(ROOT, "ngs_amd", "csrc", "view_query.cpp")
    drv = os.path.join(ROOT, "tests", "c", "view_query_drive.c")
    o1, o2, exe = str(tmp_path / "vq.o"), str(tmp_path / "drive.o"), str(tmp_path / "view_query_drive")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-c", src, "-o", o1], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", *SAN, "-c", drv, "-o", o2], check=True)
    subprocess.run(["g++", *SAN, o1, o2, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["grammar", "ok", "index", "ok", "hostile", "ok"]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
