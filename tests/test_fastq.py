"""`ngs fastq` without a GPU (include/ngsq_fastq.h): the test-side model (tests/fastq_model.py) pinned on
hand-worked records whose text is written out here as literal bytes, and the command line's surface and refusals, which all
come before any GPU work and before any output file is created."""
import os
import subprocess

import pytest

from ngs_amd import build, ffi, host
from tests import bamio
from tests import fastq_model as fm
from tests.util import batch_from_records

NAMES = ["chr1", "chr2"]
LENS = [100_000, 5_000]


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def run(ngs, *args):
    return subprocess.run([ngs, *args], capture_output=True, text=True, timeout=120)


def rec(flag, seq, qual, **kw):
    return dict(flag=flag, mapq=60, ref_id=0, pos=10, mate_ref_id=0, tlen=0, cigar=f"{len(seq)}M" if seq else "*", seq=seq, qual=qual, **kw)


def write(path, recs, names):
    bamio.write_bam(str(path), batch_from_records(recs), NAMES, LENS, with_index=False, names=names, sort_order="unsorted")
    return str(path)


def model(path, **kw):
    kw.setdefault("two_files", False)
    return fm.expected_fastq(path, **kw)


def test_complement_table_is_the_bit_reversal():
    want = dict(zip("=ACMGRSVTWYHKDBN", "=TGKCYSBAWRDMHVN"))        # A<->T C<->G M<->K R<->Y V<->B H<->D; S W N = stay
    for c in range(16):
        assert fm.SEQ_CODES[fm.COMPLEMENT[c]] == ord(want[chr(fm.SEQ_CODES[c])])


def test_forward_and_reversed_reads_of_odd_and_even_length(tmp_path):
    recs = [rec(0, "ACGTN", [0, 1, 2, 3, 93]), rec(16, "ACGTN", [0, 1, 2, 3, 93]),          # odd
            rec(0, "AACGTT"[:4] + "GA", [10, 11, 12, 13, 14, 15]), rec(16, "AACGGA", [10, 11, 12, 13, 14, 15]),   # even
            rec(16, "C", [40]), rec(16, "AC", [40, 41])]
    path = write(tmp_path / "a.bam", recs, [b"f5", b"r5", b"f6", b"r6", b"r1", b"r2"])
    one, two, other, counts = model(path)
    assert one == (b"@f5\nACGTN\n+\n!\"#$~\n"
                   b"@r5\nNACGT\n+\n~$#\"!\n"
                   b"@f6\nAACGGA\n+\n+,-./0\n"
                   b"@r6\nTCCGTT\n+\n0/.-,+\n"
                   b"@r1\nG\n+\nI\n"
                   b"@r2\nGT\n+\nJI\n")
    assert two == b"" and other == b""
    assert counts == dict(records_scanned=6, excluded=0, no_sequence=0, reads_one=0, reads_two=0, reads_other=6, dropped_other=0)


def test_every_code_complemented(tmp_path):
    codes = "=ACMGRSVTWYHKDBN"
    path = write(tmp_path / "c.bam", [rec(0, codes, None), rec(16, codes, None), rec(16, codes + "A", None)], [b"f", b"r", b"o"])
    one, _, _, _ = model(path, default_quality=40)
    assert one == (b"@f\n=ACMGRSVTWYHKDBN\n+\n" + b"I" * 16 + b"\n"
                   b"@r\nNVHMDRWABSYCKGT=\n+\n" + b"I" * 16 + b"\n"
                   b"@o\nTNVHMDRWABSYCKGT=\n+\n" + b"I" * 17 + b"\n")


def test_missing_qual_empty_name_and_no_sequence(tmp_path):
    recs = [rec(0, "ACG", None), rec(16, "ACG", None), rec(0, "TT", [5, 6]), rec(4, "", None), rec(0x104, "", None)]
    path = write(tmp_path / "m.bam", recs, [b"q", b"qr", b"", b"none", b"sec"])
    one, _, _, counts = model(path)
    assert one == b"@q\nACG\n+\n\"\"\"\n@qr\nCGT\n+\n\"\"\"\n@\nTT\n+\n&'\n"           # default quality 1 is '"'; an empty name is '@' alone
    assert (counts["records_scanned"], counts["no_sequence"], counts["excluded"], counts["reads_other"]) == (5, 1, 1, 3)
    assert model(path, default_quality=0)[0].startswith(b"@q\nACG\n+\n!!!\n")
    assert model(path, default_quality=93)[0].startswith(b"@q\nACG\n+\n~~~\n")


def test_classes_modes_and_the_suffix(tmp_path):
    flags = [0x41, 0x81, 0xC1, 0x01, 0x51, 0x141, 0x881]      # one, two, both, neither, a reversed one, a secondary one, a supplementary two
    names = [b"a", b"b", b"c", b"d", b"e", b"f", b"g"]
    path = write(tmp_path / "k.bam", [rec(f, "AC", [1, 2]) for f in flags], names)
    t = {n: b"@" + n + b"\nAC\n+\n\"#\n" for n in names}
    t[b"e"] = b"@e\nGT\n+\n#\"\n"
    one, two, other, counts = model(path)
    assert one == t[b"a"] + t[b"b"] + t[b"c"] + t[b"d"] + t[b"e"] and two == b"" and other == b""
    assert counts == dict(records_scanned=7, excluded=2, no_sequence=0, reads_one=2, reads_two=1, reads_other=2, dropped_other=0)
    one, two, other, counts = model(path, two_files=True)
    assert (one, two, other) == (t[b"a"] + t[b"e"], t[b"b"], b"") and counts["dropped_other"] == 2 and counts["reads_other"] == 2
    one, two, other, counts = model(path, two_files=True, other=True)
    assert (one, two, other) == (t[b"a"] + t[b"e"], t[b"b"], t[b"c"] + t[b"d"]) and counts["dropped_other"] == 0
    one, two, other, _ = model(path, two_files=True, other=True, suffix=True)
    assert one == b"@a/1\nAC\n+\n\"#\n@e/1\nGT\n+\n#\"\n" and two == b"@b/2\nAC\n+\n\"#\n" and other == t[b"c"] + t[b"d"]   # others get none
    assert model(path, suffix=True)[0] == b"@a/1\nAC\n+\n\"#\n@b/2\nAC\n+\n\"#\n" + t[b"c"] + t[b"d"] + b"@e/1\nGT\n+\n#\"\n"
    # the filters: everything, only the secondary and supplementary, read ones only, the first three records
    assert model(path, exclude=0)[3]["excluded"] == 0 and model(path, exclude=0)[0].count(b"@") == 7
    assert model(path, exclude=0, require=0x100)[0] == t[b"f"]
    assert model(path, require=0x40)[0] == t[b"a"] + t[b"c"] + t[b"e"]
    assert model(path, max_records=3)[0] == t[b"a"] + t[b"b"] + t[b"c"] and model(path, max_records=0)[3]["records_scanned"] == 0


def test_a_score_of_94_in_a_kept_and_in_an_excluded_record(tmp_path):
    good = rec(0, "ACGT", [1, 2, 3, 4])
    kept = write(tmp_path / "e.bam", [good, good, rec(0, "ACGT", [1, 94, 3, 4]), rec(0, "ACGT", [95, 2, 3, 4])], [b"n"] * 4)
    assert model(kept) == "writing FASTQ record: record 2: quality score above 93"
    assert model(kept, max_records=2)[0] == b"@n\nACGT\n+\n\"#$%\n" * 2
    excluded = write(tmp_path / "x.bam", [good, rec(0x100, "ACGT", [1, 94, 3, 4]), good], [b"n"] * 3)
    one, _, _, counts = model(excluded)
    assert one == b"@n\nACGT\n+\n\"#$%\n" * 2 and counts["excluded"] == 1
    assert model(excluded, exclude=0) == "writing FASTQ record: record 1: quality score above 93"
    # 0xFF behind the first byte is a score, not a missing QUAL
    late = write(tmp_path / "l.bam", [rec(0, "AC", [3, 255])], [b"n"])
    assert model(late) == "writing FASTQ record: record 0: quality score above 93"


def test_binding_and_wrapper_are_there():
    assert "ngsq_bam_write_fastq" in ffi.PROTOTYPES and hasattr(host, "bam_to_fastq")
    assert (ffi.FASTQ_EXCLUDE_FLAGS, ffi.FASTQ_DEFAULT_QUALITY, ffi.FASTQ_MAX_QUALITY) == (2304, 1, 93)


def test_struct_layouts_match_the_header(tmp_path):
    import ctypes as C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ngsq_fastq.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(ngsq_fastq_options), offsetof(ngsq_fastq_options, max_records), sizeof(ngsq_fastq_report),\n'
                   '         offsetof(ngsq_fastq_report, text_bytes), offsetof(ngsq_fastq_report, blocks), offsetof(ngsq_fastq_report, total_ms));\n'
                   '  return 0;\n}\n')
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(tmp_path / "probe")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(ffi.FastqOptions), ffi.FastqOptions.max_records.offset, C.sizeof(ffi.FastqReport), ffi.FastqReport.text_bytes.offset,
                   ffi.FastqReport.blocks.offset, ffi.FastqReport.total_ms.offset]


# ---- the command line ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_bam(tmp_path_factory):
    d = tmp_path_factory.mktemp("fq")
    return write(d / "in.bam", [rec(0x41, "ACGT", [1, 2, 3, 4]), rec(0x81, "ACGT", [1, 2, 3, 4])], [b"p", b"p"])


def refusals(bam, d):
    """(arguments, message): every refusal of the command line."""
    p = lambda name: os.path.join(d, name)
    return [
        ([], "the following required arguments were not provided: <BAM> <READ_ONES_FILE>"),
        ([bam], "the following required arguments were not provided: <READ_ONES_FILE>"),
        ([bam, p("a.fq"), p("b.fq"), p("c.fq")], f"unexpected argument '{p('c.fq')}' found"),
        ([bam, p("o.bam")], f"opening reads one file: {p('o.bam')}: incompatible formats: required FASTQ, found BAM"),
        ([bam, p("a.fastq"), p("o.sam")], f"opening reads two file: {p('o.sam')}: incompatible formats: required FASTQ, found SAM"),
        ([bam, p("a.fastq"), p("b.fastq"), "--other", p("o.fa.gz")], f"opening other reads file: {p('o.fa.gz')}: incompatible formats: required FASTQ, found Gzipped FASTA"),
        ([bam, p("a.txt")], f"opening reads one file: {p('a.txt')}: Not able to determine filetype for extension: txt"),
        ([bam, p("a.fastq"), p("a.fastq")], f"opening reads two file: {p('a.fastq')}: the same file as the read one file"),
        ([bam, p("a.fastq"), p("b.fastq"), "--other", p("b.fastq")], f"opening other reads file: {p('b.fastq')}: the same file as the read two file"),
        ([bam, p("a.fastq"), p("b.fastq"), "--other", p("a.fastq")], f"opening other reads file: {p('a.fastq')}: the same file as the read one file"),
        ([p("in.fastq"), p("in.fastq")], "opening BAM input file: " + p("in.fastq") + ": incompatible formats: required BAM, found FASTQ"),
        ([bam, p("a.fastq"), "--other", p("c.fastq")], "the argument '--other <FILE>' needs <READ_TWOS_FILE>"),
        ([bam, p("a.fastq"), "--default-quality", "94"], "invalid value '94' for '--default-quality <INT>': a quality score is at most 93"),
        ([bam, p("a.fastq"), "--default-quality", "x"], "invalid value 'x' for '--default-quality <INT>': invalid digit found in string"),
        ([bam, p("a.fastq"), "--exclude-flags", "65536"], "invalid value '65536' for '--exclude-flags <INT>': number too large to fit in target type"),
        ([bam, p("a.fastq"), "--require-flags", "65536"], "invalid value '65536' for '--require-flags <INT>': number too large to fit in target type"),
        ([bam, p("a.fastq"), "--exclude-flags", ""], "invalid value '' for '--exclude-flags <INT>': cannot parse integer from empty string"),
        ([bam, p("a.fastq"), "-n", "ten"], "invalid value 'ten' for '--num-records <USIZE>': invalid digit found in string"),
        ([bam, p("a.fastq"), "--gzip-effort", "high"], "--gzip-effort needs --gzip device"),
        ([bam, p("a.fastq"), "--gzip", "device", "--gzip-effort", "high"], "--gzip-effort needs --gzip device"),      # (no .gz output)
        ([bam, p("a.fastq.gz"), "--gzip", "host", "--gzip-effort", "high"], "--gzip-effort needs --gzip device"),
        ([bam, p("a.fastq.gz"), "--gzip", "gpu"], "invalid value 'gpu' for '--gzip <WHERE>' [possible values: host, device]"),
        ([bam, p("a.fastq"), "--pair"], "unexpected argument '--pair' found"),
        ([bam, p("a.fastq"), "--other"], "a value is required for '--other <FILE>' but none was supplied"),
        ([p("missing.bam"), p("a.fastq")], "opening BAM input file: "),
        ([p("x.sam"), p("a.fastq")], f"opening BAM input file: {p('x.sam')}: incompatible formats: required BAM, found SAM"),
    ]


def test_every_refusal_prints_its_message_and_creates_nothing(ngs, small_bam, tmp_path):
    for args, msg in refusals(small_bam, str(tmp_path)):
        before = set(os.listdir(tmp_path))
        r = run(ngs, "fastq", *args)
        assert r.returncode == 1, (args, r.stderr)
        assert "Error: " + msg in r.stderr, (args, r.stderr)
        assert set(os.listdir(tmp_path)) == before, args


def test_output_equal_to_input_is_refused(ngs, small_bam, tmp_path):
    """By another name too: a hard link to the input with a FASTQ extension."""
    link = str(tmp_path / "in.fastq")
    os.link(small_bam, link)
    size = os.path.getsize(small_bam)
    for args in ([small_bam, link], [small_bam, str(tmp_path / "a.fastq"), link], [small_bam, str(tmp_path / "a.fq"), str(tmp_path / "b.fq"), "--other", link]):
        before = set(os.listdir(tmp_path))
        r = run(ngs, "fastq", *args)
        assert r.returncode == 1 and f"{link}: the same file as the input" in r.stderr, r.stderr
        assert set(os.listdir(tmp_path)) == before and os.path.getsize(small_bam) == size
    # two outputs that are one file under two names
    a, b = str(tmp_path / "x.fastq"), str(tmp_path / "y.fastq")
    open(a, "w").close()
    os.link(a, b)
    r = run(ngs, "fastq", small_bam, a, b)
    assert r.returncode == 1 and f"Error: opening reads two file: {b}: the same file as the read one file" in r.stderr


def test_help(ngs):
    r = run(ngs, "fastq", "--help")
    assert r.returncode == 0
    h = r.stderr + r.stdout
    for s in ("Usage: ngs fastq [OPTIONS] <BAM> <READ_ONES_FILE> [<READ_TWOS_FILE>]", "--other <FILE>", "--exclude-flags <INT>", "[default: 2304]",
              "--require-flags <INT>", "-n, --num-records <USIZE>", "--name-suffix", "--default-quality <INT>", "--gzip <WHERE>", "--gzip-effort <EFFORT>",
              "--device <N>", "-t, --threads <N>", "Nothing is paired", "coordinate-sorted"):
        assert s in h, s
    assert run(ngs, "-q", "fastq", "-h").returncode == 0


def test_convert_still_refuses_the_direction(ngs, small_bam, tmp_path):
    r = run(ngs, "convert", small_bam, str(tmp_path / "o.fastq"))
    assert r.returncode == 1 and "Conversion from BAM to FASTQ is not currently supported" in r.stderr
