"""`ngs markdup` without a GPU (include/ngsq_markdup.h): the test-side model (tests/markdup_model.py)
pinned on hand-worked files whose expected flags are written out here as literals, the sweep's generator held to at least one
duplicate pair and one duplicate fragment per seed, the structures against the header, and the command line's refusals, which
all come before any GPU work and before any output file is created."""
import json
import os
import struct
import subprocess

import pytest

from ngs_amd import build, ffi, host
from tests import markdup_model as mm
from tools.fuzz_markdup import markdup_case, rec, write_bam

SWEEP_SEEDS = 24


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def run(ngs, *args):
    return subprocess.run([ngs, *args], capture_output=True, text=True, timeout=120)


def q(v, l=100):
    return bytes([v]) * l


def flags_in(stream):
    """The flags of the records of a decompressed BAM stream."""
    l_text = struct.unpack_from("<i", stream, 4)[0]
    n_ref = struct.unpack_from("<i", stream, 8 + l_text)[0]
    p = 12 + l_text
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", stream, p)[0]
    out = []
    while p < len(stream):
        out.append(struct.unpack_from("<H", stream, p + 18)[0])
        p += 4 + struct.unpack_from("<I", stream, p)[0]
    return out


def marked(tmp_path, recs, **kw):
    """(output flags, metrics) of the model on a file of these records."""
    path = write_bam(str(tmp_path / "h.bam"), recs)
    got = mm.expected_markdup(path, **kw)
    assert not isinstance(got, str), got
    return flags_in(got[0]), got[1]


def pair(name, pos1, pos2, s1, s2, f1=0x41, f2=0x91, c1="100M", c2="100M", ref2=0):
    return [rec(name, f1, 0, pos1, c1, q(s1)), rec(name, f2, ref2, pos2, c2, q(s2))]


# ---- the hand files: every expected flag is a literal ----------------------------------------------------------------------
def hand_pairs():
    """Two identical pairs, the second of the higher score, and a fragment on the pairs' forward end with the highest score of
    all; a secondary and a supplementary record of the losing pair's name; an unmapped read that came in marked."""
    return (pair(b"a", 100, 300, 20, 20) + pair(b"b", 100, 300, 30, 30) + [rec(b"f", 0, 0, 100, "100M", q(41))] +
            [rec(b"a", 0x141, 0, 100, "100M", q(30)), rec(b"a", 0x841 | 0x400, 0, 100, "100M", q(30)), rec(b"u", 0x404, -1, -1, "", q(30))])


HAND_PAIRS_FLAGS = [0x441, 0x491, 0x41, 0x91, 0x400, 0x141, 0x841, 0x4]
HAND_PAIRS_REMOVED = [0x41, 0x91, 0x141, 0x841, 0x4]
HAND_PAIRS_METRICS = dict(records=8, candidates=5, pairs=2, fragments=1, duplicate_pairs=1, duplicate_fragments=1, duplicate_records=3, cleared=2,
                          ambiguous=0, duplication=0.6)
HAND_PAIRS_JSON = ('{\n  "records": 8,\n  "candidates": 5,\n  "pairs": 2,\n  "fragments": 1,\n  "duplicate_pairs": 1,\n  "duplicate_fragments": 1,\n'
                   '  "duplicate_records": 3,\n  "cleared": 2,\n  "ambiguous": 0,\n  "name_collisions": 0,\n  "duplication": 0.600000\n}\n')


def hand_clips():
    """Fragments whose clips keep the end.  Forward end 100: 100M at 100, 5S95M at 105, 5H95M at 105, 3H2S95M at 105.  Reverse end
    199: 100M at 100, 90M10S at 100, 90M7S3H at 100; 10=5X3D20N60M at 102 (span 98); 50M5I2P48M at 102 (I and P ignored).  The
    scores rise along each group, so the last of a group survives."""
    fwd = [rec(b"f%d" % k, 0, 0, pos, c, q(20 + k, l)) for k, (pos, c, l) in enumerate(((100, "100M", 100), (105, "5S95M", 100), (105, "5H95M", 95), (105, "3H2S95M", 97)))]
    rev = [rec(b"r%d" % k, 0x10, 0, pos, c, q(20 + k, l))
           for k, (pos, c, l) in enumerate(((100, "100M", 100), (100, "90M10S", 100), (100, "90M7S3H", 97), (102, "10=5X3D20N60M", 75), (102, "50M5I2P48M", 103)))]
    return fwd + rev


HAND_CLIPS_FLAGS = [0x400, 0x400, 0x400, 0x0, 0x410, 0x410, 0x410, 0x410, 0x10]


def test_two_identical_pairs_and_what_stands_beside_them(tmp_path):
    flags, m = marked(tmp_path, hand_pairs())
    assert flags == HAND_PAIRS_FLAGS and m == HAND_PAIRS_METRICS
    assert mm.metrics_json(m) == HAND_PAIRS_JSON
    flags, m = marked(tmp_path, hand_pairs(), remove=True)
    assert flags == HAND_PAIRS_REMOVED and m == HAND_PAIRS_METRICS
    # the scores the other way round: the first pair stays
    flags, _ = marked(tmp_path, pair(b"a", 100, 300, 30, 30) + pair(b"b", 100, 300, 20, 20))
    assert flags == [0x41, 0x91, 0x441, 0x491]
    # the sum decides, not either read
    flags, _ = marked(tmp_path, pair(b"a", 100, 300, 40, 15) + pair(b"b", 100, 300, 28, 28))
    assert flags == [0x441, 0x491, 0x41, 0x91]


def test_equal_scores_the_file_order_decides(tmp_path):
    a, b = pair(b"a", 100, 300, 30, 30), pair(b"b", 100, 300, 30, 30)
    flags, _ = marked(tmp_path, [b[0], a[0], a[1], b[1]])             # b's earlier record is record 0
    assert flags == [0x41, 0x441, 0x491, 0x91]
    flags, _ = marked(tmp_path, [a[1], b[1], b[0], a[0]])             # a's earlier record is its read two, record 0
    assert flags == [0x91, 0x491, 0x441, 0x41]
    flags, _ = marked(tmp_path, [rec(b"x", 0, 0, 100, "100M", q(30)), rec(b"y", 0, 0, 100, "100M", q(30))])
    assert flags == [0x0, 0x400]


def test_fr_against_rf(tmp_path):
    """Ends 100 and 399.  A: one forward at 100, two reverse at 399.  B: one reverse at 100 (pos 1), two forward at 399: other
    tuples, no duplicates.  C: one reverse at 399, two forward at 100: A's tuples with the reads swapped, a duplicate."""
    a = pair(b"a", 100, 300, 30, 30)
    b = pair(b"b", 1, 399, 40, 40, f1=0x51, f2=0x81)
    c = pair(b"c", 300, 100, 20, 20, f1=0x51, f2=0x81)
    flags, m = marked(tmp_path, a + b + c)
    assert flags == [0x41, 0x91, 0x51, 0x81, 0x451, 0x481] and m["duplicate_pairs"] == 1


def test_clips_keep_the_end(tmp_path):
    flags, m = marked(tmp_path, hand_clips())
    assert flags == HAND_CLIPS_FLAGS and m["duplicate_fragments"] == 7 and m["fragments"] == 9
    assert mm.unclipped_end(105, False, [(3, 5), (2, 4), (95, 0)]) == 100 and mm.unclipped_end(100, True, [(90, 0), (7, 4), (3, 5)]) == 199
    assert mm.unclipped_end(102, True, [(10, 7), (5, 8), (3, 2), (20, 3), (60, 0)]) == 199
    assert mm.unclipped_end(102, True, [(50, 0), (5, 1), (2, 6), (48, 0)]) == 199
    # a clip inside the read (behind an M) is no part of the leading run
    assert mm.unclipped_end(100, False, [(10, 0), (5, 4), (10, 0)]) == 100


def test_a_cigar_of_zero_operations(tmp_path):
    recs = [rec(b"z1", 0, 0, 50, "", q(30, 10)), rec(b"z2", 0x10, 0, 50, "", q(30, 10)), rec(b"z3", 0, 0, 50, "10M", q(20, 10)),
            rec(b"z4", 0x10, 0, 41, "10M", q(40, 10))]
    flags, _ = marked(tmp_path, recs)
    assert flags == [0x0, 0x410, 0x400, 0x10]                          # ends (50, +): z1 over z3; (50, -): z4 over z2


def test_fragments_pairs_and_mates_that_are_not_there(tmp_path):
    # a pair whose mate is unmapped is a fragment: beside a fragment of the same end the better score stays
    recs = [rec(b"m", 0x49, 0, 100, "100M", q(20)), rec(b"m", 0x85, 0, 100, "", q(20)), rec(b"s", 0, 0, 100, "100M", q(30))]
    flags, m = marked(tmp_path, recs)
    assert flags == [0x449, 0x85, 0x0] and (m["pairs"], m["fragments"], m["candidates"]) == (0, 2, 2)
    # mates on two references
    flags, m = marked(tmp_path, pair(b"a", 100, 300, 20, 20, ref2=1) + pair(b"b", 100, 300, 30, 30, ref2=1) + pair(b"c", 100, 300, 40, 40))
    assert flags == [0x441, 0x491, 0x41, 0x91, 0x41, 0x91] and m["duplicate_pairs"] == 1
    # a name with two read ones: all three are fragments, and ambiguous; the read two has its end to itself
    recs = [rec(b"d", 0x41, 0, 100, "100M", q(30)), rec(b"d", 0x41, 0, 100, "100M", q(20)), rec(b"d", 0x91, 0, 300, "100M", q(20))]
    flags, m = marked(tmp_path, recs)
    assert flags == [0x41, 0x441, 0x91] and (m["pairs"], m["ambiguous"]) == (0, 3)
    # -n cuts a pair: its first record alone is a fragment, and a duplicate beside the pair member at its end
    recs = pair(b"a", 100, 300, 20, 20) + [rec(b"b", 0x41, 0, 100, "100M", q(40)), rec(b"b", 0x91, 0, 300, "100M", q(40))]
    assert marked(tmp_path, recs)[0] == [0x441, 0x491, 0x41, 0x91]
    flags, m = marked(tmp_path, recs, max_records=3)
    assert flags == [0x41, 0x91, 0x441] and (m["records"], m["pairs"], m["fragments"]) == (3, 1, 1)


def test_scores(tmp_path):
    """QUAL missing scores 0; 14 counts nothing, 15 counts."""
    recs = [rec(b"n", 0, 0, 100, "100M", None, l_seq=100), rec(b"l", 0, 0, 100, "100M", q(14)), rec(b"h", 0, 0, 100, "10M", q(15, 10))]
    flags, _ = marked(tmp_path, recs)
    assert flags == [0x400, 0x400, 0x0]                                # 0, 0 and 150: the last stays
    flags, _ = marked(tmp_path, recs[:2])
    assert flags == [0x0, 0x400]                                       # 0 and 0: the file order
    flags, _ = marked(tmp_path, [rec(b"a", 0x400, 0, 100, "100M", q(30)), rec(b"b", 0, 0, 100, "100M", q(20))])
    assert flags == [0x0, 0x400]                                       # an incoming 0x400 on the survivor is cleared


def test_an_end_outside_the_packed_range(tmp_path):
    far = [((1 << 28) - 1, "H")] * 4 + [(9, "H"), (10, "M")]             # a leading run of 2^30 + 5
    flags, _ = marked(tmp_path, [rec(b"a", 0, 0, 5, far, q(30, 10))])     # u = -2^30: the bound itself
    assert flags == [0x0]
    bad = [rec(b"a", 0, 0, 100, "10M", q(30, 10)), rec(b"b", 0x4, 0, 4, far, q(30, 10)), rec(b"c", 0, 0, 4, far, q(30, 10)),
           rec(b"d", 0, 0, 3, [((1 << 28) - 1, "H")] * 5, q(30, 10))]
    path = write_bam(str(tmp_path / "bad.bam"), bad)
    assert mm.expected_markdup(path) == "reading BAM record: record 2 (0-based): unclipped end outside what markdup can hold"
    assert not isinstance(mm.expected_markdup(path, max_records=2), str)      # the unmapped record is no candidate


def test_the_sweep_s_files_hold_duplicates_of_both_kinds(tmp_path):
    for seed in range(SWEEP_SEEDS):
        case = markdup_case(seed, str(tmp_path))
        _, m = mm.expected_markdup(case["path"], remove=case["opts"]["remove"], max_records=case["opts"]["max_records"] or None)
        assert m["duplicate_pairs"] >= 1 and m["duplicate_fragments"] >= 1 and m["ambiguous"] >= 1, (seed, m)
        os.unlink(case["path"])


# ---- the interface -------------------------------------------------------------------------------------------------------
def test_binding_and_wrapper_are_there():
    assert "ngsq_bam_mark_duplicates" in ffi.PROTOTYPES and "ngsq_markdup_bytes_per_record" in ffi.PROTOTYPES and hasattr(host, "bam_mark_duplicates")


def test_struct_layouts_match_the_header(tmp_path):
    import ctypes as C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ngsq_markdup.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ngsq_markdup_options), offsetof(ngsq_markdup_options, hash_bits),\n'
                   '         offsetof(ngsq_markdup_options, max_records), offsetof(ngsq_markdup_options, memory_budget), sizeof(ngsq_markdup_report),\n'
                   '         offsetof(ngsq_markdup_report, duplicate_records), offsetof(ngsq_markdup_report, duplication), offsetof(ngsq_markdup_report, batches),\n'
                   '         offsetof(ngsq_markdup_report, compressed_bytes), offsetof(ngsq_markdup_report, ends_ms), offsetof(ngsq_markdup_report, total_ms));\n'
                   '  return 0;\n}\n')
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(tmp_path / "probe")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split()]
    O, R = ffi.MarkdupOptions, ffi.MarkdupReport
    assert got == [C.sizeof(O), O.hash_bits.offset, O.max_records.offset, O.memory_budget.offset, C.sizeof(R), R.duplicate_records.offset,
                   R.duplication.offset, R.batches.offset, R.compressed_bytes.offset, R.ends_ms.offset, R.total_ms.offset]
    assert (C.sizeof(O), C.sizeof(R)) == (48, 232)


# ---- the command line ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_bam(tmp_path_factory):
    d = tmp_path_factory.mktemp("md")
    return write_bam(str(d / "in.bam"), hand_pairs())


def refusals(bam, d):
    p = lambda name: os.path.join(d, name)
    size = "a size is decimal digits with an optional K, M or G suffix"
    usage = "\n\nUsage: ngs markdup [OPTIONS] <BAM> <OUT_BAM>"
    return [
        ([], "the following required arguments were not provided: <BAM> <OUT_BAM>" + usage),
        ([bam], "the following required arguments were not provided: <OUT_BAM>" + usage),
        ([bam, p("o.bam"), p("x.bam")], f"unexpected argument '{p('x.bam')}' found"),
        ([p("in.sam"), p("o.bam")], f"opening BAM input file: {p('in.sam')}: incompatible formats: required BAM, found SAM"),
        ([p("in.txt"), p("o.bam")], f"failed to detect from input filetype: {p('in.txt')}: Failed parsing of bioinformatics file format."),
        ([bam, p("o.sam")], f"opening BAM output file: {p('o.sam')}: incompatible formats: required BAM, found SAM"),
        ([bam, p("o.txt")], f"failed to deteect to input filetype: {p('o.txt')}: Failed parsing of bioinformatics file format."),
        ([bam, bam], f"Conversion from BAM to BAM needs two files: {bam} is the input"),
        ([bam, p("exists.bam")], f"refusing to overwrite existing output file: {p('exists.bam')}. Please delete and rerun if you'd like to replace it."),
        ([bam, p("link.bam")], f"Conversion from BAM to BAM needs two files: {p('link.bam')} is the input"),
        ([p("none.bam"), p("o.bam")], "opening BAM input file: "),
        ([bam, p("o.bam"), "--metrics"], "a value is required for '--metrics <FILE>' but none was supplied"),
        ([bam, p("o.bam"), "--metrics", p("o.bam")], f"opening metrics file: {p('o.bam')}: the same file as the output"),
        ([bam, p("o.bam"), "--metrics", bam], f"opening metrics file: {bam}: the same file as the input"),
        ([bam, p("o.bam"), "--memory", "x"], f"invalid value 'x' for '--memory <SIZE>': {size}"),
        ([bam, p("o.bam"), "--memory", "0"], "invalid value '0' for '--memory <SIZE>': a size is at least one byte"),
        ([bam, p("o.bam"), "--gzip-effort", "max"], "invalid value 'max' for '--gzip-effort <EFFORT>' [possible values: normal, high]"),
        ([bam, p("o.bam"), "--gzip", "host"], "unexpected argument '--gzip' found"),
        ([bam, p("o.bam"), "-n", "-1"], "invalid value '-1' for '--num-records <USIZE>': invalid digit found in string"),
        ([bam, p("o.bam"), "--remove=1"], "unexpected argument '--remove=1' found"),
    ]


def test_every_refusal_prints_its_message_and_creates_nothing(ngs, small_bam, tmp_path):
    open(tmp_path / "exists.bam", "wb").write(b"kept")
    os.link(small_bam, tmp_path / "link.bam")
    for args, msg in refusals(small_bam, str(tmp_path)):
        before = set(os.listdir(tmp_path))
        r = run(ngs, "markdup", *args)
        assert r.returncode == 1, (args, r.stderr)
        assert "Error: " + msg in r.stderr, (args, r.stderr)
        assert set(os.listdir(tmp_path)) == before, args
    assert open(tmp_path / "exists.bam", "rb").read() == b"kept"


def test_help_names_the_options(ngs):
    r = run(ngs, "markdup", "--help")
    assert r.returncode == 0
    h = r.stderr + r.stdout
    for s in ("Usage: ngs markdup [OPTIONS] <BAM> <OUT_BAM>", "--remove\n", "--metrics <FILE>", "--gzip-effort <EFFORT>", "--num-records <USIZE>", "--memory <SIZE>",
              "--device <N>", "--threads <N>", "it must not exist"):
        assert s in h, s


def test_the_metrics_document_parses(tmp_path):
    doc = json.loads(HAND_PAIRS_JSON)
    assert list(doc) == list(mm.METRIC_KEYS) + ["name_collisions", "duplication"] and doc["duplication"] == 0.6
