"""`ngs depth --by <N|BED> --thresholds <T[,T...]>` without a GPU: the test-side model
(tests/depth_thresholds_model.py) on a case worked by hand, against the per-base model and on its own invariants; the command line
as far as it answers in front of the device -- the help, every refusal with and without -o, nothing written and no file left;
ngsq_bam_depth_thresholds' refusals with a context pointer that is never looked at, the empty interval list and an empty region;
and every input tests/test_depth_thresholds_gpu.py adds to those of tests/test_depth.py and tests/test_depth_by.py held, by the
model alone, to the edge it is named for.  The tests of the model -- the hand case, the per-base comparison, the invariants and
test_model_inputs_reach_their_edges -- call the model and never the new code, so they pass with or without
ngsq_bam_depth_thresholds; every other test of this file needs the new option, the new symbol or the new binding."""
import os

import numpy as np
import pytest

from ngs_amd import ffi, host
from tests import bamio
from tests import depth_model as dm
from tests import depth_thresholds_model as tm
from tests import depth_windows_model as wm
from tests import test_depth as td
from tests import test_depth_by as tb
from tests.test_depth import rec, write_case
from tests.test_depth_by import files, intervals_of, ngs, run  # noqa: F401  (files and ngs are fixtures)

MAX = 2 ** 31 - 1


# ---- the input the GPU tests add ------------------------------------------------------------------------------------------------
CARRY_L = 70_007


def case_carry():
    """One sequence of 70 007 positions under one 70000M record, plus a few short ones: whole blocks of the 1024-position granule in
    which every position counts, counts above 65 535, depths of 2 and 3 around a block boundary, and a record clipped at L."""
    T = td.tile()
    recs = [rec(0, 0, "70000M"), rec(0, 100, "50M"), rec(0, 120, "10M"), rec(0, 3 * T - 10, "20M"), rec(0, 40 * T, "%dM" % T),
            rec(0, 69_990, "10M"), rec(0, 70_003, "30M")]
    return ["k"], [CARRY_L], recs


def bed_carry():
    """Intervals on case_carry: over three tiles of 1024 with start and end in different tiles, counts above 65 535, whole blocks,
    and ends exactly on block boundaries."""
    T = td.tile()
    return [(0, 1000, 3000), (0, 5, 69_000), (0, 0, CARRY_L), (0, T, 2 * T), (0, 40 * T - 1, 41 * T + 1), (0, 2 * T, 67 * T), (0, 69_999, 70_001),
            (0, 3 * T - 10, 3 * T)]


PILES_THRESHOLDS = [1, 10, 100, 1000, 1001]


# ---- the model --------------------------------------------------------------------------------------------------------------------
def test_model_on_a_case_worked_by_hand(tmp_path):
    """The ten-position sequence of tests/test_depth.py's hand case, thresholds 1,2,3:
           position 0 1 2 3 4 5 6 7 8 9
           depth    0 0 1 2 2 1 1 0 1 1
       windows of 4: [0,4) holds 0 0 1 2: sum 3, mean 0.75; two positions reach 1, one reaches 2, none 3.
                     [4,8) holds 2 1 1 0: sum 4, mean 1.00; 3, 1, 0.      [8,10) holds 1 1: sum 2, mean 1.00; 2, 0, 0.
       b (5 positions) has no record: 0.00 and three zeros a window.
       c (8 positions, default filters): 0 1 1 0 1 0 0 0: [0,4) sum 2, 0.50; 2, 0, 0.  [4,8) sum 1, 0.25; 1, 0, 0.
       Two overlapping BED intervals on a, in the file's order: [3,9) holds 2 2 1 1 0 1: sum 7 over 6 = 1.1667 -> 1.17; 5, 2, 0.
                                                                [1,6) holds 0 1 2 2 1: sum 6 over 5 = 1.20; 4, 2, 0."""
    path = write_case(str(tmp_path / "h.bam"), ["a", "b", "c"], [10, 5, 8],
                      [rec(0, 2, "3M"), rec(0, 3, "2M1D1M"), rec(0, 8, "5M"), rec(2, 0, "8M", flag=1024), rec(2, 1, "2M"), rec(2, 7, "*"),
                       rec(2, 4, "1M", mapq=3)])
    got, info = tm.expected(path, [1, 2, 3], window=4)
    assert got == (b"a\t0\t4\t0.75\t2\t1\t0\na\t4\t8\t1.00\t3\t1\t0\na\t8\t10\t1.00\t2\t0\t0\n"
                   b"b\t0\t4\t0.00\t0\t0\t0\nb\t4\t5\t0.00\t0\t0\t0\n"
                   b"c\t0\t4\t0.50\t2\t0\t0\nc\t4\t8\t0.25\t1\t0\t0\n")
    assert info["covered"] == [10, 2, 0] and info["lines"] == 7 and info["sequences"] == 3 and info["depth_sum"] == 12
    assert info["counts"][:3] == [[2, 1, 0], [3, 1, 0], [2, 0, 0]]
    got, info = tm.expected(path, [1, 2, 3], intervals=[(0, 3, 9), (0, 1, 6)])
    assert got == b"a\t3\t9\t1.17\t5\t2\t0\na\t1\t6\t1.20\t4\t2\t0\n" and info["covered"] == [9, 4, 0] and info["sequences"] == 1
    assert tm.expected(path, [2], window=4, query="a:4-9")[0] == b"a\t3\t4\t2.00\t1\na\t4\t8\t1.00\t1\na\t8\t9\t1.00\t0\n"
    assert tm.expected(path, [1, MAX], window=MAX, exclude_flags=0)[0] == b"a\t0\t10\t0.90\t7\t0\nb\t0\t5\t0.00\t0\t0\nc\t0\t8\t1.38\t8\t0\n"
    assert tm.expected(path, [1], intervals=[])[0] == b"" and tm.expected(path, [1], window=4, query="c:9")[1]["covered"] == [0]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_against_the_per_base_model(tmp_path, seed):
    """For every T, the sum of n over --by 1's lines -- and over the lines of any other window size -- is the summed length of the
    runs of depth >= T of the per-base model (tests/depth_model.py's text)."""
    names, lens, hb = td.case_random(seed)
    path = str(tmp_path / "r.bam")
    bamio.write_bam(path, hb, names, lens, with_index=False)
    runs = [tuple(map(int, ln.split(b"\t")[1:])) for ln in dm.expected(path)[0].splitlines()]
    top = max(d for _, _, d in runs)
    thresholds = sorted({1, 2, 3, max(top - 1, 1), max(top, 1), top + 1, MAX})[:8]
    want = [sum(e - s for s, e, d in runs if d >= t) for t in thresholds]
    assert want[0] > 0 and want[-1] == 0
    for window in (1, 37, MAX):
        assert tm.expected(path, thresholds, window=window)[1]["covered"] == want


def test_model_invariants(tmp_path):
    """n_1 >= ... >= n_K, n_k <= end - start, and cutting the last K columns gives depth_windows_model's bytes."""
    names, lens, hb = td.case_random(5)
    path = str(tmp_path / "r.bam")
    bamio.write_bam(path, hb, names, lens, with_index=False)
    rng = np.random.default_rng(5)
    iv = []
    for _ in range(200):
        r = int(rng.integers(0, len(lens)))
        s = int(rng.integers(0, lens[r]))
        iv.append((r, s, int(rng.integers(s + 1, lens[r] + 1))))
    for thresholds in ([1], [1, 2, 3, 4, 5, 6, 7, 8], [2, 50, MAX]):
        for kw in (dict(window=1), dict(window=100), dict(intervals=iv)):
            text, info = tm.expected(path, thresholds, **kw)
            assert tm.first_columns(text, len(thresholds)) == wm.expected(path, **kw)[0]
            plain = wm.expected(path, **kw)[1]
            assert all(info[k] == plain[k] for k in plain)
            lines = text.splitlines()
            assert len(lines) == len(info["counts"]) == info["lines"]
            for ln, n in zip(lines, info["counts"]):
                f = ln.split(b"\t")
                assert [int(x) for x in f[4:]] == n and len(n) == len(thresholds)
                assert all(a >= b for a, b in zip(n, n[1:])) and n[0] <= int(f[2]) - int(f[1])
            assert info["covered"] == [sum(n[k] for n in info["counts"]) for k in range(len(thresholds))]


def test_model_parses_the_list():
    assert tm.parse_thresholds("1,10,20,30") == [1, 10, 20, 30] and tm.parse_thresholds("+5") == [5] and tm.parse_thresholds("2147483647") == [MAX]
    for text, why in (("", "invalid value '' for '--thresholds <T,...>': cannot parse integer from empty string"),
                      ("1,,2", "invalid value '' for '--thresholds <T,...>': cannot parse integer from empty string"),
                      ("1,x2", "invalid value 'x2' for '--thresholds <T,...>': invalid digit found in string"),
                      ("3,2147483648", "invalid value '2147483648' for '--thresholds <T,...>': number too large to fit in target type"),
                      ("0,1", "invalid value '0' for '--thresholds <T,...>': a threshold must be at least 1"),
                      ("1,2,3,4,5,6,7,8,9", "invalid value '1,2,3,4,5,6,7,8,9' for '--thresholds <T,...>': at most 8 thresholds"),
                      ("1,3,2", "invalid value '1,3,2' for '--thresholds <T,...>': thresholds must be strictly ascending")):
        with pytest.raises(tm.ThresholdsError) as e:
            tm.parse_thresholds(text)
        assert str(e.value) == why


def test_model_inputs_reach_their_edges(lib, tmp_path):
    """Calls the model alone: passes with or without the new code."""
    T = td.tile()
    assert T == 1024                                                    # the granule the counts are relative to
    # carries: whole blocks that count in full, counts above 16 bits, intervals over three tiles, ends on block boundaries
    names, lens, recs = case_carry()
    path = write_case(str(tmp_path / "k.bam"), names, lens, recs)
    d = td.depth_of(path, 0)
    assert len(d) == CARRY_L and (d[:70_000] >= 1).all() and (d[70_000:70_003] == 0).all() and (d[70_003:] == 1).all() and d.max() == 3
    assert d[3 * T - 1] == 2 and d[3 * T] == 2 and d[3 * T + 10] == 1 and d[41 * T - 1] == 2 and d[41 * T] == 1 and d[69_999] == 2
    info = tm.expected(path, [1, 2, 3], window=T)[1]
    assert info["counts"][0] == [T, 50, 10] and all(n[0] == T for n in info["counts"][:68]) and info["counts"][40] == [T, T, 0]
    assert info["counts"][68] == [70_004 - 68 * T, 10, 0] and info["covered"] == [70_004, 50 + 20 + T + 10, 10]
    assert tm.expected(path, [1, 2], window=MAX)[1]["counts"] == [[70_004, 1104]] and 70_004 > 65_535
    assert tm.expected(path, [1], window=66_000)[1]["counts"] == [[66_000], [4_004]]
    iv = bed_carry()
    counts = tm.expected(path, [1, 2, 3], intervals=iv)[1]["counts"]
    assert counts[0] == [2000, 0, 0] and iv[0][1] // T == 0 and (iv[0][2] - 1) // T == 2                  # three tiles of 1024
    assert counts[1][0] == 68_995 > 65_535 and counts[2] == [70_004, 1104, 10] and counts[3] == [T, 0, 0]
    assert counts[4] == [T + 2, T, 0] and counts[5] == [65 * T, T + 20, 0] and counts[6] == [1, 1, 0] and counts[7] == [10, 10, 0]
    assert {e % T for _, _, e in iv} >= {0, 1} and {s % T for _, s, _ in iv} >= {0, T - 1}
    # depth against T on the piles: every position where the depth is T - 1, T and T + 1, climbing and falling
    names, lens, recs = td.case_piles()
    path = write_case(str(tmp_path / "p.bam"), names, lens, recs)
    d = td.depth_of(path, 0)
    up, down = d[:int(d.argmax()) + 1], d[int(d.argmax()):]
    for t in PILES_THRESHOLDS:
        for v in (t - 1, t, t + 1):
            assert v > 1000 or ((up == v).any() and (down == v).any()), (t, v)
    info = tm.expected(path, PILES_THRESHOLDS, window=1)[1]
    assert info["covered"] == [int((d >= t).sum()) for t in PILES_THRESHOLDS] and info["covered"][3] == 1 and info["covered"][4] == 0
    assert {tuple(n) for n in info["counts"]} == {(0,) * 5, (1, 0, 0, 0, 0), (1, 1, 0, 0, 0), (1, 1, 1, 0, 0), (1, 1, 1, 1, 0)}
    # block and tile edges: window and interval ends at G - 1, G, G + 1 and at the sequence's last position, with counts that differ there
    names, lens, recs = td.case_tiles()
    path = write_case(str(tmp_path / "t.bam"), names, lens, recs)
    L = lens[0]
    d = td.depth_of(path, 0)
    assert d[T - 2] == 2 and d[T - 1] == 3 and d[T] == 4 and d[T + 1] == 1 and d[L - 1] == 3
    by1 = tm.expected(path, [1, 2, 3, 4], window=1)[1]["counts"]
    assert by1[T - 2] == [1, 1, 0, 0] and by1[T - 1] == [1, 1, 1, 0] and by1[T] == [1, 1, 1, 1] and by1[T + 1] == [1, 0, 0, 0] and by1[L - 1] == [1, 1, 1, 0]
    ends = {e for _, _, e in tb.bed_tiles()}
    assert {T - 1, T, T + 1, L, 4 * T} <= ends
    # the smallest files: the largest depth and the one above it
    names, lens, recs = td.case_small()["L1"]
    path = write_case(str(tmp_path / "s.bam"), names, lens, recs)
    assert tm.expected(path, [1, 2, 3, MAX], window=1)[0] == b"a\t0\t1\t1.00\t1\t0\t0\t0\nb\t0\t1\t2.00\t1\t1\t0\t0\nc\t0\t1\t0.00\t0\t0\t0\t0\n"
    # the 195-sequence header: uncounted sequences between counted ones give K zeros
    names, lens, recs = td.case_genome()
    path = write_case(str(tmp_path / "g.bam"), names, lens, recs)
    text = tm.expected(path, [1, 2], window=1000)[0]
    assert text.startswith(b"chr1\t0\t1000\t0.00\t0\t0\n") and b"\t0.00\t0\t0\nchr2\t" in text and text.endswith(b"\t0.00\t0\t0\n")


# ---- the command line -------------------------------------------------------------------------------------------------------------
def test_help_names_the_option(ngs):
    r = run(ngs, "depth", "--help")
    h = r.stderr.decode()
    assert r.returncode == 0 and r.stdout == b""
    for s in ("--thresholds <T,...>", "<name> <start> <end> <mean> <n_1> ... <n_K>", "strictly ascending", "--by <N|BED>", "<name> <start> <end> <mean>",
              "two decimals", "rounded half up", "Usage: ngs depth [OPTIONS] <BAM> [QUERY]"):
        assert s in h, s


def test_every_refusal_prints_its_message_and_writes_nothing(ngs, files):
    out = os.path.join(files["d"], "never_t.txt")
    f = files
    opt = "'--thresholds <T,...>'"
    cases = [
        (["--thresholds", "1,2", f["good"]], "the following required arguments were not provided: --by <N|BED>"),
        (["--by", "100", f["good"], "--thresholds"], "a value is required for '--thresholds <T,...>' but none was supplied"),
        (["--by", "100", "--thresholds", "", f["good"]], f"invalid value '' for {opt}: cannot parse integer from empty string"),
        (["--by", "100", "--thresholds", "1,,2", f["good"]], f"invalid value '' for {opt}: cannot parse integer from empty string"),
        (["--by", "100", "--thresholds", "1,2,", f["good"]], f"invalid value '' for {opt}: cannot parse integer from empty string"),
        (["--by", "100", "--thresholds", "1,x2", f["good"]], f"invalid value 'x2' for {opt}: invalid digit found in string"),
        (["--by", "100", "--thresholds", "1,+", f["good"]], f"invalid value '+' for {opt}: invalid digit found in string"),
        (["--by", "100", "--thresholds", "1, 2", f["good"]], f"invalid value ' 2' for {opt}: invalid digit found in string"),
        (["--by", "100", "--thresholds", "3,2147483648", f["good"]], f"invalid value '2147483648' for {opt}: number too large to fit in target type"),
        (["--by", f["bed"], "--thresholds", "0", f["good"]], f"invalid value '0' for {opt}: a threshold must be at least 1"),
        (["--by", "100", "--thresholds", "0,1", f["good"]], f"invalid value '0' for {opt}: a threshold must be at least 1"),
        (["--by", "100", "--thresholds", "1,2,3,4,5,6,7,8,9", f["good"]], f"invalid value '1,2,3,4,5,6,7,8,9' for {opt}: at most 8 thresholds"),
        (["--by", "100", "--thresholds", "1,3,2", f["good"]], f"invalid value '1,3,2' for {opt}: thresholds must be strictly ascending"),
        (["--by", f["bed"], "--thresholds", "2,2", f["good"]], f"invalid value '2,2' for {opt}: thresholds must be strictly ascending"),
        # given twice, the last one holds: the good list does not excuse the bad one behind it, and a bad one in front is forgotten
        (["--by", "100", "--thresholds", "1,2", "--thresholds", "2,1", f["good"]], f"invalid value '2,1' for {opt}: thresholds must be strictly ascending"),
        (["--by", "100", "--thresholds", "2,1", "--thresholds", "1,2", f["unsorted"]], "the input BAM must be coordinate-sorted to compute depth"),
        # what --by refuses, it refuses with thresholds as well
        (["--by", "0", "--thresholds", "1", f["good"]], "invalid value '0' for '--by <N|BED>': window size must be at least 1"),
        (["--by", f["bed"], "--thresholds", "1", f["good"], "q1"], "the argument '--by <BED>' cannot be used with '[QUERY]'"),
        (["--by", f["bad"], "--thresholds", "1", f["good"]], "reading BED file: line 2: start 30 is not below end 20"),
        (["--by", "100", "--thresholds", "1", f["good"], "chrX:5"], "querying BAM file: "),
    ]
    for args, msg in cases:
        for extra in ([], ["-o", out]):
            r = run(ngs, "depth", *extra, *args)
            assert r.returncode == 1, (args, r.stderr)
            assert b"Error: " in r.stderr and msg.encode() in r.stderr, (args, r.stderr)
            assert r.stdout == b"" and not os.path.exists(out), args
    # the model's parser says the same of every list above
    for args, msg in cases[2:15]:
        with pytest.raises(tm.ThresholdsError) as e:
            tm.parse_thresholds(args[args.index("--thresholds") + 1] if args.count("--thresholds") == 1 else args[5])
        assert str(e.value) == msg


# ---- the library in front of the device ---------------------------------------------------------------------------------------------
def thresholds_of(t):
    return (ffi.C.c_uint32 * max(len(t), 1))(*t)


def test_the_library_refuses_before_any_gpu_work(lib, files, tmp_path):
    C = ffi.C
    fake = C.cast(C.c_void_p(8), ffi.ctx_p)                    # never looked at: every call ends in front of the device
    out = str(tmp_path / "o")
    one = intervals_of([(0, 10, 20)])
    INV = ffi.ERR_INVALID_ARGUMENT
    ok = thresholds_of([1, 10])
    BAD = "null or invalid thresholds"
    # (path, ctx, window, intervals, n, thresholds, K, query) -> code, message
    cases = [
        (files["good"], fake, 100, None, 0, ok, 0, None, INV, BAD),
        (files["good"], fake, 100, None, 0, thresholds_of(list(range(1, 10))), 9, None, INV, BAD),
        (files["good"], fake, 100, None, 0, None, 2, None, INV, BAD),
        (files["good"], fake, 100, None, 0, thresholds_of([0, 5]), 2, None, INV, BAD),
        (files["good"], fake, 100, None, 0, thresholds_of([5, 2 ** 31]), 2, None, INV, BAD),
        (files["good"], fake, 100, None, 0, thresholds_of([5, 4]), 2, None, INV, BAD),
        (files["good"], fake, 0, one, 1, thresholds_of([5, 5]), 2, None, INV, BAD),
        (files["unsorted"], fake, 100, None, 0, thresholds_of([5, 5]), 2, None, INV, BAD),                  # before the header is looked at
        # what ngsq_bam_depth_windows refuses
        (files["good"], None, 100, None, 0, ok, 2, None, INV, "null or invalid argument"),
        (files["good"], fake, 2 ** 31, None, 0, ok, 2, None, INV, "null or invalid argument"),
        (files["good"], fake, 100, one, 1, ok, 2, None, INV, "null or invalid argument"),
        (files["good"], fake, 0, one, 1, ok, 2, b"q1", INV, "mean depth per BED interval cannot be combined with a query"),
        (files["good"], fake, 0, intervals_of([(3, 10, 20)]), 1, ok, 2, None, INV, "interval 0 is not one of the file's"),
        (files["unsorted"], fake, 100, None, 0, ok, 2, None, ffi.ERR_UNSORTED, dm.NOT_SORTED),
        (files["unsorted"], fake, 0, None, 0, ok, 2, None, ffi.ERR_UNSORTED, dm.NOT_SORTED),
        (files["good"], fake, 100, None, 0, ok, 2, b"nope", INV, "querying BAM file: "),
    ]
    for path, ctx, window, iv, n, thr, K, query, code, msg in cases:
        bam = C.c_void_p()
        assert lib.ngsq_bam_open(path.encode(), 0, C.byref(bam)) == 0
        try:
            fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
            rc = lib.ngsq_bam_depth_thresholds(bam, ctx, fd, window, iv, n, thr, K, query, None, 1796, 0, 0, 0, 0, 0, None)
            os.close(fd)
            assert rc == code, (window, n, K, query, rc)
            assert msg in lib.ngsq_bam_last_error().decode(), (msg, lib.ngsq_bam_last_error())
            assert os.path.getsize(out) == 0
        finally:
            lib.ngsq_bam_close(bam)
    assert not tm.valid([]) and not tm.valid(list(range(1, 10))) and not tm.valid(None) and not tm.valid([0, 5]) and not tm.valid([5, 2 ** 31])
    assert not tm.valid([5, 4]) and not tm.valid([5, 5]) and tm.valid([1, 10]) and tm.valid([MAX])


def test_no_interval_and_an_empty_region_need_no_gpu(lib, files, tmp_path):
    """The empty interval list and a region behind its sequence's end: OK, nothing written, every count 0, covered included."""
    C = ffi.C
    fake = C.cast(C.c_void_p(8), ffi.ctx_p)
    out = str(tmp_path / "o")
    thr = thresholds_of([1, 2, 3])
    for window, query in ((0, None), (0, b"q1"), (0, b"nope"), (100, b"q3:5001"), (MAX, b"q1:300001")):
        bam = C.c_void_p()
        assert lib.ngsq_bam_open(files["good"].encode(), 0, C.byref(bam)) == 0
        try:
            fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
            rep = ffi.DepthThresholdsReport()
            rep.lines = rep.records_scanned = 77
            for k in range(8):
                rep.covered[k] = 77
            assert lib.ngsq_bam_depth_thresholds(bam, fake, fd, window, None, 0, thr, 3, query, None, 1796, 0, 0, 0, 0, 0, C.byref(rep)) == 0
            os.close(fd)
            assert os.path.getsize(out) == 0
            for k in ("records_scanned", "records_counted", "lines", "text_bytes", "sequences", "depth_sum", "tiles", "passes", "batches", "ranges"):
                assert getattr(rep, k) == 0, k
            assert list(rep.covered) == [0] * 8
        finally:
            lib.ngsq_bam_close(bam)
    assert tm.expected(files["good"], [1, 2, 3], intervals=[])[1]["covered"] == [0, 0, 0]
    assert tm.expected(files["good"], [1, 2, 3], window=100, query="q3:5001")[0] == b""


def test_the_bindings_declare_the_call(lib):
    assert "ngsq_bam_depth_thresholds" in ffi.PROTOTYPES and ffi.DEPTH_MAX_THRESHOLDS == 8 == tm.MAX_THRESHOLDS
    fields = [k for k, _ in ffi.DepthThresholdsReport._fields_]
    assert fields[:-1] == [k for k, _ in ffi.DepthWindowsReport._fields_] and fields[-1] == "covered"
    assert ffi.C.sizeof(ffi.DepthThresholdsReport) == ffi.C.sizeof(ffi.DepthWindowsReport) + 64
    assert ffi.DepthThresholdsReport.covered.offset == ffi.C.sizeof(ffi.DepthWindowsReport)
    import inspect
    assert inspect.signature(host.bam_depth_windows).parameters["thresholds"].default is None
