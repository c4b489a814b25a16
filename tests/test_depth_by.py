"""`ngs depth --by <N|BED>` without a GPU: the command line as far as it answers in front of the device --
the help, every refusal with and without -o, nothing written and no file left; ngsq_bam_depth_windows' refusals with a context
pointer that is never looked at, the empty interval list and an empty region; and every input tests/test_depth_by_gpu.py adds to
those of tests/test_depth.py held, by the model alone, to the edge it is named for.  That last test, test_model_inputs_reach_their_edges,
calls the model and never the new code, so it alone of this file passes with or without ngsq_bam_depth_windows."""
import os
import subprocess

import pytest

from ngs_amd import build, ffi, host
from tests import bamio
from tests import depth_model as dm
from tests import depth_windows_model as wm
from tests import test_depth as td
from tests.test_depth import rec, write_case
from tests.util import batch_from_records

MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def run(ngs, *args):
    return subprocess.run([ngs, *args], capture_output=True, timeout=120)


# ---- the inputs the GPU tests add: name -> (names, lens, records) ---------------------------------------------------------------
def case_wide():
    """3000 records 1M1999998N1M at position 0 of a sequence of 2 000 100: depth 3000 over two million positions, a sum of
    6 000 000 000, above 2^32."""
    return ["g"], [2_000_100], [rec(0, 0, "1M1999998N1M") for _ in range(3000)]


def case_rounding():
    """199/200 carries into 1.00, 1/200 rounds up to 0.01, and a last window of one position."""
    return ["a", "b", "c"], [200, 200, 201], [rec(0, 0, "199M"), rec(1, 5, "1M"), rec(2, 7, "1M")]


PASS_WINDOWS = [255, 256, 257, 513]


def case_passes():
    """Sequences of exactly 255, 256, 257 and 513 windows of 3 positions (the last window short), a record in each."""
    lens = [3 * w - 1 for w in PASS_WINDOWS]
    return ["w%d" % w for w in PASS_WINDOWS], lens, [rec(r, L - 4, "10M") for r, L in enumerate(lens)] + [rec(3, 700, "5M")]


def passes_of(line_counts, lines_per_pass=256):
    """Format passes of a call whose line sources have these many lines."""
    return sum(-(-n // lines_per_pass) for n in line_counts if n)


def tile_windows():
    """The window sizes the tile tests take case_tiles through."""
    T = td.tile()
    L = 5 * T + 7
    return [1, 2, 3, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 5, L - 1, L, L + 1, MAX]


def bed_tiles():
    """Intervals on case_tiles: a start and an end at each of T - 1, T, T + 1, 0 and L, one over three tiles, one of a single
    position; then overlapping, nested, repeated and descending ones."""
    T = td.tile()
    L = 5 * T + 7
    iv = [(0, T - 1, T + 5), (0, T, T + 5), (0, T + 1, T + 5), (0, 0, 9), (0, 5, T - 1), (0, 5, T), (0, 5, T + 1), (0, L - 3, L), (0, 0, L),
          (0, T - 5, 3 * T + 5), (0, T, T + 1), (0, 2 * T - 1, 2 * T)]
    iv += [(0, 100, 300), (0, 200, 400), (0, 220, 230), (0, 220, 230), (0, 4 * T, L), (0, 3 * T, 4 * T), (0, 50, 60), (0, 0, 1)]
    return iv


def test_model_inputs_reach_their_edges(lib, tmp_path):
    T = td.tile()
    # a window boundary at T - 1, T and T + 1, and windows over several tiles, on case_tiles
    names, lens, recs = td.case_tiles()
    L = lens[0]
    assert L == 5 * T + 7
    ends = {n: {e for _, e in wm.windows(0, L, n)} for n in tile_windows()}
    assert T - 1 in ends[T - 1] and T in ends[T] and T + 1 in ends[T + 1] and T in ends[1] and T - 1 in ends[1] and T + 1 in ends[1]
    assert ends[2 * T + 5] == {2 * T + 5, 4 * T + 10, L} and ends[L] == {L} == ends[L + 1] == ends[MAX] and ends[L - 1] == {L - 1, L}
    iv = bed_tiles()
    assert {s for _, s, _ in iv} >= {0, T - 1, T, T + 1} and {e for _, _, e in iv} >= {T - 1, T, T + 1, L}
    assert any(e - s > 2 * T for _, s, e in iv) and any(e - s == 1 for _, s, e in iv)
    assert any(a[1] > b[1] for a, b in zip(iv, iv[1:])) and any(a == b for a, b in zip(iv, iv[1:]))
    path = write_case(str(tmp_path / "t.bam"), names, lens, recs)
    text, info = wm.expected(path, intervals=iv)
    assert info["lines"] == len(iv) and [tuple(map(int, ln.split(b"\t")[1:3])) for ln in text.splitlines()] == [(s, e) for _, s, e in iv]
    # a line of x.995 that carries, 0.005 that rounds up, a last window of one position
    names, lens, recs = case_rounding()
    path = write_case(str(tmp_path / "r.bam"), names, lens, recs)
    assert wm.expected(path, window=200)[0] == b"a\t0\t200\t1.00\nb\t0\t200\t0.01\nc\t0\t200\t0.01\nc\t200\t201\t0.00\n"
    # a sum above 2^32
    names, lens, recs = case_wide()
    path = write_case(str(tmp_path / "g.bam"), names, lens, recs)
    assert os.path.getsize(path) < 20_000
    text, info = wm.expected(path, window=MAX)
    assert text == b"g\t0\t2000100\t2999.85\n" and info["depth_sum"] == 6_000_000_000 > 2 ** 32
    for n, lines in ((65536, 31), (1000, 2001)):
        info = wm.expected(path, window=n)[1]
        assert info["lines"] == lines and info["depth_sum"] == 6_000_000_000
    assert 21 * 65536 * 3000 < 2 ** 32 < 22 * 65536 * 3000                  # P crosses 2^32 in the 22nd tile of 65536: the carry holds it from there
    # lines against passes
    names, lens, recs = case_passes()
    path = write_case(str(tmp_path / "p.bam"), names, lens, recs)
    assert [len(wm.windows(0, x, 3)) for x in lens] == PASS_WINDOWS and wm.expected(path, window=3)[1]["lines"] == sum(PASS_WINDOWS)
    assert passes_of(PASS_WINDOWS) == 1 + 1 + 2 + 3
    # piles: means through 9.99 -> 10.00, 99 -> 100, 999 -> 1000
    names, lens, recs = td.case_piles()
    path = write_case(str(tmp_path / "piles.bam"), names, lens, recs)
    means = {ln.split(b"\t")[3] for n in (1, 7) for ln in wm.expected(path, window=n)[0].splitlines()}
    assert {b"9.00", b"10.00", b"99.00", b"100.00", b"999.00", b"1000.00"} <= means
    assert any(len(m) == 4 for m in means) and any(len(m) == 5 for m in means) and any(len(m) == 6 for m in means) and any(len(m) == 7 for m in means)
    # powers of ten in the coordinates
    names, lens, recs = td.case_pow10()
    text = wm.expected(write_case(str(tmp_path / "w.bam"), names, lens, recs), window=10)[0]
    starts = {int(ln.split(b"\t")[1]) for ln in text.splitlines()}
    assert all(10 ** k in starts for k in range(1, 6))
    # batches in BED mode: records on sequences without an interval are still counted
    names, lens, recs = td.case_batches()
    path = write_case(str(tmp_path / "b.bam"), names, lens, recs)
    iv = [(0, 10, 500), (3, 0, 50), (5, 100, 11000)]
    info = wm.expected(path, intervals=iv)[1]
    assert info["records_counted"] == dm.expected(path)[1]["records_counted"] and info["sequences"] == 3
    assert {r["ref_id"] for r in recs} >= {1, 2, 4} and 3 not in {r["ref_id"] for r in recs}


# ---- the command line -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("by")
    names, lens, recs = td.case_query()
    good = write_case(str(d / "good.bam"), names, lens, recs[:50])
    unsorted = str(d / "unsorted.bam")
    bamio.write_bam(unsorted, batch_from_records(recs[:5]), names, lens, with_index=False, sort_order="unsorted")
    bed = str(d / "ok.bed")
    with open(bed, "wb") as f:
        f.write(b"q1\t10\t20\nq3\t5\t50\n")
    bad = str(d / "bad.bed")
    with open(bad, "wb") as f:
        f.write(b"q1\t10\t20\nq1\t30\t20\n")
    return dict(d=str(d), good=good, unsorted=unsorted, bed=bed, bad=bad)


def test_help_names_the_option(ngs):
    r = run(ngs, "depth", "--help")
    h = r.stderr.decode()
    assert r.returncode == 0 and r.stdout == b""
    for s in ("--by <N|BED>", "<name> <start> <end> <mean>", "two decimals", "rounded half up", "Usage: ngs depth [OPTIONS] <BAM> [QUERY]"):
        assert s in h, s


def test_every_refusal_prints_its_message_and_writes_nothing(ngs, files):
    out = os.path.join(files["d"], "never.txt")
    f = files
    cases = [
        ([f["good"], "--by"], "a value is required for '--by <N|BED>' but none was supplied"),
        (["--by", "0", f["good"]], "invalid value '0' for '--by <N|BED>': window size must be at least 1"),
        (["--by", "+0", f["good"]], "invalid value '+0' for '--by <N|BED>': window size must be at least 1"),
        (["--by", "2147483648", f["good"]], "invalid value '2147483648' for '--by <N|BED>': number too large to fit in target type"),
        (["--by", "+2147483648", f["good"]], "invalid value '+2147483648' for '--by <N|BED>': number too large to fit in target type"),
        (["--by", os.path.join(f["d"], "missing.bed"), f["good"]], "opening BED file: "),
        (["--by", f["bad"], f["good"]], "reading BED file: line 2: start 30 is not below end 20"),
        (["--by", f["bed"], f["good"], "q1"], "the argument '--by <BED>' cannot be used with '[QUERY]'"),
        (["--by", "100", f["unsorted"]], "the input BAM must be coordinate-sorted to compute depth"),
        (["--by", f["bed"], f["unsorted"]], "the input BAM must be coordinate-sorted to compute depth"),
        (["--by", "100", f["good"], "chrX:5"], "querying BAM file: "),
    ]
    for args, msg in cases:
        for extra in ([], ["-o", out]):
            r = run(ngs, "depth", *extra, *args)
            assert r.returncode == 1, (args, r.stderr)
            assert b"Error: " in r.stderr and msg.encode() in r.stderr, (args, r.stderr)
            assert r.stdout == b"" and not os.path.exists(out), args


# ---- the library in front of the device ---------------------------------------------------------------------------------------------
def intervals_of(iv):
    return (ffi.DepthInterval * max(len(iv), 1))(*[ffi.DepthInterval(*v) for v in iv])


def test_the_library_refuses_before_any_gpu_work(lib, files, tmp_path):
    C = ffi.C
    fake = C.cast(C.c_void_p(8), ffi.ctx_p)                    # never looked at: every call ends in front of the device
    out = str(tmp_path / "o")
    one = intervals_of([(0, 10, 20)])
    INV = ffi.ERR_INVALID_ARGUMENT
    # (path, fd_ok, ctx, window, intervals, n, query, exclude, mapq) -> code, message
    cases = [
        (files["good"], True, None, 100, None, 0, None, 1796, 0, INV, "null or invalid argument"),
        (files["good"], False, fake, 100, None, 0, None, 1796, 0, INV, "null or invalid argument"),
        (files["good"], True, fake, 100, None, 0, None, 65536, 0, INV, "null or invalid argument"),
        (files["good"], True, fake, 100, None, 0, None, 0, 256, INV, "null or invalid argument"),
        (files["good"], True, fake, 2 ** 31, None, 0, None, 1796, 0, INV, "null or invalid argument"),
        (files["good"], True, fake, 100, one, 1, None, 1796, 0, INV, "null or invalid argument"),          # a window and intervals
        (files["good"], True, fake, 0, None, 1, None, 1796, 0, INV, "null or invalid argument"),           # a count without a list
        (files["good"], True, fake, 0, one, 1, b"q1", 1796, 0, INV, "mean depth per BED interval cannot be combined with a query"),
        (files["good"], True, fake, 0, intervals_of([(3, 10, 20)]), 1, None, 1796, 0, INV, "interval 0 is not one of the file's"),
        (files["good"], True, fake, 0, intervals_of([(-1, 10, 20)]), 1, None, 1796, 0, INV, "interval 0 is not one of the file's"),
        (files["good"], True, fake, 0, intervals_of([(0, 10, 20), (0, 20, 20)]), 2, None, 1796, 0, INV, "interval 1 is not one of the file's"),
        (files["good"], True, fake, 0, intervals_of([(2, 10, 5001)]), 1, None, 1796, 0, INV, "interval 0 is not one of the file's"),
        (files["unsorted"], True, fake, 100, None, 0, None, 1796, 0, ffi.ERR_UNSORTED, dm.NOT_SORTED),
        (files["unsorted"], True, fake, 0, one, 1, None, 1796, 0, ffi.ERR_UNSORTED, dm.NOT_SORTED),
        (files["unsorted"], True, fake, 0, None, 0, None, 1796, 0, ffi.ERR_UNSORTED, dm.NOT_SORTED),       # the empty list does not excuse the header
        (files["good"], True, fake, 100, None, 0, b"", 1796, 0, INV, "parsing query: "),
        (files["good"], True, fake, 100, None, 0, b"nope", 1796, 0, INV, "querying BAM file: "),
    ]
    for path, fd_ok, ctx, window, iv, n, query, exclude, mapq, code, msg in cases:
        bam = C.c_void_p()
        assert lib.ngsq_bam_open(path.encode(), 0, C.byref(bam)) == 0
        try:
            fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
            rc = lib.ngsq_bam_depth_windows(bam, ctx, fd if fd_ok else -1, window, iv, n, query, None, exclude, mapq, 0, 0, 0, 0, None)
            os.close(fd)
            assert rc == code, (window, n, query, rc)
            assert msg in lib.ngsq_bam_last_error().decode(), (msg, lib.ngsq_bam_last_error())
            assert os.path.getsize(out) == 0
        finally:
            lib.ngsq_bam_close(bam)
    # a query without an index
    noindex = write_case(str(tmp_path / "noindex.bam"), *td.case_query()[:2], td.case_query()[2][:50], index=False)
    bam = C.c_void_p()
    assert lib.ngsq_bam_open(noindex.encode(), 0, C.byref(bam)) == 0
    try:
        fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
        assert lib.ngsq_bam_depth_windows(bam, fake, fd, 100, None, 0, b"q1", None, 1796, 0, 0, 0, 0, 0, None) == INV
        assert "reading BAM index: " in lib.ngsq_bam_last_error().decode()
        os.close(fd)
    finally:
        lib.ngsq_bam_close(bam)


def test_a_reader_that_is_not_fresh_is_refused(lib, files, tmp_path):
    """A batch read on the host first: NGSQ_ERR_STATE in window mode, in interval mode and for the empty list, nothing written."""
    C = ffi.C
    fake = C.cast(C.c_void_p(8), ffi.ctx_p)
    out = str(tmp_path / "o")
    one = intervals_of([(0, 10, 20)])
    for window, iv, n in ((100, None, 0), (0, one, 1), (0, None, 0)):
        bam = C.c_void_p()
        assert lib.ngsq_bam_open(files["good"].encode(), 0, C.byref(bam)) == 0
        try:
            b = ffi.Batch()
            assert lib.ngsq_bam_next_batch(bam, 10, C.byref(b)) == 0 and b.n_records == 10
            fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
            rc = lib.ngsq_bam_depth_windows(bam, fake, fd, window, iv, n, None, None, 1796, 0, 0, 0, 0, 0, None)
            os.close(fd)
            assert rc == ffi.ERR_STATE, (window, n, rc)
            assert "the depth is computed from a reader no record has been read from" in lib.ngsq_bam_last_error().decode()
            assert os.path.getsize(out) == 0
        finally:
            lib.ngsq_bam_close(bam)


def test_no_interval_and_an_empty_region_need_no_gpu(lib, files, tmp_path):
    """The empty interval list and a region behind its sequence's end: OK, nothing written, every count 0."""
    C = ffi.C
    fake = C.cast(C.c_void_p(8), ffi.ctx_p)
    out = str(tmp_path / "o")
    # (the empty list with a query: no interval is combined with it, so it is not refused, and the query is not looked at)
    for window, query in ((0, None), (0, b"q1"), (0, b"nope"), (100, b"q3:5001"), (MAX, b"q1:300001")):
        bam = C.c_void_p()
        assert lib.ngsq_bam_open(files["good"].encode(), 0, C.byref(bam)) == 0
        try:
            fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
            rep = ffi.DepthWindowsReport()
            rep.lines = rep.records_scanned = 77
            assert lib.ngsq_bam_depth_windows(bam, fake, fd, window, None, 0, query, None, 1796, 0, 0, 0, 0, 0, C.byref(rep)) == 0
            os.close(fd)
            assert os.path.getsize(out) == 0
            for k in ("records_scanned", "records_counted", "lines", "text_bytes", "sequences", "depth_sum", "tiles", "passes", "batches", "ranges"):
                assert getattr(rep, k) == 0, k
        finally:
            lib.ngsq_bam_close(bam)
    assert wm.expected(files["good"], intervals=[])[0] == b"" and wm.expected(files["good"], window=100, query="q3:5001")[0] == b""


def test_the_bindings_declare_the_call(lib):
    assert "ngsq_bam_depth_windows" in ffi.PROTOTYPES and hasattr(host, "bam_depth_windows")
    assert [k for k, _ in ffi.DepthWindowsReport._fields_][:6] == ["records_scanned", "records_counted", "lines", "text_bytes", "sequences", "depth_sum"]
