"""`ngs depth --by <N|BED>` on the GPU: the bytes ngsq_bam_depth_windows writes equal the test-side model's
(tests/depth_windows_model.py) and the report's counts the model's, on the inputs tests/test_depth.py and tests/test_depth_by.py
build and hold to their edges: the smallest files; windows against tiles at every window size around a wave, a block, a tile and
the sequence; lines against format passes; sums above 2^32 with the carry of P across tiles; rounding and digits; filters,
batches, the 195-sequence header; regions; BED intervals at tile edges, overlapping, repeated and unsorted, on sequences with
and without records; a record out of order; the command line; and twelve random files."""
import os
import subprocess

import numpy as np
import pytest

from ngs_amd import build, ffi, host
from tests import bamio
from tests import depth_model as dm
from tests import depth_windows_model as wm
from tests import test_depth as td
from tests import test_depth_by as tb
from tests.test_depth_gpu import same
from tests.test_view import indexed_copy

pytestmark = pytest.mark.gpu

MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


@pytest.fixture(scope="module")
def d(tmp_path_factory):
    return tmp_path_factory.mktemp("depthby")


_model = {}


def model(path, window, intervals, query, exclude_flags, min_mapq):
    """The model's answer, computed once per input and question."""
    key = (path, window, None if intervals is None else tuple(intervals), query, exclude_flags, min_mapq)
    if key not in _model:
        _model[key] = wm.expected(path, window=window, intervals=intervals, query=query, exclude_flags=exclude_flags, min_mapq=min_mapq)
    return _model[key]


def check(lib, path, d, window=0, intervals=None, query=None, bed=None, **kw):
    """One call against the model: the bytes, and the report's counts."""
    out = str(d / "o.txt")
    rep = host.bam_depth_windows(path, out, window=window, intervals=None if bed else intervals, bed=bed, query=query, lib=lib, **kw)
    got = open(out, "rb").read()
    want, info = model(path, window, intervals, query, kw.get("exclude_flags", dm.EXCLUDE_FLAGS), kw.get("min_mapq", 0))
    same(got, want)
    assert rep["text_bytes"] == len(got) and rep["lines"] == info["lines"] == got.count(b"\n")
    assert rep["records_counted"] == info["records_counted"] and rep["sequences"] == info["sequences"]
    assert rep["depth_sum"] == info["depth_sum"] % 2 ** 64
    if info["records_scanned"] is not None:
        assert rep["records_scanned"] == info["records_scanned"] and rep["ranges"] == 0
    return got, rep


# ---- the smallest files ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [4, 1, MAX])
@pytest.mark.parametrize("name", ["no_record", "one_record", "L1"])
def test_smallest_files(gpu_lib, d, name, window):
    names, lens, recs = td.case_small()[name]
    path = str(d / (name + ".bam"))
    if not os.path.exists(path):
        td.write_case(path, names, lens, recs)
    for t in (1, 0):
        got, rep = check(gpu_lib, path, d, window=window, tile_positions=t)
    if name == "no_record" and window == 4:
        assert got == b"".join(b"a\t%d\t%d\t0.00\n" % (k, k + 4) for k in range(0, 1000, 4)) + b"b\t0\t1\t0.00\n"
        assert rep["lines"] == 251 and rep["tiles"] == 0 and rep["batches"] == 0 and rep["passes"] == 2
    if name == "L1" and window == 1:
        assert got == b"a\t0\t1\t1.00\nb\t0\t1\t2.00\nc\t0\t1\t0.00\n"


# ---- windows against tiles --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shape_files(d):
    out = {}
    for name, case in (("lengths", td.case_lengths), ("tiles", td.case_tiles), ("pow10", td.case_pow10), ("piles", td.case_piles)):
        names, lens, recs = case()
        out[name] = (td.write_case(str(d / (name + ".bam")), names, lens, recs), lens)
    return out


@pytest.mark.parametrize("which", range(17))
@pytest.mark.parametrize("name", ["tiles", "lengths"])
def test_window_sizes_at_every_tile_size(gpu_lib, d, shape_files, name, which):
    path, lens = shape_files[name]
    T = td.tile()
    window = tb.tile_windows()[which]
    for t in (1, T, T + 1, 0):
        got, rep = check(gpu_lib, path, d, window=window, tile_positions=t)
        eff = host.depth_tile_positions(t, lib=gpu_lib)
        assert rep["tiles"] == sum(-(-L // eff) for L in lens)   # every sequence of these files has records
    check(gpu_lib, path, d, window=window, tile_positions=1, lines_per_pass=1)


@pytest.mark.parametrize("tile", [1, 0])
def test_lines_against_passes(gpu_lib, d, tile):
    """255, 256, 257 and 513 windows at 256 lines a pass: with one tile a sequence each sequence is one line source."""
    names, lens, recs = tb.case_passes()
    path = str(d / "passes.bam")
    if not os.path.exists(path):
        td.write_case(path, names, lens, recs)
    _, rep = check(gpu_lib, path, d, window=3, lines_per_pass=1, tile_positions=tile)
    if tile == 0:
        assert rep["passes"] == tb.passes_of(tb.PASS_WINDOWS) == 7 and rep["tiles"] == 4
    else:
        # tiles of 1024 positions end 341 or 342 windows each: the windows that end in every tile, at 256 lines a pass
        T = td.tile()
        per_tile = [[min(t0 + T, L) // 3 - t0 // 3 + (1 if t0 + T >= L and L % 3 else 0) for t0 in range(0, L, T)] for L in lens]
        assert rep["passes"] == sum(tb.passes_of(x) for x in per_tile)
    _, rep = check(gpu_lib, path, d, window=3)
    assert rep["passes"] == 4


# ---- 64 bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [65536, 0])
def test_sums_above_32_bits(gpu_lib, d, tile):
    names, lens, recs = tb.case_wide()
    path = str(d / "wide.bam")
    if not os.path.exists(path):
        td.write_case(path, names, lens, recs)
    got, rep = check(gpu_lib, path, d, window=MAX, tile_positions=tile)
    assert got == b"g\t0\t2000100\t2999.85\n" and rep["depth_sum"] == 6_000_000_000
    for window, lines in ((65536, 31), (1000, 2001)):
        got, rep = check(gpu_lib, path, d, window=window, tile_positions=tile)
        assert rep["lines"] == lines and rep["depth_sum"] == 6_000_000_000
    if tile:
        assert rep["tiles"] == 31


# ---- rounding and digits ----------------------------------------------------------------------------------------------------------
def test_rounding_carries_and_rounds_half_up(gpu_lib, d):
    names, lens, recs = tb.case_rounding()
    path = td.write_case(str(d / "rounding.bam"), names, lens, recs)
    got, _ = check(gpu_lib, path, d, window=200)
    assert got == b"a\t0\t200\t1.00\nb\t0\t200\t0.01\nc\t0\t200\t0.01\nc\t200\t201\t0.00\n"


@pytest.mark.parametrize("name,windows", [("piles", (1, 7)), ("pow10", (1, 10))])
def test_digits_of_means_and_coordinates(gpu_lib, d, shape_files, name, windows):
    path, _ = shape_files[name]
    for window in windows:
        got, _ = check(gpu_lib, path, d, window=window, tile_positions=1)
        if name == "piles":                                       # means of one to three digits, and of four at one position a window
            assert {4, 5, 6} <= {len(ln.split(b"\t")[3]) for ln in got.splitlines()}
        if name == "piles" and window == 1:
            assert b"\t1000.00\n" in got and b"\t999.00\n" in got and b"\t10.00\n" in got and b"\t9.00\n" in got
    check(gpu_lib, path, d, window=windows[1], lines_per_pass=1)


# ---- filters, batches, header -----------------------------------------------------------------------------------------------------
def test_flag_bits_and_mapq(gpu_lib, d):
    names, lens, recs = td.case_filters()
    path = td.write_case(str(d / "filters.bam"), names, lens, recs)
    check(gpu_lib, path, d, window=10)
    for bits in (0, 4, 256, 512, 1024, 65535):
        check(gpu_lib, path, d, window=10, exclude_flags=bits)
    for m in (9, 10, 11, 255):
        check(gpu_lib, path, d, window=10, exclude_flags=0, min_mapq=m)
    check(gpu_lib, path, d, window=10, min_mapq=10)
    check(gpu_lib, path, d, intervals=[(0, 100, 400), (0, 300, 350)], min_mapq=10)


@pytest.fixture(scope="module")
def batches_file(d):
    names, lens, recs = td.case_batches()
    return td.write_case(str(d / "batches.bam"), names, lens, recs), len(recs)


@pytest.mark.parametrize("batch", [1, 7, 64, 65, 0])
def test_batch_sizes(gpu_lib, d, batches_file, batch):
    path, n = batches_file
    got, rep = check(gpu_lib, path, d, window=100, batch_records=batch, tile_positions=1)
    assert rep["batches"] >= (-(-n // batch) if batch else 1)
    assert b"b3\t0\t50\t0.00\n" in got


def test_genome_header_with_empty_sequences_around_covered_ones(gpu_lib, d):
    names, lens, recs = td.case_genome()
    path = td.write_case(str(d / "genome.bam"), names, lens, recs)
    got, rep = check(gpu_lib, path, d, window=1000, batch_records=64)
    assert got.startswith(b"chr1\t0\t1000\t0.00\n") and got.endswith(b"\t%d\t0.00\n" % lens[-1]) and rep["sequences"] == 195
    check(gpu_lib, path, d, window=1000)


def test_long_cigar_fixture(gpu_lib, tmp_path):
    path = indexed_copy("hand_longcigar.bam", tmp_path)
    got, _ = check(gpu_lib, path, tmp_path, window=1000)
    assert got.startswith(b"chr1\t0\t1000\t0.00\nchr1\t1000\t2000\t0.0")
    check(gpu_lib, path, tmp_path, window=7, query="chr1:1001-1040")
    check(gpu_lib, path, tmp_path, intervals=[(0, 1000, 1035), (0, 990, 1010)])


# ---- regions ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def query_file(d):
    names, lens, recs = td.case_query()
    return td.write_case(str(d / "query.bam"), names, lens, recs, block_payload=3000)


@pytest.mark.parametrize("query", td.QUERIES)
def test_regions(gpu_lib, d, query_file, query):
    for window in (7, 1000):
        got, rep = check(gpu_lib, query_file, d, window=window, query=query, batch_records=257)
        if query in ("q2", "q2:100-200", "q1:300001"):
            assert rep["records_scanned"] == 0 and rep["tiles"] == 0            # a region without a record, an empty region
        check(gpu_lib, query_file, d, window=window, query=query, tile_positions=1, lines_per_pass=1)
    if query == "q1:4500-5500":
        got, _ = check(gpu_lib, query_file, d, window=1000, query=query)
        assert got == b"q1\t4499\t5000\t1.00\nq1\t5000\t5500\t1.00\n"                 # the first and the last window short, aligned to 0


def test_one_walk_per_chunk_gives_the_same_bytes(gpu_lib, d, query_file):
    a, ra = check(gpu_lib, query_file, d, window=1000, query="q1:6000-200000", coalesce_gap=1, batch_records=500)
    b, rb = check(gpu_lib, query_file, d, window=1000, query="q1:6000-200000")
    assert a == b and ra["ranges"] >= 2 and rb["ranges"] == 1


# ---- BED ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [1, 0])
def test_bed_intervals_against_tiles_in_file_order(gpu_lib, d, shape_files, tile):
    path, _ = shape_files["tiles"]
    iv = tb.bed_tiles()
    got, rep = check(gpu_lib, path, d, intervals=iv, tile_positions=tile)
    assert [tuple(map(int, ln.split(b"\t")[1:3])) for ln in got.splitlines()] == [(s, e) for _, s, e in iv]
    assert rep["passes"] == 1


def test_bed_on_sequences_with_and_without_records(gpu_lib, d, batches_file):
    """Intervals on b0 and b5 (records), b3 (none); b1, b2 and b4 have records and no interval: their records still count."""
    path, _ = batches_file
    iv = [(5, 100, 11000), (0, 10, 500), (3, 0, 50), (0, 8000, 9000), (5, 0, 12000)]
    for batch in (7, 0):
        got, rep = check(gpu_lib, path, d, intervals=iv, batch_records=batch, tile_positions=1)
        assert rep["records_counted"] == dm.expected(path)[1]["records_counted"] and rep["sequences"] == 3
    assert [ln.split(b"\t")[0] for ln in got.splitlines()] == [b"b0", b"b0", b"b3", b"b5", b"b5"] and b"b3\t0\t50\t0.00\n" in got
    # b0 and b5 went through the reduce pass, and b3 where a batch reaches over it; b1, b2 and b4 (1 + 7 + 1 tiles) did not
    assert 9 + 12 <= rep["tiles"] <= 9 + 12 + 1


@pytest.mark.parametrize("n", [255, 256, 257])
def test_bed_lines_against_passes(gpu_lib, d, batches_file, n):
    path, _ = batches_file
    rng = np.random.default_rng(n)
    iv = []
    for _ in range(n):
        s = int(rng.integers(0, 8999))
        iv.append((0, s, int(rng.integers(s + 1, 9001))))
    _, rep = check(gpu_lib, path, d, intervals=iv, lines_per_pass=1)
    assert rep["passes"] == -(-n // 256)


def test_bed_file_and_list_give_the_same(gpu_lib, d, batches_file):
    """A BED file read with bed=, its last end clipped to L by the reader, and the same intervals passed as a list."""
    path, _ = batches_file
    bed = str(d / "t.bed")
    with open(bed, "wb") as f:
        f.write(b"#c\nb5\t100\t200\tx\nb0\t0\t9000\nb0\t8990\t99999\r\nb4\t1\t2\n")
    iv = host.depth_read_bed(path, bed, lib=gpu_lib)
    assert iv == [(5, 100, 200), (0, 0, 9000), (0, 8990, 9000), (4, 1, 2)]
    a, _ = check(gpu_lib, path, d, intervals=iv, bed=bed)
    b, _ = check(gpu_lib, path, d, intervals=iv)
    assert a == b and b"b0\t8990\t9000\t" in a


def test_the_empty_bed(gpu_lib, d, batches_file):
    path, _ = batches_file
    bed = str(d / "empty.bed")
    with open(bed, "wb") as f:
        f.write(b"# nothing\n\ntrack x\n")
    got, rep = check(gpu_lib, path, d, intervals=[], bed=bed)
    assert got == b"" and rep["records_scanned"] == 0 and rep["batches"] == 0 and rep["lines"] == 0


# ---- order --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad,batch", td.ORDER_CASES)
def test_a_record_out_of_order(gpu_lib, d, bad, batch):
    names, lens, recs = td.case_order(bad)
    path = td.write_case(str(d / ("order%d.bam" % bad)), names, lens, recs, in_order=False)
    with pytest.raises(dm.DepthError) as want:
        wm.expected(path, window=100)
    for kw in (dict(window=100), dict(intervals=[(0, 5, 4000)])):
        with pytest.raises(host.NgsqError) as e:
            host.bam_depth_windows(path, str(d / "o.txt"), batch_records=batch, lib=gpu_lib, **kw)
        assert e.value.code == ffi.ERR_UNSORTED and e.value.message == str(want.value)
        assert f"record {bad} (0-based) is out of coordinate order" in e.value.message


# ---- the command line -------------------------------------------------------------------------------------------------------------
def test_command_line_file_stdout_bed_and_closed_pipe(gpu_lib, ngs, d, query_file):
    lib_out = str(d / "lib.txt")
    host.bam_depth_windows(query_file, lib_out, window=100, lib=gpu_lib)
    want = open(lib_out, "rb").read()
    same(want, wm.expected(query_file, window=100)[0])
    out = str(d / "cli.txt")
    r = subprocess.run([ngs, "depth", "--by", "100", "-o", out, query_file], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    same(open(out, "rb").read(), want)
    r = subprocess.run([ngs, "-q", "depth", "--by", "+100", query_file], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    same(r.stdout, want)
    r = subprocess.run([ngs, "depth", "--by", "1000", query_file, "q1:4500-5500"], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == b"q1\t4499\t5000\t1.00\nq1\t5000\t5500\t1.00\n", r.stderr
    bed = str(d / "cli.bed")
    with open(bed, "wb") as f:
        f.write(b"q3\t4000\t9000\nq1\t4000\t6000\nq2\t5\t6\n")
    host.bam_depth_windows(query_file, lib_out, bed=bed, lib=gpu_lib)
    r = subprocess.run([ngs, "depth", "-v", "--by", bed, query_file], capture_output=True, timeout=120)
    assert r.returncode == 0 and b"format passes" in r.stderr, r.stderr
    same(r.stdout, open(lib_out, "rb").read())
    same(r.stdout, wm.expected(query_file, intervals=[(2, 4000, 5000), (0, 4000, 6000), (1, 5, 6)])[0])
    r = subprocess.run([ngs, "depth", "--by", "100", "-o", "/dev/full", query_file], capture_output=True, timeout=120)
    assert r.returncode == 1 and b"Error: writing depth to stream: No space left on device (os error 28)" in r.stderr
    p = subprocess.Popen([ngs, "depth", "--by", "1", query_file], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    p.stdout.close()                                                    # the reader goes away: the write's error, not a signal
    err = p.stderr.read()
    assert p.wait(timeout=120) == 1 and b"Error: writing depth to stream: Broken pipe (os error 32)" in err


# ---- random files -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_random_files(gpu_lib, d, seed):
    names, lens, hb = td.case_random(seed)
    path = str(d / ("random%d.bam" % seed))
    bamio.write_bam(path, hb, names, lens, with_index=False)
    rng = np.random.default_rng(1000 + seed)
    check(gpu_lib, path, d, window=int(rng.integers(1, 5001)), tile_positions=1, exclude_flags=int(rng.choice([dm.EXCLUDE_FLAGS, 0])))
    iv = []
    for _ in range(int(rng.integers(1, 301))):
        r = int(rng.integers(0, len(lens)))
        s = int(rng.integers(0, lens[r]))
        iv.append((r, s, int(rng.integers(s + 1, lens[r] + 1))))
    check(gpu_lib, path, d, intervals=iv, tile_positions=1, batch_records=int(rng.choice([63, 64, 65, 257])), min_mapq=int(rng.choice([0, 4])))
