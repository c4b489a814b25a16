"""`ngs depth --by <N|BED> --thresholds <T[,T...]>` on the GPU: the bytes ngsq_bam_depth_thresholds writes
equal the test-side model's (tests/depth_thresholds_model.py), the report's counts -- `covered` among them -- the model's, and the
first four columns ngsq_bam_depth_windows' bytes of the same question, on the inputs tests/test_depth.py, tests/test_depth_by.py
and tests/test_depth_thresholds.py build and hold to their edges: the smallest files; the depth at T - 1, T and T + 1; window and
interval ends at the 1024-position granule's and the tile's edges, at tile sizes 1, T, T + 1 and the default and at 256 lines a
pass; the carries of the counts over many tiles, whole blocks and counts above 16 bits; filters, batches, the 195-sequence
header; regions; BED intervals of every kind; a record out of order; the command line; and twelve random files.  Every test here
calls the new entry or the new flag and so fails without them."""
import os
import subprocess

import numpy as np
import pytest

from ngs_amd import build, ffi, host
from tests import bamio
from tests import depth_model as dm
from tests import depth_thresholds_model as tm
from tests import test_depth as td
from tests import test_depth_by as tb
from tests import test_depth_thresholds as tt
from tests.test_depth_gpu import same

pytestmark = pytest.mark.gpu

MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


@pytest.fixture(scope="module")
def d(tmp_path_factory):
    return tmp_path_factory.mktemp("depththr")


_model, _plain = {}, {}


def model(path, thresholds, window, intervals, query, exclude_flags, min_mapq):
    """The model's answer, computed once per input and question."""
    key = (path, tuple(thresholds), window, None if intervals is None else tuple(intervals), query, exclude_flags, min_mapq)
    if key not in _model:
        _model[key] = tm.expected(path, thresholds, window=window, intervals=intervals, query=query, exclude_flags=exclude_flags, min_mapq=min_mapq)
    return _model[key]


def plain(lib, path, d, window, intervals, query, exclude_flags, min_mapq):
    """ngsq_bam_depth_windows' bytes of the same question, computed once per input and question (they depend on nothing else)."""
    key = (path, window, None if intervals is None else tuple(intervals), query, exclude_flags, min_mapq)
    if key not in _plain:
        out = str(d / "plain.txt")
        host.bam_depth_windows(path, out, window=window, intervals=intervals, query=query, exclude_flags=exclude_flags, min_mapq=min_mapq, lib=lib)
        _plain[key] = open(out, "rb").read()
    return _plain[key]


def check(lib, path, d, thresholds, window=0, intervals=None, query=None, bed=None, **kw):
    """One call against the model: the bytes, the report's counts, and the first four columns against the call without thresholds."""
    out = str(d / "o.txt")
    rep = host.bam_depth_windows(path, out, window=window, intervals=None if bed else intervals, bed=bed, query=query, thresholds=thresholds, lib=lib, **kw)
    got = open(out, "rb").read()
    ex, mq = kw.get("exclude_flags", dm.EXCLUDE_FLAGS), kw.get("min_mapq", 0)
    want, info = model(path, thresholds, window, intervals, query, ex, mq)
    same(got, want)
    assert rep["text_bytes"] == len(got) and rep["lines"] == info["lines"] == got.count(b"\n")
    assert rep["records_counted"] == info["records_counted"] and rep["sequences"] == info["sequences"]
    assert rep["depth_sum"] == info["depth_sum"] % 2 ** 64
    assert rep["covered"] == info["covered"] and len(rep["covered"]) == len(thresholds)
    if info["records_scanned"] is not None:
        assert rep["records_scanned"] == info["records_scanned"] and rep["ranges"] == 0
    same(tm.first_columns(got, len(thresholds)), plain(lib, path, d, window, intervals, query, ex, mq))
    return got, rep


# ---- the smallest files ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [1, 4, MAX])
@pytest.mark.parametrize("name", ["no_record", "one_record", "L1"])
def test_smallest_files(gpu_lib, d, name, window):
    """K = 1, 2 and 8; thresholds 1, the largest depth (2 on L1), the largest depth + 1, and 2^31 - 1."""
    names, lens, recs = td.case_small()[name]
    path = str(d / (name + ".bam"))
    if not os.path.exists(path):
        td.write_case(path, names, lens, recs)
    for thresholds in ([1], [2], [3], [MAX], [1, 2], [2, 3], [1, 2, 3, 4, 5, 6, 7, MAX]):
        for t in (1, 0):
            got, rep = check(gpu_lib, path, d, thresholds, window=window, tile_positions=t)
    if name == "no_record" and window == 4:
        assert got == b"".join(b"a\t%d\t%d\t0.00" % (k, k + 4) + b"\t0" * 8 + b"\n" for k in range(0, 1000, 4)) + b"b\t0\t1\t0.00" + b"\t0" * 8 + b"\n"
        assert rep["tiles"] == 0 and rep["batches"] == 0 and rep["covered"] == [0] * 8
    if name == "L1" and window == 1:
        assert got == b"a\t0\t1\t1.00\t1" + b"\t0" * 7 + b"\nb\t0\t1\t2.00\t1\t1" + b"\t0" * 6 + b"\nc\t0\t1\t0.00" + b"\t0" * 8 + b"\n"
    if name == "one_record" and window == MAX:
        assert got == b"a\t0\t1000\t0.01\t5" + b"\t0" * 7 + b"\n"


# ---- the depth against T ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shape_files(d):
    out = {}
    for name, case in (("lengths", td.case_lengths), ("tiles", td.case_tiles), ("piles", td.case_piles), ("carry", tt.case_carry)):
        names, lens, recs = case()
        out[name] = (td.write_case(str(d / (name + ".bam")), names, lens, recs), lens)
    return out


@pytest.mark.parametrize("window", [1, 7, 1000])
def test_depth_at_and_around_every_threshold(gpu_lib, d, shape_files, window):
    path, _ = shape_files["piles"]
    for t in (1, 0):
        got, rep = check(gpu_lib, path, d, tt.PILES_THRESHOLDS, window=window, tile_positions=t)
    assert rep["covered"][3] == 1 and rep["covered"][4] == 0 and rep["covered"][0] == 1999
    check(gpu_lib, path, d, tt.PILES_THRESHOLDS, window=window, lines_per_pass=1)
    check(gpu_lib, path, d, [999, 1000], intervals=[(0, 1498, 1501), (0, 1499, 1500), (0, 0, 4000), (0, 1500, 1501)])


# ---- block and tile edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(17))
@pytest.mark.parametrize("name", ["tiles", "lengths"])
def test_window_sizes_at_every_tile_size(gpu_lib, d, shape_files, name, which):
    path, lens = shape_files[name]
    T = td.tile()
    window = tb.tile_windows()[which]
    for t in (1, T, T + 1, 0):
        got, rep = check(gpu_lib, path, d, [1, 2, 3, 4], window=window, tile_positions=t)
        eff = host.depth_tile_positions(t, lib=gpu_lib)
        assert rep["tiles"] == sum(-(-L // eff) for L in lens)
    check(gpu_lib, path, d, [1, 2, 3, 4], window=window, tile_positions=1, lines_per_pass=1)
    check(gpu_lib, path, d, [2], window=window, tile_positions=T + 1, lines_per_pass=1)


@pytest.mark.parametrize("tile", [1, 1025, 0])
def test_bed_intervals_against_blocks_and_tiles_in_file_order(gpu_lib, d, shape_files, tile):
    """Starts and ends at G - 1, G, G + 1, 0 and L; with a tile of 2 G the block boundary at G lies inside a tile, with one of G on its end."""
    path, _ = shape_files["tiles"]
    iv = tb.bed_tiles()
    for thresholds in ([1, 2, 3, 4], [1, 2, 3, 4, 5, 6, 7, 8], [3]):
        got, rep = check(gpu_lib, path, d, thresholds, intervals=iv, tile_positions=tile)
        assert [tuple(map(int, ln.split(b"\t")[1:3])) for ln in got.splitlines()] == [(s, e) for _, s, e in iv]
        assert rep["passes"] == 1


# ---- carries ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [1, 4097, 0])
def test_counts_carried_over_tiles_and_above_16_bits(gpu_lib, d, shape_files, tile):
    path, _ = shape_files["carry"]
    T = td.tile()
    for window in (MAX, 66_000, T, T - 1, 3 * T, 5000):
        got, rep = check(gpu_lib, path, d, [1, 2, 3], window=window, tile_positions=tile)
        assert rep["covered"] == [70_004, 1104, 10]
        if window == MAX:
            assert got == b"k\t0\t70007\t1.02\t70004\t1104\t10\n"
    got, rep = check(gpu_lib, path, d, [1, 2, 3, 4, 5], intervals=tt.bed_carry(), tile_positions=tile)
    assert got.splitlines()[1].endswith(b"\t68995\t1094\t10\t0\t0") and got.splitlines()[0].endswith(b"\t2000\t0\t0\t0\t0")
    check(gpu_lib, path, d, [1, 2], window=T, tile_positions=tile, lines_per_pass=1)


# ---- filters, batches, header -----------------------------------------------------------------------------------------------------
def test_flag_bits_and_mapq(gpu_lib, d):
    names, lens, recs = td.case_filters()
    path = td.write_case(str(d / "filters.bam"), names, lens, recs)
    thr = [1, 2, 3, 5]
    check(gpu_lib, path, d, thr, window=10)
    for bits in (0, 4, 256, 512, 1024, 65535):
        check(gpu_lib, path, d, thr, window=10, exclude_flags=bits)
    for m in (9, 10, 11, 255):
        check(gpu_lib, path, d, thr, window=10, exclude_flags=0, min_mapq=m)
    check(gpu_lib, path, d, thr, window=10, min_mapq=10)
    check(gpu_lib, path, d, thr, intervals=[(0, 100, 400), (0, 300, 350)], min_mapq=10)


@pytest.fixture(scope="module")
def batches_file(d):
    names, lens, recs = td.case_batches()
    return td.write_case(str(d / "batches.bam"), names, lens, recs), len(recs)


@pytest.mark.parametrize("batch", [1, 7, 64, 65, 0])
def test_batch_sizes(gpu_lib, d, batches_file, batch):
    path, n = batches_file
    got, rep = check(gpu_lib, path, d, [1, 2, 4], window=100, batch_records=batch, tile_positions=1)
    assert rep["batches"] >= (-(-n // batch) if batch else 1)
    assert b"b3\t0\t50\t0.00\t0\t0\t0\n" in got


def test_genome_header_with_uncounted_sequences_between_counted_ones(gpu_lib, d):
    names, lens, recs = td.case_genome()
    path = td.write_case(str(d / "genome.bam"), names, lens, recs)
    got, rep = check(gpu_lib, path, d, [1, 2], window=1000, batch_records=64)
    assert got.startswith(b"chr1\t0\t1000\t0.00\t0\t0\n") and got.endswith(b"\t%d\t0.00\t0\t0\n" % lens[-1]) and rep["sequences"] == 195
    assert b"\t0.00\t0\t0\nchr2\t" in got and rep["covered"][0] > 0
    check(gpu_lib, path, d, [1, 2], window=1000)


# ---- regions ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def query_file(d):
    names, lens, recs = td.case_query()
    return td.write_case(str(d / "query.bam"), names, lens, recs, block_payload=3000)


@pytest.mark.parametrize("query", td.QUERIES)
def test_regions(gpu_lib, d, query_file, query):
    for window in (7, 1000):
        got, rep = check(gpu_lib, query_file, d, [1, 2, 3], window=window, query=query, batch_records=257)
        if query in ("q2", "q2:100-200", "q1:300001"):
            assert rep["records_scanned"] == 0 and rep["tiles"] == 0 and rep["covered"] == [0, 0, 0]
        check(gpu_lib, query_file, d, [1, 2, 3], window=window, query=query, tile_positions=1, lines_per_pass=1)
    if query == "q1:4500-5500":
        got, _ = check(gpu_lib, query_file, d, [1, 2], window=1000, query=query)
        assert got == b"q1\t4499\t5000\t1.00\t501\t0\nq1\t5000\t5500\t1.00\t500\t0\n"


def test_one_walk_per_chunk_gives_the_same_bytes(gpu_lib, d, query_file):
    a, ra = check(gpu_lib, query_file, d, [1, 2], window=1000, query="q1:6000-200000", coalesce_gap=1, batch_records=500)
    b, rb = check(gpu_lib, query_file, d, [1, 2], window=1000, query="q1:6000-200000")
    assert a == b and ra["ranges"] >= 2 and rb["ranges"] == 1


# ---- BED ----------------------------------------------------------------------------------------------------------------------------
def test_bed_on_sequences_with_and_without_records(gpu_lib, d, batches_file):
    """Intervals on b0 and b5 (records), b3 (none); b1, b2 and b4 have records and no interval; overlapping, nested, repeated, descending."""
    path, _ = batches_file
    iv = [(5, 100, 11000), (0, 10, 500), (3, 0, 50), (0, 8000, 9000), (5, 0, 12000), (0, 200, 300), (0, 200, 300), (0, 100, 400), (5, 50, 60)]
    for batch in (7, 0):
        got, rep = check(gpu_lib, path, d, [1, 2, 3], intervals=iv, batch_records=batch, tile_positions=1)
        assert rep["records_counted"] == dm.expected(path)[1]["records_counted"] and rep["sequences"] == 3
    assert [ln.split(b"\t")[0] for ln in got.splitlines()] == [b"b0"] * 5 + [b"b3"] + [b"b5"] * 3 and b"b3\t0\t50\t0.00\t0\t0\t0\n" in got


@pytest.mark.parametrize("n", [255, 256, 257])
def test_bed_lines_against_passes(gpu_lib, d, batches_file, n):
    path, _ = batches_file
    rng = np.random.default_rng(n)
    iv = []
    for _ in range(n):
        s = int(rng.integers(0, 8999))
        iv.append((0, s, int(rng.integers(s + 1, 9001))))
    _, rep = check(gpu_lib, path, d, [1, 2, 3, 4, 5, 6, 7, 8], intervals=iv, lines_per_pass=1)
    assert rep["passes"] == -(-n // 256)


def test_bed_file_and_list_give_the_same_and_the_empty_bed(gpu_lib, d, batches_file):
    path, _ = batches_file
    bed = str(d / "t.bed")
    with open(bed, "wb") as f:
        f.write(b"#c\nb5\t100\t200\tx\nb0\t0\t9000\nb0\t8990\t99999\r\nb4\t1\t2\n")
    iv = host.depth_read_bed(path, bed, lib=gpu_lib)
    a, _ = check(gpu_lib, path, d, [1, 3], intervals=iv, bed=bed)
    b, _ = check(gpu_lib, path, d, [1, 3], intervals=iv)
    assert a == b and b"b0\t8990\t9000\t" in a
    with open(bed, "wb") as f:
        f.write(b"# nothing\n\ntrack x\n")
    got, rep = check(gpu_lib, path, d, [1, 3], intervals=[], bed=bed)
    assert got == b"" and rep["records_scanned"] == 0 and rep["batches"] == 0 and rep["lines"] == 0 and rep["covered"] == [0, 0]


# ---- order --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad,batch", td.ORDER_CASES)
def test_a_record_out_of_order(gpu_lib, d, bad, batch):
    names, lens, recs = td.case_order(bad)
    path = td.write_case(str(d / ("order%d.bam" % bad)), names, lens, recs, in_order=False)
    with pytest.raises(dm.DepthError) as want:
        tm.expected(path, [1, 2], window=100)
    for kw in (dict(window=100), dict(intervals=[(0, 5, 4000)])):
        with pytest.raises(host.NgsqError) as e:
            host.bam_depth_windows(path, str(d / "o.txt"), batch_records=batch, thresholds=[1, 2], lib=gpu_lib, **kw)
        assert e.value.code == ffi.ERR_UNSORTED and e.value.message == str(want.value)
        assert f"record {bad} (0-based) is out of coordinate order" in e.value.message


# ---- the command line -------------------------------------------------------------------------------------------------------------
def test_command_line_file_stdout_bed_and_closed_pipe(gpu_lib, ngs, d, query_file):
    want = tm.expected(query_file, [1, 2, 3], window=100)[0]
    out = str(d / "cli.txt")
    r = subprocess.run([ngs, "depth", "--by", "100", "--thresholds", "1,2,3", "-o", out, query_file], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    same(open(out, "rb").read(), want)
    r = subprocess.run([ngs, "-q", "depth", "--thresholds", "9,8", "--by", "+100", "--thresholds", "+1,2,+3", query_file], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr                                   # given twice: the last one holds
    same(r.stdout, want)
    r = subprocess.run([ngs, "depth", "--by", "1000", "--thresholds", "1,2147483647", query_file, "q1:4500-5500"], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == b"q1\t4499\t5000\t1.00\t501\t0\nq1\t5000\t5500\t1.00\t500\t0\n", r.stderr
    bed = str(d / "cli.bed")
    with open(bed, "wb") as f:
        f.write(b"q3\t4000\t9000\nq1\t4000\t6000\nq2\t5\t6\n")
    iv = [(2, 4000, 5000), (0, 4000, 6000), (1, 5, 6)]
    want_bed, info = tm.expected(query_file, [1, 2], intervals=iv)
    r = subprocess.run([ngs, "depth", "-v", "--by", bed, "--thresholds", "1,2", query_file], capture_output=True, timeout=120)
    assert r.returncode == 0 and b"format passes" in r.stderr, r.stderr
    assert (", covered %d %d," % tuple(info["covered"])).encode() in r.stderr, r.stderr
    same(r.stdout, want_bed)
    r = subprocess.run([ngs, "depth", "-v", "--by", bed, query_file], capture_output=True, timeout=120)
    assert r.returncode == 0 and b"covered" not in r.stderr                # the -v line of a call without thresholds is as it was
    r = subprocess.run([ngs, "depth", "--by", "100", "--thresholds", "1", "-o", "/dev/full", query_file], capture_output=True, timeout=120)
    assert r.returncode == 1 and b"Error: writing depth to stream: No space left on device (os error 28)" in r.stderr
    p = subprocess.Popen([ngs, "depth", "--by", "1", "--thresholds", "1,2,3,4,5,6,7,8", query_file], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    p.stdout.close()                                                    # the reader goes away: the write's error, not a signal
    err = p.stderr.read()
    assert p.wait(timeout=120) == 1 and b"Error: writing depth to stream: Broken pipe (os error 32)" in err


# ---- random files -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_random_files(gpu_lib, d, seed):
    names, lens, hb = td.case_random(seed)
    path = str(d / ("random%d.bam" % seed))
    bamio.write_bam(path, hb, names, lens, with_index=False)
    rng = np.random.default_rng(2000 + seed)
    thresholds = sorted(set(int(x) for x in rng.integers(1, 12, size=int(rng.integers(1, 9)))))
    check(gpu_lib, path, d, thresholds, window=int(rng.integers(1, 5001)), tile_positions=1, exclude_flags=int(rng.choice([dm.EXCLUDE_FLAGS, 0])))
    iv = []
    for _ in range(int(rng.integers(1, 301))):
        r = int(rng.integers(0, len(lens)))
        s = int(rng.integers(0, lens[r]))
        iv.append((r, s, int(rng.integers(s + 1, lens[r] + 1))))
    check(gpu_lib, path, d, thresholds, intervals=iv, tile_positions=int(rng.choice([1, 1025])), batch_records=int(rng.choice([63, 64, 65, 257])),
          min_mapq=int(rng.choice([0, 4])))
