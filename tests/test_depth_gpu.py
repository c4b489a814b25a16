"""`ngs depth <BAM> [QUERY]` on the GPU: the bytes the device writes equal the test-side model's
(tests/depth_model.py) and the report's counts the model's, on the inputs tests/test_depth.py builds and holds to their edges:
the smallest files, sequences of 63 / 64 / 65 and tile - 1 / tile / tile + 1 positions, depth changes at both sides of a tile's
edge, a run over three tiles, records at 0, at, over and behind the end, at tile sizes 1, T, T + 1 and the default; every
filtered flag bit and the mapq minimum; piles through 10, 100 and 1000; coordinates through every power of ten; batch sizes
1, 7, 64, 65 and the default; the 195-sequence header with empty sequences around covered ones; regions through the index; a
record out of order in the first batch and across a batch boundary; the command line into a file, a pipe and a full device; and
twelve random files."""
import os
import subprocess

import numpy as np
import pytest

from ngs_amd import build, ffi, host
from tests import bamio
from tests import depth_model as dm
from tests import test_depth as td
from tests.test_view import indexed_copy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


@pytest.fixture(scope="module")
def d(tmp_path_factory):
    return tmp_path_factory.mktemp("depth")


def same(got: bytes, want: bytes):
    if got != want:
        k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"{len(got)} bytes against {len(want)}, first difference at {k}: {got[max(0, k - 60):k + 60]!r} against "
                             f"{want[max(0, k - 60):k + 60]!r}")


def check(lib, path, d, query=None, **kw):
    """One call against the model: the bytes, and the report's counts."""
    out = str(d / "o.bedgraph")
    rep = host.bam_depth(path, out, query=query, lib=lib, **kw)
    got = open(out, "rb").read()
    want, info = dm.expected(path, query, kw.get("exclude_flags", dm.EXCLUDE_FLAGS), kw.get("min_mapq", 0))
    same(got, want)
    assert rep["text_bytes"] == len(got) and rep["runs"] == info["runs"] == got.count(b"\n")
    assert rep["records_counted"] == info["records_counted"] and rep["sequences"] == info["sequences"]
    if info["records_scanned"] is not None:
        assert rep["records_scanned"] == info["records_scanned"] and rep["ranges"] == 0
    return got, rep


def tile_sizes():
    T = td.tile()
    return [1, T, T + 1, 0]


# ---- the smallest files, lengths around a wave and a tile, tile edges -------------------------------------------------------
@pytest.mark.parametrize("name", ["no_record", "one_record", "L1"])
def test_smallest_files(gpu_lib, d, name):
    names, lens, recs = td.case_small()[name]
    path = td.write_case(str(d / (name + ".bam")), names, lens, recs)
    for t in (1, 0):
        got, rep = check(gpu_lib, path, d, tile_positions=t)
    if name == "no_record":
        assert got == b"a\t0\t1000\t0\nb\t0\t1\t0\n" and rep["tiles"] == 0 and rep["batches"] == 0
    if name == "L1":
        assert got == b"a\t0\t1\t1\nb\t0\t1\t2\nc\t0\t1\t0\n"


@pytest.fixture(scope="module")
def shape_files(d):
    out = {}
    for name, case in (("lengths", td.case_lengths), ("tiles", td.case_tiles), ("pow10", td.case_pow10)):
        names, lens, recs = case()
        out[name] = (td.write_case(str(d / (name + ".bam")), names, lens, recs), lens)
    return out


@pytest.mark.parametrize("which", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["lengths", "tiles", "pow10"])
def test_lengths_and_tile_edges_at_every_tile_size(gpu_lib, d, shape_files, name, which):
    path, lens = shape_files[name]
    t = tile_sizes()[which]
    got, rep = check(gpu_lib, path, d, tile_positions=t)
    eff = host.depth_tile_positions(t, lib=gpu_lib)
    assert rep["tiles"] == sum(-(-L // eff) for L in lens)       # every sequence of these files has records
    if name == "tiles":
        T = td.tile()
        assert b"t\t%d\t%d\t1\n" % (2 * T - 10, 3 * T + 20) in got  # the run over three tiles is one line


def test_piles_through_ten_hundred_thousand(gpu_lib, d):
    names, lens, recs = td.case_piles()
    path = td.write_case(str(d / "piles.bam"), names, lens, recs)
    got, _ = check(gpu_lib, path, d, tile_positions=1)
    assert b"\t1000\n" in got and b"\t999\n" in got and b"\t10\n" in got
    check(gpu_lib, path, d, batch_records=64)


# ---- the filters ------------------------------------------------------------------------------------------------------------
def test_flag_bits_and_mapq(gpu_lib, d):
    names, lens, recs = td.case_filters()
    path = td.write_case(str(d / "filters.bam"), names, lens, recs)
    check(gpu_lib, path, d)
    for bits in (0, 4, 256, 512, 1024, 65535):
        check(gpu_lib, path, d, exclude_flags=bits)
    for m in (1, 10, 11, 255):
        check(gpu_lib, path, d, exclude_flags=0, min_mapq=m)
    check(gpu_lib, path, d, min_mapq=10)


def test_long_cigar_fixture(gpu_lib, tmp_path):
    path = indexed_copy("hand_longcigar.bam", tmp_path)
    got, _ = check(gpu_lib, path, tmp_path)
    assert got.startswith(b"chr1\t0\t1000\t0\nchr1\t1000\t1035\t1\n")
    for q in ("chr1", "chr1:1035-2000", "chr1:1036-2000", "chr1:1-1000", "chr1:1001-1001", "chr2"):
        check(gpu_lib, path, tmp_path, q)


# ---- batches and sequences --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 7, 64, 65, 0])
def test_batch_sizes(gpu_lib, d, batch):
    names, lens, recs = td.case_batches()
    path = str(d / "batches.bam")
    if not os.path.exists(path):
        td.write_case(path, names, lens, recs)
    got, rep = check(gpu_lib, path, d, batch_records=batch, tile_positions=1)
    assert rep["batches"] >= (-(-len(recs) // batch) if batch else 1)
    assert b"b3\t0\t50\t0\n" in got


def test_genome_header_with_empty_sequences_around_covered_ones(gpu_lib, d):
    names, lens, recs = td.case_genome()
    path = td.write_case(str(d / "genome.bam"), names, lens, recs)
    got, rep = check(gpu_lib, path, d, batch_records=64)
    assert got.startswith(b"chr1\t0\t%d\t0\nchr2\t0\t" % lens[0]) and got.endswith(b"%s\t0\t%d\t0\n" % (names[-1].encode(), lens[-1]))
    assert rep["sequences"] == 195
    check(gpu_lib, path, d)


# ---- regions ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def query_file(d):
    names, lens, recs = td.case_query()
    return td.write_case(str(d / "query.bam"), names, lens, recs, block_payload=3000)


@pytest.mark.parametrize("query", td.QUERIES)
def test_regions(gpu_lib, d, query_file, query):
    got, rep = check(gpu_lib, query_file, d, query, batch_records=257)
    if query in ("q2", "q2:100-200", "q1:300001"):
        assert rep["records_scanned"] == 0 and rep["tiles"] == 0
    check(gpu_lib, query_file, d, query, tile_positions=1)


def test_one_walk_per_chunk_gives_the_same_bytes(gpu_lib, d, query_file):
    a, ra = check(gpu_lib, query_file, d, "q1:6000-200000", coalesce_gap=1, batch_records=500)
    b, rb = check(gpu_lib, query_file, d, "q1:6000-200000")
    assert a == b and ra["ranges"] >= 2 and rb["ranges"] == 1


# ---- order ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad,batch", td.ORDER_CASES)
def test_a_record_out_of_order(gpu_lib, d, bad, batch):
    """Record `bad` starts in front of the record before it: in the first batch, and as the first record of a later batch, where
    only the carry across the batch boundary can tell."""
    names, lens, recs = td.case_order(bad)
    path = td.write_case(str(d / ("order%d.bam" % bad)), names, lens, recs, in_order=False)
    with pytest.raises(dm.DepthError) as want:
        dm.expected(path)
    with pytest.raises(host.NgsqError) as e:
        host.bam_depth(path, str(d / "o.bedgraph"), batch_records=batch, lib=gpu_lib)
    assert e.value.code == ffi.ERR_UNSORTED and e.value.message == str(want.value)
    assert f"record {bad} (0-based) is out of coordinate order" in e.value.message


def test_a_placed_record_behind_an_unplaced_one(gpu_lib, d):
    recs = [td.rec(0, 100, "30M"), td.rec(-1, -1, "*", flag=4), td.rec(0, 200, "30M")]
    path = td.write_case(str(d / "unplaced.bam"), ["o"], [5000], recs, in_order=False)
    with pytest.raises(host.NgsqError) as e:
        host.bam_depth(path, str(d / "o.bedgraph"), lib=gpu_lib)
    assert e.value.code == ffi.ERR_UNSORTED and "record 2 (0-based)" in e.value.message


# ---- the command line -------------------------------------------------------------------------------------------------------
def test_command_line_file_stdout_pipe_and_full_device(gpu_lib, ngs, d, query_file):
    want = dm.expected(query_file)[0]
    out = str(d / "cli.bedgraph")
    r = subprocess.run([ngs, "depth", "-o", out, query_file], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    same(open(out, "rb").read(), want)
    r = subprocess.run([ngs, "-q", "depth", query_file], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    same(r.stdout, want)
    r = subprocess.run([ngs, "depth", "--exclude-flags", "0", "--min-mapq", "61", query_file, "q1:4500-5500"], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == b"q1\t4499\t5500\t0\n", r.stderr
    r = subprocess.run([ngs, "depth", "-o", "/dev/full", query_file], capture_output=True, timeout=120)
    assert r.returncode == 1 and b"Error: writing depth to stream: No space left on device (os error 28)" in r.stderr
    p = subprocess.Popen([ngs, "depth", query_file], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    p.stdout.close()                                                    # the reader goes away: the write's error, not a signal
    err = p.stderr.read()
    assert p.wait(timeout=120) == 1 and b"Error: writing depth to stream: Broken pipe (os error 32)" in err


# ---- random files -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_random_files(gpu_lib, d, seed):
    names, lens, hb = td.case_random(seed)
    path = str(d / ("random%d.bam" % seed))
    bamio.write_bam(path, hb, names, lens, with_index=False)
    rng = np.random.default_rng(seed)
    check(gpu_lib, path, d, exclude_flags=0)
    check(gpu_lib, path, d, batch_records=int(rng.choice([1, 7, 63, 64, 65, 257])) if hb.n < 400 else int(rng.choice([63, 64, 65, 257])),
          tile_positions=int(rng.choice([1, td.tile() + 1])), exclude_flags=int(rng.choice([dm.EXCLUDE_FLAGS, 0, 0x904])),
          min_mapq=int(rng.choice([0, 4, 60])))
