"""`ngs view <BAM> [QUERY]` on the GPU: what the device selects and formats equals the test-side model
(tests/view_model.py) byte for byte -- on the hand-assembled files in all three modes, at both sides of every edge of an
interval (a record ending at S or S-1, starting at E or E+1, reaching the region only by a D or N, a zero-span record at S,
the 16 kb window boundary, a region past the sequence, a sequence without records), on files of 1 / 63 / 64 / 65 / 129 records
(a wave takes 64), through two chunks far apart in the file walked as one range or as two, and on a randomised slice of files
and regions; the range ingest hands out the records the model says; a record without SAM text ends the view only when the
region selects it; a full device gives the write's message."""
import ctypes as C
import os

import numpy as np
import pytest

from ngs_amd import build, ffi, host
from tests import bamio
from tests import view_model as vm
from tests.test_convert_gpu import assert_same
from tests.test_index import LENS, NAMES, index_sorted_batch
from tests.test_view import indexed_copy, run, write_indexed
from tests.util import batch_from_records

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def view(lib, path, out, query=None, mode="full", **kw):
    rep = host.bam_view(path, out, query=query, mode=mode, lib=lib, **kw)
    return open(out, "rb").read(), rep


def check(lib, path, out, query=None, mode="records-only", **kw):
    """One view against the model, the report against the bytes."""
    got, rep = view(lib, path, out, query, mode, **kw)
    want = vm.expected_view(path, query, mode)
    assert_same(got, want)
    assert rep["header_bytes"] + rep["text_bytes"] == len(got)
    assert rep["records_written"] == (0 if mode == "header-only" else want.count(b"\n") - (vm.header_bytes(path).count(b"\n") if mode == "full" else 0))
    return got, rep


def rec(ref, pos, cigar="50M", name=None, qual=30, flag=0):
    """A record dict for batch_from_records: the read as long as its CIGAR says (one base for an empty CIGAR)."""
    from tests.util import parse_cigar
    ops = parse_cigar(cigar)
    l = sum(c >> 4 for c in ops if (c & 15) in (0, 1, 4, 7, 8)) if ops else 1
    return dict(flag=flag, mapq=60, ref_id=ref, pos=pos, mate_ref_id=-1, tlen=0, cigar=cigar, seq="ACGT" * (l // 4) + "ACGT"[:l % 4],
                qual=[qual] * l, name=name)


def write_records(path, recs, **kw):
    """recs in any order -> a coordinate-sorted file with the model's index; the records' names are "r<k>" unless given."""
    order = sorted(range(len(recs)), key=lambda k: ((recs[k]["ref_id"] < 0 or recs[k]["pos"] < 0), recs[k]["ref_id"], recs[k]["pos"], k))
    recs = [recs[k] for k in order]
    names = [(r["name"] or "r%d" % k).encode() for k, r in enumerate(recs)]
    return write_indexed(path, batch_from_records(recs), names=names, **kw), recs


def filler(rng, n, refs=(0, 2)):
    """Short random records on the given sequences, a few of them without a span or with a D / N."""
    out = []
    for _ in range(n):
        r = int(rng.choice(refs))
        cigar = str(rng.choice(["50M", "20S30M", "10M5D20M", "10M300N10M", "*", "25M2I23M", "5H40M5H", "30M"]))
        out.append(rec(r, int(rng.integers(0, LENS[r] - 100)), cigar, qual=int(rng.integers(0, 94))))
    return out


# ---- the hand files ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,queries", [
    ("hand_spec.bam", [None, "chr1", "chr2", "chr1:149-300", "chr1:150-300", "chr1:331-331", "chr1:440-458", "chr1:459-5001", "chr1:5041",
                       "chr1:100001", "chr2:130-200"]),
    ("hand_longcigar.bam", [None, "chr1", "chr1:1035-2000", "chr1:1036-2000", "chr1:1-1000", "chr2"])])
def test_hand_files_every_mode(gpu_lib, tmp_path, name, queries):
    path = indexed_copy(name, tmp_path)
    for q in queries:
        for mode in vm.MODES:
            got, rep = check(gpu_lib, path, str(tmp_path / "o.sam"), q, mode)
            if mode == "header-only":
                assert got == vm.header_bytes(path)
    if name == "hand_spec.bam":
        assert view(gpu_lib, path, str(tmp_path / "o.sam"))[0] == open(os.path.join(GOLDEN, "hand_spec.sam"), "rb").read()


def test_committed_index_without_bins_selects_nothing(gpu_lib, tmp_path):
    path = os.path.join(GOLDEN, "hand_spec.bam")
    got, rep = check(gpu_lib, path, str(tmp_path / "o.sam"), "chr1", "full")
    assert got == vm.header_bytes(path) and rep["chunks"] == 0 and rep["ranges"] == 0 and rep["records_scanned"] == 0


# ---- both sides of every edge -----------------------------------------------------------------------------------------------
S, E = 20000, 20100
EDGE_RECORDS = [
    rec(0, S - 50, "50M", "ends_at_S"), rec(0, S - 51, "50M", "ends_at_S-1"),
    rec(0, E - 1, "50M", "starts_at_E"), rec(0, E, "50M", "starts_at_E+1"),
    rec(0, 19000, "10M1500N10M", "over_by_N"), rec(0, 19000, "10M900N10M", "short_of_by_N"),
    rec(0, 19500, "5M2000D5M", "over_by_D"), rec(0, 19500, "5M400D5M", "short_of_by_D"),
    rec(0, S - 1, "*", "zero_span_at_S"), rec(0, S - 2, "*", "zero_span_at_S-1"), rec(0, S - 1, "10S", "clip_only_at_S"),
    rec(0, E - 1, "3I", "zero_span_at_E"), rec(0, E, "3I", "zero_span_at_E+1"),
    rec(0, 16382, "1M", "p16383"), rec(0, 16382, "2M", "p16383_16384"), rec(0, 16383, "1M", "p16384"), rec(0, 16384, "1M", "p16385"),
    rec(0, 16385, "1M", "p16386"), rec(0, 16383, "*", "z16384"), rec(0, 16384, "*", "z16385"),
    rec(2, 4990, "30M", "over_the_end"), rec(2, 5010, "30M", "past_the_end"),
    rec(-1, -1, "*", "unplaced", flag=4), rec(0, -1, "*", "no_position", flag=4),
]
EDGE_QUERIES = {
    f"chr1:{S}-{E}": (["ends_at_S", "starts_at_E", "over_by_N", "over_by_D", "zero_span_at_S", "clip_only_at_S", "zero_span_at_E"],
                      ["ends_at_S-1", "starts_at_E+1", "short_of_by_N", "short_of_by_D", "zero_span_at_S-1", "zero_span_at_E+1"]),
    "chr1:16384-16384": (["p16383_16384", "p16384", "z16384"], ["p16383", "p16385", "z16385", "p16386"]),
    "chr1:16385-16385": (["p16385", "z16385"], ["p16383", "p16383_16384", "p16384", "z16384", "p16386"]),
    "chr1:16384-16385": (["p16383_16384", "p16384", "z16384", "p16385", "z16385"], ["p16383", "p16386"]),
    "chr3:5001-6000": (["over_the_end", "past_the_end"], []),          # a region past the sequence's end
    "chr3:5041": ([], ["over_the_end", "past_the_end"]),
    "chr3:5020-5020": (["over_the_end", "past_the_end"], []),
    "chr2": ([], []),                                                   # a sequence without records
    "chr2:1-70000": ([], []),
    "chr1": (["ends_at_S", "over_by_N", "zero_span_at_S", "p16386"], ["over_the_end", "unplaced", "no_position"]),
    "chr3": (["over_the_end", "past_the_end"], ["ends_at_S", "unplaced"]),
    "chr1:300001": ([], ["ends_at_S"]),
}


@pytest.fixture(scope="module")
def edge_file(tmp_path_factory):
    d = tmp_path_factory.mktemp("edges")
    recs = EDGE_RECORDS + filler(np.random.default_rng(41), 3000)
    path, _ = write_records(str(d / "e.bam"), recs, block_payload=3000)
    return path


@pytest.mark.parametrize("query", list(EDGE_QUERIES))
def test_interval_edges(gpu_lib, tmp_path, edge_file, query):
    inside, outside = EDGE_QUERIES[query]
    got, rep = check(gpu_lib, edge_file, str(tmp_path / "o.sam"), query, batch_records=257)
    names = {ln.split(b"\t")[0].decode() for ln in got.split(b"\n") if ln}
    assert not [n for n in inside if n not in names], query
    assert not [n for n in outside if n in names], query
    assert rep["batches"] >= rep["records_scanned"] // 257
    assert_same(view(gpu_lib, edge_file, str(tmp_path / "f.sam"), query, "full", batch_records=1000)[0], vm.expected_view(edge_file, query, "full"))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_lane_and_wave_edges(gpu_lib, tmp_path, n):
    """Files of n records, every second one inside the region: the kept count of a wave and of its last lanes."""
    recs = [rec(0, 1000 + 10 * k if k % 2 == 0 else 50000 + 10 * k, "30M") for k in range(n)]
    path, _ = write_records(str(tmp_path / "w.bam"), recs)
    for q in ("chr1:1000-3000", "chr1", "chr1:50000", "chr2"):
        _, rep = check(gpu_lib, path, str(tmp_path / "o.sam"), q)
    _, rep = check(gpu_lib, path, str(tmp_path / "o.sam"), "chr1:1000-3000")
    assert rep["records_written"] == (n + 1) // 2
    check(gpu_lib, path, str(tmp_path / "o.sam"), None, "full")


def test_two_distant_chunks_walked_as_one_range_or_two(gpu_lib, tmp_path):
    """A 50M40000N50M record at pos 1000 and 2000 short records behind it: the region chr1:40500-40600 is reached by the long
    record (a bin of its own, at the file's beginning) and by the short ones near it (hundreds of blocks further on)."""
    recs = [rec(0, 1000, "50M40000N50M", "long")] + [rec(0, 1001 + 29 * k, "30M") for k in range(2000)]
    path, _ = write_records(str(tmp_path / "d.bam"), recs, block_payload=2000)
    q = "chr1:40500-40600"
    chunks = host.bam_query_chunks(path, q, lib=gpu_lib)[3]
    assert len(chunks) >= 2 and (chunks[-1][0] >> 16) - (chunks[0][1] >> 16) > 5_000
    each, rep1 = check(gpu_lib, path, str(tmp_path / "a.sam"), q, coalesce_gap=1, batch_records=257)
    one, rep2 = check(gpu_lib, path, str(tmp_path / "b.sam"), q, coalesce_gap=1 << 62, batch_records=257)
    assert each == one and each.startswith(b"long\t")
    assert rep1["ranges"] == len(chunks) > 1 and rep2["ranges"] == 1
    assert rep1["records_scanned"] < rep2["records_scanned"]
    dflt, rep3 = check(gpu_lib, path, str(tmp_path / "c.sam"), q)
    assert dflt == one and rep3["chunks"] == len(chunks)


def test_neighbouring_chunks_in_one_block_are_not_written_twice(gpu_lib, tmp_path):
    """coalesce_gap 1 walks every merged chunk on its own; a walk hands out records behind its end, to the end of their block,
    and those are the next walk's: each record is written once."""
    recs = [rec(0, 100 + 3 * k, "30M" if k % 7 else "10M20000N10M") for k in range(600)]
    path, _ = write_records(str(tmp_path / "n.bam"), recs, block_payload=60000)
    for q in ("chr1:200-900", "chr1:20100-20200", "chr1"):
        each, rep = check(gpu_lib, path, str(tmp_path / "a.sam"), q, coalesce_gap=1)
        assert each == view(gpu_lib, path, str(tmp_path / "b.sam"), q, "records-only")[0]
    assert rep["ranges"] == rep["chunks"]


# ---- the range ingest ---------------------------------------------------------------------------------------------------------
def test_range_begin_hands_out_the_models_records(gpu_lib, tmp_path):
    hb = index_sorted_batch(51, 6000, max_len=150)
    path = write_indexed(str(tmp_path / "r.bam"), hb, block_payload=5000)
    offs = np.array(vm.record_offsets(path), dtype=np.uint64)
    size = os.path.getsize(path)
    mid = [k for k in range(len(offs)) if int(offs[k]) & 0xFFFF]            # records that start inside a block
    assert len(mid) > 100
    ctx = host.QcContext(LENS, [1] * len(LENS), lib=gpu_lib)
    h = C.c_void_p()
    assert gpu_lib.ngsq_bam_open(path.encode(), 1, C.byref(h)) == 0
    try:
        def walk(begin, end):
            assert gpu_lib.ngsq_bam_range_begin(h, ctx._ctx, begin, end) == 0, gpu_lib.ngsq_bam_last_error()
            ids = []
            while True:
                b = ffi.Batch()
                assert gpu_lib.ngsq_bam_next_batch_device(h, ctx._ctx, 257, C.byref(b)) == 0, gpu_lib.ngsq_bam_last_error()
                if b.n_records == 0:
                    break
                assert b.first_record_index == sum(len(x) for x in ids)        # numbered within the range
                a = np.zeros(b.n_records, dtype=np.uint64)
                assert gpu_lib.ngsq_memcpy_d2h(ctx._ctx, a.ctypes.data, b.record_id, a.nbytes) == 0
                ids.append(a)
            return np.concatenate(ids) if ids else np.zeros(0, np.uint64)

        def want(i, end):
            """From record i on, the records that start in the blocks up to the block of `end` (in front of it when end is its first byte)."""
            last_block = (end >> 16) - (0 if end & 0xFFFF else 1)
            return offs[i:][(offs[i:] >> np.uint64(16)) <= np.uint64(last_block)]

        i, j = mid[40], mid[-60]
        cases = [(i, int(offs[j])),                                  # begins and ends inside blocks, hundreds of blocks apart
                 (i, int(offs[i]) + 1),                              # ends in the block it begins in
                 (mid[5], int(offs[mid[300]]) >> 16 << 16),           # ends on a block's first byte: in front of that block
                 (mid[-20], int(offs[-1])),                          # ends in the file's last block with data
                 (mid[-20], size << 16),                             # ... and at the end of the file
                 (0, int(offs[mid[30]]))]                            # from the file's first record
        for k, end in cases:
            got = walk(int(offs[k]) if k else 0, end)
            w = want(k, end)
            assert len(w) and np.array_equal(got, w), (k, hex(end), len(got), len(w))
        info = ffi.ShardInfo()
        assert gpu_lib.ngsq_bam_shard_end(h, C.byref(info)) == 0 and info.n_records == len(want(0, int(offs[mid[30]])))
        assert gpu_lib.ngsq_bam_range_begin(h, ctx._ctx, int(offs[j]), int(offs[i])) != 0          # ends in front of its beginning
        assert gpu_lib.ngsq_bam_range_begin(h, ctx._ctx, (size + 5) << 16, (size + 9) << 16) != 0   # behind the file
    finally:
        gpu_lib.ngsq_bam_close(h)
        ctx.close()


# ---- a randomised slice -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_random_files_and_regions(gpu_lib, tmp_path, seed):
    rng = np.random.default_rng(600 + seed)
    for f in range(5):
        n = int(rng.choice([40, 300, 1500, 4000]))
        hb = index_sorted_batch(rng, n, max_len=int(rng.choice([60, 200])))
        path = write_indexed(str(tmp_path / f"r{f}.bam"), hb, block_payload=int(rng.choice([700, 5000, 60000])),
                             aux=[bamio.aligner_aux(rng, int(hb.cols["l_seq"][i])) for i in range(hb.n)])
        for _ in range(3):
            r = int(rng.integers(0, 3))
            s = int(rng.integers(1, LENS[r] + 200))
            e = s + int(rng.choice([0, 1, 300, 16384, 100000]))
            q = f"{NAMES[r]}:{s}-{e}" if rng.random() < 0.8 else NAMES[r] if rng.random() < 0.5 else f"{NAMES[r]}:{s}"
            check(gpu_lib, path, str(tmp_path / "o.sam"), q, str(rng.choice(["full", "records-only"])),
                  batch_records=int(rng.choice([257, 1000, 0])), coalesce_gap=int(rng.choice([0, 1, 20000, 1 << 62])))


# ---- the command line ---------------------------------------------------------------------------------------------------------
def test_command_line_prints_what_the_model_prints(gpu_lib, ngs, edge_file):
    for args, q, mode in ((["chr3:1000-2000"], "chr3:1000-2000", "full"), (["-m", "records-only", f"chr1:{S}-{E}"], f"chr1:{S}-{E}", "records-only"),
                          ([], None, "full"), (["--mode", "records-only"], None, "records-only")):
        r = run(ngs, "view", edge_file, *args)
        assert r.returncode == 0, r.stderr
        assert_same(r.stdout, vm.expected_view(edge_file, q, mode))
    for args, context in ((["chrX"], "querying BAM file: "), ([""], "parsing query: ")):
        r = run(ngs, "view", edge_file, *args)
        assert r.returncode == 1 and r.stdout == b"" and b"Error: " + context.encode() in r.stderr


def test_command_line_without_an_index(gpu_lib, ngs, tmp_path):
    """No .bai is needed without a query; with one, its absence is the reading error and nothing is written."""
    path, _ = write_records(str(tmp_path / "x.bam"), filler(np.random.default_rng(43), 200))
    os.remove(path + ".bai")
    r = run(ngs, "view", path)
    assert r.returncode == 0 and r.stdout == vm.expected_view(path)
    r = run(ngs, "view", path, "chr1")
    assert r.returncode == 1 and r.stdout == b"" and b"Error: reading BAM index: " in r.stderr
    open(path + ".bai", "wb").write(b"BAI\1\3\0\0")
    r = run(ngs, "view", path, "chr1")
    assert r.returncode == 1 and r.stdout == b"" and b"Error: reading BAM index: " in r.stderr


def test_a_reader_that_goes_away_ends_the_command_with_the_write_error(gpu_lib, ngs, tmp_path):
    """`ngs view x.bam | head`: SIGPIPE is ignored, the failed write is the command's error."""
    import subprocess
    path, _ = write_records(str(tmp_path / "p.bam"), filler(np.random.default_rng(44), 20000))
    rd, wr = os.pipe()
    os.close(rd)
    r = subprocess.run([ngs, "view", "-m", "records-only", path], stdout=wr, stderr=subprocess.PIPE, timeout=120)
    os.close(wr)
    assert r.returncode == 1 and b"Error: writing record to stream: Broken pipe (os error 32)" in r.stderr


# ---- records without SAM text, writes that fail ---------------------------------------------------------------------------
def test_a_bad_record_matters_only_inside_the_region(gpu_lib, tmp_path):
    recs = filler(np.random.default_rng(45), 1500, refs=(0,)) + [rec(0, 150000, "50M", "bad", qual=94)]
    path, recs = write_records(str(tmp_path / "b.bam"), recs, block_payload=3000)
    index = [k for k, r in enumerate(recs) if r["name"] == "bad"][0]
    assert 100 < index < 1400
    for q in ("chr1:150001-150050", "chr1:150050-160000", "chr1", None):
        with pytest.raises(vm.ViewError, match=f"writing record to stream: record {index}: quality score above 93"):
            vm.expected_view(path, q, "records-only")
        for gap in (0, 1):
            with pytest.raises(host.NgsqError) as e:
                view(gpu_lib, path, str(tmp_path / "o.sam"), q, "records-only", batch_records=257, coalesce_gap=gap)
            assert f"writing record to stream: record {index}: quality score above 93" in str(e.value), q
    for q in ("chr1:1-150000", "chr1:150051", "chr1:150051-150051", "chr3"):        # the record is not selected: not examined
        check(gpu_lib, path, str(tmp_path / "o.sam"), q, batch_records=257)


def test_a_full_device_gives_the_write_message(gpu_lib, edge_file):
    with pytest.raises(host.NgsqError) as e:
        host.bam_view(edge_file, "/dev/full", query="chr1", mode="records-only", lib=gpu_lib)
    assert "writing record to stream: No space left on device (os error 28)" in str(e.value)
    with pytest.raises(host.NgsqError) as e:
        host.bam_view(edge_file, "/dev/full", mode="records-only", lib=gpu_lib)
    assert "writing record to stream: No space left on device (os error 28)" in str(e.value)
    with pytest.raises(host.NgsqError) as e:
        host.bam_view(edge_file, "/dev/full", query="chr1", mode="full", lib=gpu_lib)
    assert "writing BAM header to stream: No space left on device (os error 28)" in str(e.value)


def test_convert_and_view_without_a_query_write_the_same_records(gpu_lib, tmp_path, edge_file):
    """The run the two commands share: the whole file through `ngs view` is `ngs convert`'s text."""
    host.bam_to_sam(edge_file, str(tmp_path / "c.sam"), lib=gpu_lib, batch_records=700)
    got, rep = view(gpu_lib, edge_file, str(tmp_path / "v.sam"), batch_records=700)
    assert got == open(tmp_path / "c.sam", "rb").read()
    assert rep["ranges"] == 0 and rep["chunks"] == 0 and rep["records_written"] == rep["records_scanned"] == got.count(b"\n") - 4
