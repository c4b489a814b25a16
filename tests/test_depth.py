"""`ngs depth <BAM> [QUERY]` without a GPU: the test-side model (tests/depth_model.py) on a case worked
by hand, on the long-CIGAR hand file against the depths tests/test_hand_bam.py holds, and against the oracle's Coverage depth
histogram on random sorted records; every input of tests/test_depth_gpu.py held to reach the edge it is named for; and the command
line as far as it answers without a GPU: the help, every refusal, the unsorted header, a query without an index, a query that does
not parse or names no sequence.  Nothing is written in any of them."""
import os
import subprocess

import numpy as np
import pytest

from ngs_amd import build, ffi, host
from ngs_amd.genome_shape import grch38_no_alt
from tests import bai_model as bm
from tests import bamio
from tests import depth_model as dm
from tests import view_model as vm
from tests.test_hand_bam import LONG_EXPECT
from tests.test_index import index_sorted_batch
from tests.util import batch_from_records, parse_cigar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def run(ngs, *args):
    return subprocess.run([ngs, *args], capture_output=True, timeout=120)


def rec(ref, pos, cigar="50M", flag=0, mapq=60):
    """A record dict for batch_from_records: the read as long as its CIGAR says (one base for an empty CIGAR)."""
    ops = parse_cigar(cigar)
    l = sum(c >> 4 for c in ops if (c & 15) in (0, 1, 4, 7, 8)) if ops else 1
    return dict(flag=flag, mapq=mapq, ref_id=ref, pos=pos, mate_ref_id=-1, tlen=0, cigar=cigar, seq="ACGT" * (l // 4) + "ACGT"[:l % 4], qual=[30] * l)


def sort_key(r):
    return ((r["ref_id"] < 0 or r["pos"] < 0), r["ref_id"], r["pos"])


def write_case(path, names, lens, recs, in_order=True, index=True, **kw):
    """recs (sorted here unless in_order is False) as a BAM file whose header says SO:coordinate, the model's index beside it."""
    if in_order:
        recs = sorted(recs, key=sort_key)
    kw.setdefault("with_index", False)
    bamio.write_bam(path, batch_from_records(recs), names, lens, **kw)
    if index and in_order:
        with open(path + ".bai", "wb") as f:
            f.write(bm.expected_bai(path))
    return path


def depth_of(path, ref, **kw):
    """The model's depth of every position of sequence ref."""
    names, lens, recs, _ = dm.read(path)
    return dm.depths([r for r in recs if dm.counts(r, **kw)], ref, 0, lens[ref])


# ---- the inputs of the GPU tests: name -> (names, lens, records) ---------------------------------------------------------
def tile():
    return host.depth_tile_positions(1)


def case_small():
    """No record; one record; L = 1."""
    return {
        "no_record": (["a", "b"], [1000, 1], []),
        "one_record": (["a"], [1000], [rec(0, 10, "5M")]),
        "L1": (["a", "b", "c"], [1, 1, 1], [rec(0, 0, "1M"), rec(1, 0, "5M"), rec(1, 0, "1M")]),
    }


def case_lengths():
    """Sequences of 63, 64, 65 and tile - 1, tile, tile + 1 positions; in each a record at position 0, one ending exactly at L,
    one reaching beyond L and one starting at L."""
    T = tile()
    lens = [63, 64, 65, T - 1, T, T + 1]
    recs = []
    for r, L in enumerate(lens):
        recs += [rec(r, 0, "7M"), rec(r, L - 5, "5M"), rec(r, L - 3, "10M"), rec(r, L, "4M"), rec(r, L // 2, "3M2D3M")]
    return ["s%d" % L for L in lens], lens, recs


def case_tiles():
    """One sequence of 5 T + 7 positions: the depth changes exactly at T - 1, T and T + 1, one run covers the end of tile 1, all of
    tile 2 and the start of tile 3 (tile 2 has no change in it), records at position 0, ending at L, reaching beyond L, starting at L."""
    T = tile()
    L = 5 * T + 7
    recs = [rec(0, 0, "3M"), rec(0, 0, "9M"),
            rec(0, T - 1, "2M"), rec(0, T, "1M"), rec(0, T - 20, "21M"), rec(0, T - 30, "31M"), rec(0, T + 1, "40M"),
            rec(0, 2 * T - 10, "%dM" % (T + 30)),                        # the run [2T - 10, 3T + 20)
            rec(0, 4 * T - 1, "2M"), rec(0, 4 * T, "%dM" % (T + 7)), rec(0, L - 4, "4M"), rec(0, L - 2, "50M"), rec(0, L, "5M")]
    return ["t"], [L], recs


def case_filters():
    """Every filtered flag bit alone, the other bits alone, a no-CIGAR record, and mapq 9, 10 and 255 around a minimum of 10."""
    recs = [rec(0, 100 + 10 * k, "30M", flag=1 << k) for k in range(12)]
    recs += [rec(0, 300, "*"), rec(0, 305, "10S"), rec(0, 310, "20M", mapq=9), rec(0, 315, "20M", mapq=10), rec(0, 320, "20M", mapq=255),
             rec(0, 325, "20M", mapq=0), rec(-1, -1, "*", flag=4), rec(0, -1, "*", flag=4)]
    return ["f"], [500], recs


def case_piles():
    """The depth climbs one by one from 1 to 1000 and down again: every crossing 9 -> 10, 99 -> 100, 999 -> 1000 in both directions."""
    return ["p"], [4000], [rec(0, 500 + k, "1000M") for k in range(1000)]


def case_pow10():
    """Run starts and ends at 10^k - 1, 10^k and 10^k + 1 for k = 1 .. 5."""
    recs = []
    for k in range(1, 6):
        recs += [rec(0, 10 ** k - 1, "1M"), rec(0, 10 ** k, "1M"), rec(0, 10 ** k, "1M")]
    return ["w"], [100_010], recs


def case_batches():
    """Six sequences, the second and fifth with two records each, the others with a hundred or more: at 7 records a batch a batch
    holds several sequences, and the others span several batches at every size."""
    rng = np.random.default_rng(7)
    lens = [9000, 800, 7000, 50, 600, 12000]
    recs = []
    for r, n in enumerate([150, 2, 120, 0, 2, 260]):
        recs += [rec(r, int(rng.integers(0, lens[r])), str(rng.choice(["50M", "20M5D20M", "*", "10M300N10M", "30M"])), flag=int(rng.choice([0, 16, 1024])))
                 for _ in range(n)]
    return ["b%d" % r for r in range(6)], lens, recs


def case_genome():
    """The 195-sequence header (chromosomes scaled down by 4096, contigs at their size): records on chr2, chr3, chrM and every
    seventh contig; chr1 in front, chr4 .. chrY between and the last contigs behind them are empty."""
    names, lens, _ = grch38_no_alt(4096)
    rng = np.random.default_rng(11)
    live = [1, 2, names.index("chrM")] + [r for r in range(26, len(names) - 3) if r % 7 == 0]
    recs = [rec(r, int(rng.integers(0, lens[r])), "100M") for r in live for _ in range(12)]
    return names, lens, recs


def case_query():
    """Three sequences for the region tests: a long run on q1 around 5000, a record that starts in front of 3000 and reaches in,
    nothing on q2, records near the end of q3."""
    rng = np.random.default_rng(13)
    recs = [rec(0, 4000, "2000M"), rec(0, 2990, "20M"), rec(0, 2000, "10M900N10M"), rec(2, 4990, "30M"), rec(2, 4000, "100M")]
    recs += [rec(0, int(rng.integers(6000, 290000)), "80M") for _ in range(3000)]
    return ["q1", "q2", "q3"], [300_000, 70_000, 5_000], recs


QUERIES = ["q1", "q3", "q1:4500-5500", "q1:3000-3005", "q1:2905-2915", "q3:4000-9000", "q3:4995", "q2", "q2:100-200", "q1:290500", "q1:300001",
           "q1:6000-200000"]


def case_order(bad):
    """Two hundred records in order but record `bad`, which starts in front of the record before it."""
    recs = [rec(0, 100 + 10 * k, "30M") for k in range(200)]
    recs[bad] = rec(0, 100 + 10 * (bad - 1) - 5, "30M")
    return ["o"], [5000], recs


ORDER_CASES = [(3, 0), (64, 64), (130, 64)]   # (the record out of order, records per batch): in batch 0, first of a batch, inside a later one


def case_random(seed):
    rng = np.random.default_rng(100 + seed)
    lens = [int(rng.integers(1, 100_000)), int(rng.integers(1, 3000)), int(rng.integers(1, 70)), int(rng.integers(1, 40_000))]
    hb = index_sorted_batch(rng, int(rng.integers(1, 3000)), lens=lens, weird=True, max_len=150)
    return ["r%d" % k for k in range(4)], lens, hb


# ---- the model ------------------------------------------------------------------------------------------------------------
def test_model_on_a_case_worked_by_hand(tmp_path):
    """a (10 positions): 3M at 2 covers 2..4, 2M1D1M at 3 covers 3..6, 5M at 8 is clipped to 8..9:
           position 0 1 2 3 4 5 6 7 8 9
           depth    0 0 1 2 2 1 1 0 1 1
       b (5 positions): no record.
       c (8 positions): a duplicate 8M at 0 (counts only with --exclude-flags 0), 2M at 1 covers 1..2, a record without a CIGAR at 7
       covers nothing, a record of mapq 3 (1M at 4) counts unless --min-mapq is above 3."""
    path = write_case(str(tmp_path / "h.bam"), ["a", "b", "c"], [10, 5, 8],
                      [rec(0, 2, "3M"), rec(0, 3, "2M1D1M"), rec(0, 8, "5M"), rec(2, 0, "8M", flag=1024), rec(2, 1, "2M"), rec(2, 7, "*"),
                       rec(2, 4, "1M", mapq=3)])
    a = b"a\t0\t2\t0\na\t2\t3\t1\na\t3\t5\t2\na\t5\t7\t1\na\t7\t8\t0\na\t8\t10\t1\n"
    b = b"b\t0\t5\t0\n"
    got, info = dm.expected(path)
    assert got == a + b + b"c\t0\t1\t0\nc\t1\t3\t1\nc\t3\t4\t0\nc\t4\t5\t1\nc\t5\t8\t0\n"
    assert info == dict(records_scanned=7, records_counted=6, runs=12, sequences=3)
    got, info = dm.expected(path, exclude_flags=0)
    assert got == a + b + b"c\t0\t1\t1\nc\t1\t3\t2\nc\t3\t4\t1\nc\t4\t5\t2\nc\t5\t8\t1\n" and info["records_counted"] == 7
    got, info = dm.expected(path, min_mapq=4)
    assert got == a + b + b"c\t0\t1\t0\nc\t1\t3\t1\nc\t3\t8\t0\n" and info["records_counted"] == 5
    assert dm.expected(path, "a:3-8")[0] == b"a\t2\t3\t1\na\t3\t5\t2\na\t5\t7\t1\na\t7\t8\t0\n"
    assert dm.expected(path, "a:4-5")[0] == b"a\t3\t5\t2\n"
    assert dm.expected(path, "b")[0] == b and dm.expected(path, "c:9")[0] == b"" and dm.expected(path, "a:10-40")[0] == b"a\t9\t10\t1\n"


def test_model_on_the_long_cigar_hand_file():
    """hand_longcigar.bam: one record at 1000 (0-based), CIGAR field 30S35N, CG tag 10M5D20M: LONG_EXPECT's 1-based positions."""
    path = os.path.join(GOLDEN, "hand_longcigar.bam")
    d = depth_of(path, 0)
    for p, want in LONG_EXPECT["depth"].items():
        assert d[p - 1] == want, p
    text, info = dm.expected(path)
    assert text.startswith(b"chr1\t0\t1000\t0\nchr1\t1000\t1035\t1\nchr1\t1035\t") and info["records_counted"] == 1


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_runs_sum_to_the_oracles_coverage_histogram(oracle_mod, tmp_path, seed):
    """exclude_flags = 0, min_mapq = 0: the reference's Coverage counts the same records over the same positions (coverage.rs:
    159-180).  Its per-sequence histogram has one entry more than the sequence has positions, index 0, which no record reaches:
    one position of depth 0 per covered sequence is added to the model's side.  A sequence is covered for the oracle when a
    record is yielded for it, also one without a span."""
    names, lens, hb = case_random(seed)
    path = str(tmp_path / "r.bam")
    bamio.write_bam(path, hb, names, lens, with_index=False)
    o = oracle_mod.Oracle(lens, facets=ffi.FACET_COVERAGE, cov_cap=5000)
    o.process_batch(hb)
    o.finalize()
    cov = o.results(names)["coverage"]
    want = np.array(cov["coverage_distribution"]["values"], dtype=np.int64)
    got = np.zeros_like(want)
    covered = [names.index(n) for n in cov["mean_coverage"]]
    assert covered
    _, _, recs, _ = dm.read(path)
    kept = [r for r in recs if dm.counts(r, 0, 0)]
    for ref in covered:
        for s, e, d in dm.runs(dm.depths(kept, ref, 0, lens[ref])):
            got[d] += e - s
        got[0] += 1
    assert (got == want).all()


# ---- the GPU inputs reach their edges -------------------------------------------------------------------------------------
def changes(d):
    return set((np.flatnonzero(d[1:] != d[:-1]) + 1).tolist())


def test_inputs_reach_their_edges(lib, tmp_path):
    T = tile()
    assert T >= 64 and host.depth_tile_positions(T) == T and host.depth_tile_positions(T + 1) == 2 * T
    assert host.depth_tile_positions(0) % T == 0 and host.depth_tile_positions(0) > 2 * T
    # lengths
    names, lens, recs = case_lengths()
    path = write_case(str(tmp_path / "l.bam"), names, lens, recs)
    assert lens == [63, 64, 65, T - 1, T, T + 1]
    for r, L in enumerate(lens):
        d = depth_of(path, r)
        assert d[0] == 1 and d[L - 1] == 2 and d[L - 4] == 1 and d[L - 6] == 0
    # tiles
    names, lens, recs = case_tiles()
    path = write_case(str(tmp_path / "t.bam"), names, lens, recs)
    d, L = depth_of(path, 0), lens[0]
    ch = changes(d)
    assert {T - 1, T, T + 1} <= ch and d[0] == 2
    assert 2 * T - 10 in ch and 3 * T + 20 in ch and not [p for p in ch if 2 * T - 10 < p < 3 * T + 20]   # one run over tile 2
    assert 4 * T in ch and 4 * T - 1 in ch and d[L - 1] == 3 and L - 4 in ch and L - 2 in ch
    # filters
    names, lens, recs = case_filters()
    path = write_case(str(tmp_path / "f.bam"), names, lens, recs)
    n_all = dm.expected(path, exclude_flags=0)[1]["records_counted"]
    assert n_all == 18 and dm.expected(path)[1]["records_counted"] == 14
    for bit in (4, 256, 512, 1024):
        assert dm.expected(path, exclude_flags=bit)[1]["records_counted"] == n_all - 1
    assert [dm.expected(path, exclude_flags=0, min_mapq=m)[1]["records_counted"] for m in (0, 1, 10, 11, 255)] == [18, 17, 16, 15, 1]
    # piles and powers of ten
    names, lens, recs = case_piles()
    d = depth_of(write_case(str(tmp_path / "p.bam"), names, lens, recs), 0)
    assert d.max() == 1000 and {9, 10, 99, 100, 999, 1000} <= set(d.tolist())
    names, lens, recs = case_pow10()
    text = dm.expected(write_case(str(tmp_path / "w.bam"), names, lens, recs))[0]
    starts = {int(ln.split(b"\t")[1]) for ln in text.splitlines()}
    assert all({10 ** k - 1, 10 ** k, 10 ** k + 1} <= starts for k in range(1, 6))
    # batches: sequences b1 and b4 lie inside one batch of 7 with their neighbours
    names, lens, recs = case_batches()
    refs = [r["ref_id"] for r in sorted(recs, key=sort_key)]
    assert any(len(set(refs[k:k + 7])) >= 3 for k in range(0, len(refs), 7)) and refs.count(0) > 65 and refs.count(3) == 0
    # genome: empty sequences before, between and after covered ones
    names, lens, recs = case_genome()
    live = sorted({r["ref_id"] for r in recs})
    assert len(names) == 195 and live[0] == 1 and live[-1] < 192 and max(lens) < 200_000 * 8 and any(b - a > 1 for a, b in zip(live, live[1:]))
    # order: the model names the record, and with 64 records a batch record 64 is a batch's first
    for bad, batch in ORDER_CASES:
        names, lens, recs = case_order(bad)
        path = write_case(str(tmp_path / "o.bam"), names, lens, recs, in_order=False)
        with pytest.raises(dm.DepthError, match=f"reading BAM record: record {bad} \\(0-based\\) is out of coordinate order: " + dm.NOT_SORTED):
            dm.expected(path)
        assert batch == 0 or (bad % batch == 0) == (bad == 64)
    # queries
    names, lens, recs = case_query()
    path = write_case(str(tmp_path / "q.bam"), names, lens, recs, block_payload=3000)
    assert dm.expected(path, "q1:4500-5500")[0] == b"q1\t4499\t5500\t1\n"                   # inside one run
    assert dm.expected(path, "q1:3000-3005")[0] == b"q1\t2999\t3005\t1\n"                   # a record from in front reaches in
    assert dm.expected(path, "q1:2905-2915")[0] == b"q1\t2904\t2915\t1\n"                   # covered by an N alone
    assert dm.expected(path, "q3:4000-9000")[0].endswith(b"\t5000\t1\n")                     # E beyond L
    assert dm.expected(path, "q3:4995")[0] == b"q3\t4994\t5000\t1\n"
    assert dm.expected(path, "q2:100-200")[0] == b"q2\t99\t200\t0\n" and dm.expected(path, "q1:300001")[0] == b""
    assert len(vm.query_chunks(open(path + ".bai", "rb").read(), 0, 6000, 200000)) >= 2    # (several merged chunks: range walks to coalesce)


# ---- the command line -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli")
    names, lens, recs = case_query()
    good = write_case(str(d / "good.bam"), names, lens, recs[:50])
    unsorted = str(d / "unsorted.bam")
    bamio.write_bam(unsorted, batch_from_records(recs[:5]), names, lens, with_index=False, sort_order="unsorted")
    noindex = write_case(str(d / "noindex.bam"), names, lens, recs[:50], index=False)
    return dict(d=str(d), good=good, unsorted=unsorted, noindex=noindex)


def refusals(f):
    return [
        ([], "the following required arguments were not provided: <BAM>"),
        (["a.bam", "chr1", "more"], "unexpected argument 'more' found"),
        (["--nope", "a.bam"], "unexpected argument '--nope' found"),
        (["a.bam", "--min-mapq"], "a value is required for '--min-mapq <INT>' but none was supplied"),
        (["a.bam", "--exclude-flags"], "a value is required for '--exclude-flags <INT>' but none was supplied"),
        (["a.bam", "-o"], "a value is required for '--output <PATH>' but none was supplied"),
        (["--exclude-flags", "x", "a.bam"], "invalid value 'x' for '--exclude-flags <INT>': invalid digit found in string"),
        (["--exclude-flags", "0x4", "a.bam"], "invalid value '0x4' for '--exclude-flags <INT>': invalid digit found in string"),
        (["--exclude-flags", "65536", "a.bam"], "invalid value '65536' for '--exclude-flags <INT>': number too large to fit in target type"),
        (["--min-mapq", "256", "a.bam"], "invalid value '256' for '--min-mapq <INT>': number too large to fit in target type"),
        (["--min-mapq", "99999999999999999999999", "a.bam"], "for '--min-mapq <INT>': number too large to fit in target type"),
        (["--min-mapq", "-1", "a.bam"], "invalid value '-1' for '--min-mapq <INT>': invalid digit found in string"),
        (["x.sam"], "incompatible formats: required BAM, found SAM"),
        (["x.cram"], "incompatible formats: required BAM, found CRAM"),
        (["x.fastq.gz"], "incompatible formats: required BAM, found Gzipped FASTQ"),
        (["x.ubam"], "incompatible formats: required BAM, found Unaligned BAM"),
        (["x.unknown"], "Not able to determine filetype for extension: unknown"),
        ([os.path.join(f["d"], "missing.bam")], "missing.bam"),
        ([f["unsorted"]], "the input BAM must be coordinate-sorted to compute depth"),
        ([f["unsorted"], "q1"], "the input BAM must be coordinate-sorted to compute depth"),
        ([f["noindex"], "q1:5-9"], "reading BAM index: "),
        ([f["good"], ""], "parsing query: "),
        ([f["good"], "chrX:5"], "querying BAM file: "),
    ]


def test_every_refusal_prints_its_message_and_writes_nothing(ngs, files):
    out = os.path.join(files["d"], "never.bedgraph")
    for args, msg in refusals(files):
        for extra in ([], ["-o", out]):
            if "-o" in args and extra:
                continue
            r = run(ngs, "depth", *extra, *args)
            assert r.returncode == 1, (args, r.stderr)
            assert b"Error: " in r.stderr and msg.encode() in r.stderr, (args, r.stderr)
            assert r.stdout == b"" and not os.path.exists(out), args


def test_help_and_the_other_commands(ngs):
    for flag in ("-h", "--help"):
        r = run(ngs, "depth", flag)
        assert r.returncode == 0 and r.stdout == b""
        h = r.stderr.decode()
        for s in ("Usage: ngs depth [OPTIONS] <BAM> [QUERY]", "-o, --output <PATH>", "--exclude-flags <INT>", "[default: 1796]", "--min-mapq <INT>",
                  "[default: 0]", "--device <N>"):
            assert s in h, s
    assert run(ngs, "-q", "depth", "--help").returncode == 0
    # the commands beside it answer as before
    for cmd in ("view", "index", "convert", "generate"):
        assert run(ngs, cmd, "--help").returncode == 0
    assert run(ngs, "derive", "instrument", "--help").returncode == 0
    r = run(ngs, "nosuchcommand")
    assert r.returncode == 1 and b"Error: " in r.stderr
    assert run(ngs).returncode == 1


def test_the_library_refuses_before_any_gpu_work(lib, files, tmp_path):
    """An unsorted header, a bad query, a missing index and bad arguments are answered without a device; the tile size is pure."""
    C = ffi.C
    for path, query, code, msg in ((files["unsorted"], None, ffi.ERR_UNSORTED, dm.NOT_SORTED), (files["good"], b"", ffi.ERR_INVALID_ARGUMENT, "parsing query: "),
                                   (files["good"], b"nope", ffi.ERR_INVALID_ARGUMENT, "querying BAM file: "),
                                   (files["noindex"], b"q1", ffi.ERR_INVALID_ARGUMENT, "reading BAM index: ")):
        bam = C.c_void_p()
        assert lib.ngsq_bam_open(path.encode(), 0, C.byref(bam)) == 0
        try:
            fd = os.open(str(tmp_path / "o"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
            fake = C.cast(C.c_void_p(8), ffi.ctx_p)            # never looked at: the call fails in front of the device
            assert lib.ngsq_bam_depth(bam, fake, fd, query, None, 1796, 0, 0, 0, 0, None) == code
            assert msg in lib.ngsq_bam_last_error().decode()
            assert lib.ngsq_bam_depth(bam, None, fd, query, None, 1796, 0, 0, 0, 0, None) == ffi.ERR_INVALID_ARGUMENT
            assert lib.ngsq_bam_depth(bam, fake, fd, query, None, 65536, 0, 0, 0, 0, None) == ffi.ERR_INVALID_ARGUMENT
            assert lib.ngsq_bam_depth(bam, fake, fd, query, None, 0, 256, 0, 0, 0, None) == ffi.ERR_INVALID_ARGUMENT
            assert lib.ngsq_bam_depth(bam, fake, -1, query, None, 0, 0, 0, 0, 0, None) == ffi.ERR_INVALID_ARGUMENT
            os.close(fd)
            assert os.path.getsize(str(tmp_path / "o")) == 0
        finally:
            lib.ngsq_bam_close(bam)


def test_an_empty_interval_needs_no_gpu(lib, files, tmp_path):
    """A region that begins behind its sequence's end has no line and is no error: answered before the device is touched."""
    C = ffi.C
    bam = C.c_void_p()
    assert lib.ngsq_bam_open(files["good"].encode(), 0, C.byref(bam)) == 0
    try:
        fd = os.open(str(tmp_path / "o"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
        rep = ffi.DepthReport()
        assert lib.ngsq_bam_depth(bam, C.cast(C.c_void_p(8), ffi.ctx_p), fd, b"q3:5001", None, 1796, 0, 0, 0, 0, C.byref(rep)) == 0
        os.close(fd)
        assert os.path.getsize(str(tmp_path / "o")) == 0 and rep.runs == 0 and rep.text_bytes == 0
        assert dm.expected(files["good"], "q3:5001")[0] == b""
    finally:
        lib.ngsq_bam_close(bam)
