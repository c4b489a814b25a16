"""`ngs convert --gzip device --sort coordinate` in rounds without a GPU: the plan restated in Python
(tests/sort_rounds_model.py) held to cases worked by hand, with the per-record constants read from the library; the inputs and
budgets of tests/test_sort_rounds_gpu.py, each held to give two rounds or more and to reach the edge its case names; and the
command line's `--sort-memory`, as far as it answers before any GPU work."""
import gzip
import os
import subprocess

import pytest

from ngs_amd import build
from tests import bam_sort_model as bsm
from tests import bam_text_model as tm
from tests import sort_model as som
from tests import sort_rounds_model as srm
from tests.test_bam_sort import REFS, TEXT, rec, stream
from tests.test_bam_sort_gpu import alignment_file, bam_of
from tests.test_convert_gpu import write_long_reads
from tests.test_sam_to_bam import HEAD, random_sam

SORTED = ["--gzip", "device", "--sort", "coordinate"]
NEEDS = "Error: --sort-memory needs --gzip device and --sort coordinate and a BAM to write"


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


@pytest.fixture(scope="module")
def per(lib):
    return lib.ngsq_sort_resident_bytes_per_record()


def run(ngs, *args):
    return subprocess.run([ngs, *args], capture_output=True, text=True, timeout=120)


# ---- the constants and the plan -------------------------------------------------------------------------------------------------
def test_the_constants_are_what_the_arrays_take(lib):
    """Beside a resident record: address 8, length 4, key 8, the sort's second keys 8 and two index arrays 8, the sorted offset 8,
    and the pass table's share -- 256 entries of 8 bytes per tile of keys -- rounded up with the rest to 48.  Per record of the
    survey: key 8, length 4, second keys 8, two index arrays 8, the pass table's share rounded up; the offsets lie in the spare
    half of the keys."""
    tile = lib.ngsq_sort_tile_keys()
    table = -(-256 * 8 // tile)
    assert lib.ngsq_sort_resident_bytes_per_record() == 48 >= 8 + 4 + 8 + 8 + 8 + 8 + table
    assert lib.ngsq_sort_survey_bytes_per_record() == 8 + 4 + 8 + 8 + table


def test_model_plan_worked_by_hand():
    R = srm.Round
    # budget 100, 10 bytes per record: 40 + 30 + 2 * 10 = 90 fits, a third record of 20 would make 120
    assert srm.plan([40, 30, 20, 90, 5], 100, 10) == [R(0, 2, 70), R(2, 3, 20), R(3, 4, 90), R(4, 5, 5)]
    assert srm.plan([10, 10, 10, 10], 80, 10) == [R(0, 4, 40)]                   # exactly the budget: one round
    assert srm.plan([10, 10, 10, 10], 79, 10) == [R(0, 3, 30), R(3, 4, 10)]
    assert srm.plan([], 5, 10) == []
    with pytest.raises(srm.RecordTooLarge) as e:
        srm.plan([40, 30, 20, 90, 5], 99, 10)                                     # the record at rank 3 needs 100
    assert (e.value.rank, e.value.need) == (3, 100)
    assert [srm.walks(k) for k in (1, 2, 5)] == [1, 4, 7]


def test_model_plan_follows_the_sorted_order_and_its_ties():
    """Worked by hand on the records of tests/test_bam_sort.py: the sorted order is c1p0, c1p7, c1p7b, c1p7c, c2p9, c2p9b and the
    four unplaced ones; three records a round puts the first boundary inside the ties at (chr1, 7)."""
    names = [(b"u0", -1, -1), (b"c2p9", 1, 9), (b"c1p7", 0, 7), (b"nopos", 0, -1), (b"c1p7b", 0, 7), (b"u1", -1, -1), (b"c1p0", 0, 0),
             (b"u7", -1, 6), (b"c2p9b", 1, 9), (b"c1p7c", 0, 7)]
    recs = [rec(r, p, n.ljust(5, b"x")) for n, r, p in names]
    size = len(recs[0])
    assert all(len(r) == size for r in recs)
    bam = tm.bam_file(stream(TEXT, REFS, recs))
    plan = srm.plan_of(bam, 3 * (size + 48), 48)
    assert [(r.first, r.end) for r in plan] == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert srm.kept(recs, plan) == [[2, 4, 6], [1, 8, 9], [0, 3, 5], [7]]         # input ordinals, in input order
    assert srm.boundary_keys(recs, plan)[0] == (som.key(recs[2]), som.key(recs[9]))
    assert som.key(recs[2]) == som.key(recs[9])                                   # the boundary cuts the ties
    assert srm.budget_for(recs, 48, 4) == 3 * (size + 48) and srm.budget_for(recs, 48, 1) == 10 * (size + 48)


# ---- the inputs of the GPU tests --------------------------------------------------------------------------------------------------
def test_the_tie_group_straddles_the_boundary(per):
    bam, budget = srm.case_ties(per)
    recs = srm.records_of(bam)
    plan = srm.plan_of(bam, budget, per)
    tie = som.key(srm.raw_record(0, 5000, b"x"))
    assert len(plan) == 2 and srm.boundary_keys(recs, plan) == [(tie, tie)]
    assert sum(1 for r in recs if som.key(r) == tie) == 200
    names = [r[36:r.index(b"\0", 36)] for r in recs if som.key(r) == tie]
    assert names == [b"tie%03d" % t for t in range(200)]                          # their names tell their input order
    assert [r[36:39] for r in recs[:40]].count(b"tie") not in (0, 40)             # and they lie among the others


def test_the_unplaced_block_is_cut(per):
    bam, budget = srm.case_unplaced(per)
    recs = srm.records_of(bam)
    plan = srm.plan_of(bam, budget, per)
    unplaced = 0xFFFFFFFF << 32
    assert len(plan) == 3 and (unplaced, unplaced) in srm.boundary_keys(recs, plan)
    assert sum(1 for r in recs if som.key(r) == unplaced) == 180
    assert sum(1 for r in recs if som.key(r) == unplaced and r[4:8] != b"\xff\xff\xff\xff") == 36     # a sequence and no position


@pytest.mark.parametrize("n", [65, 257, 4097])
def test_reversed_input_gives_every_batch_to_every_round(per, n):
    bam, budget = srm.case_reversed(n, per)
    recs = srm.records_of(bam)
    plan = srm.plan_of(bam, budget, per)
    batch = -(-n // 4)
    assert len(plan) == 3
    assert [som.key(r) for r in recs] == sorted((som.key(r) for r in recs), reverse=True)
    # reversed input: a round's records are consecutive in the input, and four batches over three rounds cut every round
    touched = [srm.batches_touched(k, n, batch) for k in srm.kept(recs, plan)]
    assert all(t >= 2 for t in touched)


def test_sorted_input_gives_a_batch_to_one_round_or_two(per):
    bam, budget = srm.case_sorted(per)
    recs = srm.records_of(bam)
    plan = srm.plan_of(bam, budget, per)
    assert len(plan) == 4 and [som.key(r) for r in recs] == sorted(som.key(r) for r in recs)
    rounds_of_batch = [{k for k, ordinals in enumerate(srm.kept(recs, plan)) if any(i // 100 == b for i in ordinals)} for b in range(12)]
    assert all(1 <= len(s) <= 2 for s in rounds_of_batch) and any(len(s) == 2 for s in rounds_of_batch)
    assert all(srm.batches_touched(k, 1200, 100) <= 5 for k in srm.kept(recs, plan))        # most of the 12 batches keep nothing


def test_the_alignment_file_reaches_every_residue(per):
    bam = alignment_file()
    recs = srm.records_of(bam)
    budget = srm.alignment_budget(recs, per)
    plan = srm.plan_of(bam, budget, per)
    assert 3 <= len(plan) <= 4
    at = srm.view_offsets(bam)
    kept = srm.kept(recs, plan)
    for ordinals in kept[:3]:
        assert {at[i] % 16 for i in ordinals} == set(range(16))                   # kept records start at every residue of the view
    assert set().union(*({o % 8 for o in srm.slab_offsets(recs, k)} for k in kept)) == set(range(8))       # and land at every one of the slab
    for piece in (1000, 4096):
        cuts, inside = srm.piece_cuts(plan, piece)
        assert len(inside) >= 2                                                   # boundaries inside a piece: it spans two rounds
    assert srm.spanning_records(recs, plan, 1000)                                 # a record in two pieces, the first of them two rounds'


def test_the_long_reads_are_cut_next_to_the_longest(per, tmp_path):
    src = str(tmp_path / "l.bam")
    write_long_reads(src)
    recs = bsm.split(gzip.decompress(open(src, "rb").read()))[2]
    budget = max(len(r) for r in recs) + 2 * per + 100
    plan = srm.plan([len(recs[i]) for i in srm.order_of(recs)], budget, per)
    longest = max(range(len(recs)), key=lambda i: len(recs[i]))
    rank = srm.order_of(recs).index(longest)
    assert len(plan) >= 3 and max(len(r) for r in recs) > 64 * 8 * 64            # (many passes of a wave's 64 eight-byte words)
    assert any(r.first == rank or r.end == rank + 1 for r in plan)               # a boundary next to it


def test_random_files_give_the_rounds_their_tests_name(per, lib, tmp_path):
    survey_per = lib.ngsq_sort_survey_bytes_per_record()
    for seed, n, want in ((171, 300, 2), (172, 600, 2), (172, 600, 3), (174, 700, 2), (174, 700, 3)):
        recs = srm.records_of(bam_of(random_sam(seed, n, tmp_path), 7000))
        lengths = [len(recs[i]) for i in srm.order_of(recs)]
        assert len(srm.plan(lengths, srm.budget_for(recs, per, want), per)) == want
        most = srm.plan(lengths, srm.most_rounds_budget(recs, survey_per), per)
        assert len(most) >= 8
    recs = srm.records_of(bam_of(random_sam(176, 2000, tmp_path), 7000))
    assert 2000 * survey_per <= 64 << 10                                          # the command line's case: the survey fits 64K
    assert len(srm.plan([len(recs[i]) for i in srm.order_of(recs)], 64 << 10, per)) >= 2
    first = srm.records_of(bam_of(random_sam(173, 500, tmp_path), 7000), 333)
    assert len(first) == 333 and 333 % 100 and len(srm.plan([len(first[i]) for i in srm.order_of(first)], srm.budget_for(first, per, 3), per)) == 3


# ---- the command line, before any GPU work ----------------------------------------------------------------------------------------
@pytest.fixture()
def files(tmp_path):
    bam, sam = str(tmp_path / "in.bam"), str(tmp_path / "in.sam")
    with open(bam, "wb") as f:
        f.write(tm.bam_file(stream(TEXT, REFS, [rec(1, 3), rec(0, 8), rec(-1, -1)])))
    with open(sam, "w") as f:
        f.write(HEAD + "r\t0\tchr1\t5\t60\t4M\t=\t9\t0\tACGT\tIIII\n")
    return bam, sam


def test_help_names_the_flag(ngs):
    r = run(ngs, "convert", "--help")
    h = r.stderr + r.stdout
    assert r.returncode == 0 and "--sort-memory <SIZE>" in h and "rounds" in h[h.index("--sort-memory"):]
    for s in ("--write-index", "--sort <ORDER>", "--gzip <WHERE>", "-n, --num-records <USIZE>"):          # its lines stay
        assert s in h, s


@pytest.mark.parametrize("value,reason", [
    ("", "a size is decimal digits with an optional K, M or G suffix"), ("K", "a size is decimal digits with an optional K, M or G suffix"),
    ("12Q", "a size is decimal digits with an optional K, M or G suffix"), ("1KB", "a size is decimal digits with an optional K, M or G suffix"),
    ("1.5G", "a size is decimal digits with an optional K, M or G suffix"), ("-5", None), ("+5", "a size is decimal digits with an optional K, M or G suffix"),
    ("0x10", "a size is decimal digits with an optional K, M or G suffix"), ("0", "a size is at least one byte"), ("0M", "a size is at least one byte"),
    ("99999999999999999999", "number too large to fit in target type"), ("17179869184G", "number too large to fit in target type")])
def test_bad_sizes_are_refused(ngs, files, tmp_path, value, reason):
    before = sorted(os.listdir(tmp_path))
    r = run(ngs, "convert", *SORTED, "--sort-memory", value, files[0], str(tmp_path / "o.bam"))
    assert r.returncode == 1 and r.stdout == ""
    if reason is not None:
        assert r.stderr.strip() == f"Error: invalid value '{value}' for '--sort-memory <SIZE>': {reason}"
    assert sorted(os.listdir(tmp_path)) == before


def test_the_flag_is_refused_wherever_no_sorted_path_is_reached(ngs, files, tmp_path):
    bam, sam = files
    before = sorted(os.listdir(tmp_path))
    cases = [(SORTED, bam, "o.sam"), ([], bam, "o.sam"), (["--gzip", "device", "--sort", "none"], bam, "o.bam"),
             (["--gzip", "device"], sam, "o.bam"), (["--gzip", "host", "--sort", "coordinate"], bam, "o.bam"), ([], sam, "o.bam")]
    for args, frm, to in cases:
        for size in ("64K", "1G", "123"):
            r = run(ngs, "convert", "--sort-memory", size, *args, frm, str(tmp_path / to))
            assert (r.returncode, r.stdout, r.stderr.strip()) == (1, "", NEEDS), (args, frm, to)
        assert sorted(os.listdir(tmp_path)) == before                             # before any file is opened
    r = run(ngs, "convert", "--sort-memory", "64K", "--write-index", bam, str(tmp_path / "o.sam"))       # --write-index's refusal comes first
    assert r.stderr.strip() == "Error: --write-index needs --gzip device and --sort coordinate and a BAM to write"
    r = run(ngs, "convert", *SORTED, "--sort-memory")
    assert r.returncode == 1 and "--sort-memory <SIZE>" in r.stderr


@pytest.mark.parametrize("which", ["bam", "sam"])
def test_an_existing_index_is_still_refused_first(ngs, files, tmp_path, which):
    frm = files[0] if which == "bam" else files[1]
    to, bai = tmp_path / "sorted.bam", tmp_path / "sorted.bam.bai"
    to.write_bytes(b"what was here before")
    bai.write_bytes(b"an index of something else")
    r = run(ngs, "convert", *SORTED, "--sort-memory", "1K", "--write-index", frm, str(to))
    assert (r.returncode, r.stdout) == (1, "")
    assert r.stderr.strip() == f"Error: refusing to overwrite existing index file: {bai}. Please delete and rerun if you'd like to replace it."
    assert to.read_bytes() == b"what was here before" and bai.read_bytes() == b"an index of something else"
