"""`ngs convert --gzip device --sort coordinate` in rounds on the GPU: a BAM whose records do not fit the
budget is walked again -- a survey, then a walk per round -- and comes out as the file the in-memory path writes.  Every case
holds the decompressed output to tests/bam_sort_model.py byte for byte and the file, byte for byte, to the one the existing
in-memory entry writes for the same input and piece_bytes; the number of rounds, the walks and the largest round's residence
come from tests/sort_rounds_model.py, so a conversion that quietly stayed in one round fails.  tests/test_sort_rounds.py holds,
on the CPU, that every budget here gives two rounds or more and that the edge a case names occurs."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from ngs_amd import build, ffi, host
from tests import bam_sort_model as bsm
from tests import bam_text_model as tm
from tests import bamio
from tests import sort_rounds_model as srm
from tests import view_model as vm
from tests.test_bam_sort_gpu import CTX, alignment_file, bam_of, ingest_message, names_of
from tests.test_convert_gpu import write_long_reads
from tests.test_sam_to_bam import HEAD, NAMES, random_sam
from tests.test_sam_to_bam_gpu import line
from tests.test_sort_index_gpu import LIMIT_TEXT, M, bam_with, held, rec
from tests.util import random_batch

pytestmark = pytest.mark.gpu

SAME = ("records", "header_bytes", "bam_bytes", "compressed_bytes", "batches", "pieces", "blocks", "stored_blocks", "passes_run", "passes_skipped")


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def constants(lib):
    return lib.ngsq_sort_resident_bytes_per_record(), lib.ngsq_sort_survey_bytes_per_record()


def in_rounds(lib, bam: bytes, tmp_path, budget: int, name="r", bai=False, tile=0, **kw):
    """Convert in memory with the existing entry and at `budget` with the rounds entry; hold the rounds' file to the model and
    to the in-memory file, and its reports to the plan.  (file bytes, sort report, rounds report, path, plan)"""
    per, survey_per = constants(lib)
    src, ref, out = str(tmp_path / (name + ".in.bam")), str(tmp_path / (name + ".ref.bam")), str(tmp_path / (name + ".bam"))
    with open(src, "wb") as f:
        f.write(bam)
    for p in (ref + ".bai", out + ".bai"):
        if os.path.exists(p):
            os.remove(p)
    old = host.bam_to_sorted_bam(src, ref, lib=lib, bai_path=ref + ".bai" if bai else None, index_tile_records=tile, **kw)
    got = host.bam_to_sorted_bam(src, out, lib=lib, max_resident_bytes=budget, rounds=True, bai_path=out + ".bai" if bai else None,
                                 index_tile_records=tile, **kw)
    old_rep, rep, rr = (old[0] if bai else old), got[0], got[-1]
    raw = open(out, "rb").read()
    n_max = kw.get("max_records", 0)
    assert gzip.decompress(raw) == bsm.bam_stream(bam, n_max), "the stream differs from tests/bam_sort_model.py"
    assert raw == open(ref, "rb").read(), "the file differs from the in-memory entry's"
    recs = srm.records_of(bam, n_max)
    plan = srm.plan_of(bam, budget, per, n_max)
    print(f"rounds {rr['rounds']} (model {len(plan)}), walks {rr['walks']}, resident {rep['resident_bytes']} of {budget}")
    assert rr["rounds"] == len(plan) and rr["walks"] == srm.walks(len(plan)) and rr["budget"] == budget
    assert rr["survey_bytes"] == (len(recs) * survey_per if len(plan) > 1 else 0)
    assert rep["resident_bytes"] == max(r.resident(per) for r in plan) <= budget
    assert {k: rep[k] for k in SAME} == {k: old_rep[k] for k in SAME}
    if bai:
        index = open(out + ".bai", "rb").read()
        assert index == open(ref + ".bai", "rb").read(), "the index differs from the in-memory entry's"
        by_index = held(out, index, lib, tmp_path)
        assert {k: got[1][k] for k in ("records", "n_no_coor", "runs", "bins")} == {k: by_index[k] for k in ("records", "n_no_coor", "runs", "bins")}
    return raw, rep, rr, out, plan


# ---- 1. a file that fits ------------------------------------------------------------------------------------------------------------
def test_a_file_that_fits_is_the_old_call(gpu_lib, tmp_path):
    per, _ = constants(gpu_lib)
    bam = bam_of(random_sam(171, 300, tmp_path), 7000)
    recs = srm.records_of(bam)
    exact = sum(len(r) for r in recs) + len(recs) * per
    for budget in (0, exact):
        src, ref, out = str(tmp_path / "f.in.bam"), str(tmp_path / "f.ref.bam"), str(tmp_path / "f.bam")
        open(src, "wb").write(bam)
        old = host.bam_to_sorted_bam(src, ref, lib=gpu_lib, max_resident_bytes=budget, batch_records=100)
        rep, rr = host.bam_to_sorted_bam(src, out, lib=gpu_lib, max_resident_bytes=budget, batch_records=100, rounds=True)
        assert open(out, "rb").read() == open(ref, "rb").read()
        assert {k: v for k, v in rep.items() if not k.endswith("_ms")} == {k: v for k, v in old.items() if not k.endswith("_ms")}
        assert rr["rounds"] == 1 and rr["walks"] == 1 and rr["survey_bytes"] == 0 and rr["survey_records"] == 0 and rr["survey_ms"] == 0
        assert budget == 0 or rr["budget"] == budget
    _, _, rr, _, _ = in_rounds(gpu_lib, bam, tmp_path, exact - 1)              # one byte less: rounds
    assert rr["rounds"] == 2


# ---- 2. two, three and the most rounds ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rounds", [2, 3, 0])
def test_rounds(gpu_lib, tmp_path, rounds):
    per, survey_per = constants(gpu_lib)
    bam = bam_of(random_sam(172, 600, tmp_path), 7000)
    recs = srm.records_of(bam)
    budget = srm.budget_for(recs, per, rounds) if rounds else srm.most_rounds_budget(recs, survey_per)
    _, rep, rr, out, plan = in_rounds(gpu_lib, bam, tmp_path, budget, batch_records=170)
    assert rr["rounds"] == (rounds or len(plan)) and rr["rounds"] >= 2 and rr["survey_records"] == 600
    assert rounds or rr["rounds"] >= 8                                            # (the most the survey allows: about ten)
    assert host.build_bam_index(out, lib=gpu_lib)["records"] == 600


# ---- 3. ties and unplaced records across a boundary ---------------------------------------------------------------------------------
def test_a_tie_group_across_a_boundary_keeps_input_order(gpu_lib, tmp_path):
    per, _ = constants(gpu_lib)
    bam, budget = srm.case_ties(per)
    raw, _, rr, _, _ = in_rounds(gpu_lib, bam, tmp_path, budget, batch_records=64)
    assert rr["rounds"] == 2
    ties = [n for n in names_of(raw) if n.startswith("tie")]
    assert ties == [f"tie{t:03d}" for t in range(200)]


def test_unplaced_records_cut_by_a_boundary(gpu_lib, tmp_path):
    per, _ = constants(gpu_lib)
    bam, budget = srm.case_unplaced(per)
    raw, _, rr, out, _ = in_rounds(gpu_lib, bam, tmp_path, budget, batch_records=50, bai=True)
    assert rr["rounds"] == 3
    tail = names_of(raw)[120:]
    assert tail == [n for n in names_of(bam) if n.startswith(("u", "zero"))]     # behind the placed ones, in input order


# ---- 4. reversed and sorted input ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 257, 4097])
def test_reversed_input(gpu_lib, tmp_path, n):
    per, _ = constants(gpu_lib)
    assert n != 4097 or n == gpu_lib.ngsq_sort_tile_keys() + 1
    bam, budget = srm.case_reversed(n, per)
    _, rep, rr, _, _ = in_rounds(gpu_lib, bam, tmp_path, budget, batch_records=-(-n // 4))
    assert rr["rounds"] == 3 and rep["records"] == n


def test_sorted_input_skips_most_batches(gpu_lib, tmp_path):
    per, _ = constants(gpu_lib)
    bam, budget = srm.case_sorted(per)
    _, rep, rr, _, _ = in_rounds(gpu_lib, bam, tmp_path, budget, batch_records=100)
    assert rr["rounds"] == 4 and rep["batches"] == 12 and rep["passes_run"] >= 2


# ---- 5. alignment -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 7, 64, 65, 0])
def test_every_residue_of_a_kept_record(gpu_lib, tmp_path, batch):
    per, _ = constants(gpu_lib)
    bam = alignment_file()
    budget = srm.alignment_budget(srm.records_of(bam), per)
    for piece in (0, 1000, 4096):
        _, rep, rr, _, _ = in_rounds(gpu_lib, bam, tmp_path, budget, batch_records=batch, piece_bytes=piece)
        assert rr["rounds"] >= 3 and rep["records"] == 400


# ---- 6. long records ----------------------------------------------------------------------------------------------------------------
def test_long_records_next_to_a_boundary(gpu_lib, tmp_path):
    per, _ = constants(gpu_lib)
    src = str(tmp_path / "l.bam")
    write_long_reads(src)
    data = gzip.decompress(open(src, "rb").read())
    recs = bsm.split(data)[2]
    bam = tm.bam_file(data[:len(data) - sum(len(r) for r in recs)] + b"".join(reversed(recs)), 60000)
    budget = max(len(r) for r in recs) + 2 * per + 100                            # the longest record and the short one beside it
    _, rep, rr, _, plan = in_rounds(gpu_lib, bam, tmp_path, budget, piece_bytes=65536, bai=True)
    assert rr["rounds"] == len(plan) >= 3 and rep["records"] == len(recs)


# ---- 7. -n -----------------------------------------------------------------------------------------------------------------------------
def test_the_first_n_records_in_rounds(gpu_lib, tmp_path):
    per, _ = constants(gpu_lib)
    bam = bam_of(random_sam(173, 500, tmp_path), 7000)
    recs = srm.records_of(bam, 333)
    _, rep, rr, _, _ = in_rounds(gpu_lib, bam, tmp_path, srm.budget_for(recs, per, 3), max_records=333, batch_records=100, bai=True)
    assert rep["records"] == 333 and rr["rounds"] == 3 and rr["survey_records"] == 333


# ---- 8. the index across rounds -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rounds", [2, 3, 0])
def test_index_across_rounds(gpu_lib, tmp_path, rounds):
    per, survey_per = constants(gpu_lib)
    bam = bam_of(random_sam(174, 700, tmp_path), 7000)
    recs = srm.records_of(bam)
    budget = srm.budget_for(recs, per, rounds) if rounds else srm.most_rounds_budget(recs, survey_per)
    _, _, rr, out, _ = in_rounds(gpu_lib, bam, tmp_path, budget, bai=True, batch_records=300, piece_bytes=20000)
    assert rr["rounds"] >= max(rounds, 2)


@pytest.mark.parametrize("tile", [1, 64, 65])
def test_index_tiles_and_rounds(gpu_lib, tmp_path, tile):
    """192 sorted records per round but the last: a tile of 64 ends at every round's end, a tile of 65 inside and across rounds."""
    per, _ = constants(gpu_lib)
    recs = srm.shuffled([srm.raw_record(k * 3 // 500, 1 + 40 * k, b"n%03d" % k) for k in range(500)], 35)
    assert len({len(r) for r in recs}) == 1
    budget = 192 * (len(recs[0]) + per)
    _, _, rr, _, plan = in_rounds(gpu_lib, srm.bam_of_records(recs), tmp_path, budget, bai=True, tile=tile, piece_bytes=5000)
    assert [r.end - r.first for r in plan] == [192, 192, 116] and rr["rounds"] == 3


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------
def refused(lib, bam: bytes, tmp_path, budget: int, name="x", bai=False, **kw):
    src, out = str(tmp_path / (name + ".in.bam")), str(tmp_path / (name + ".bam"))
    open(src, "wb").write(bam)
    with pytest.raises(host.NgsqError) as e:
        host.bam_to_sorted_bam(src, out, lib=lib, max_resident_bytes=budget, rounds=True, bai_path=out + ".bai" if bai else None, **kw)
    assert os.path.getsize(out) == 0, "something was written before the refusal"
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith(name + ".bam")) == [name + ".bam"]
    return e.value


def test_budgets_too_small(gpu_lib, tmp_path):
    per, survey_per = constants(gpu_lib)
    bam = bam_of(random_sam(175, 400, tmp_path), 7000)
    need = 400 * survey_per
    e = refused(gpu_lib, bam, tmp_path, need - 1, bai=True)
    assert e.code == ffi.ERR_LIMIT
    assert e.message == f"{CTX}--sort coordinate in rounds holds a key per record in device memory: {need} bytes needed, {need - 1} allowed"
    e = refused(gpu_lib, bam, tmp_path, 150 * survey_per, batch_records=100)      # in batches: as soon as the running count shows it
    assert e.message == f"{CTX}--sort coordinate in rounds holds a key per record in device memory: {200 * survey_per} bytes needed, {150 * survey_per} allowed"
    # one record beyond the budget: 30 records of which the one at sorted rank 12 takes 3000 bytes
    recs = [srm.raw_record(0, 10 * k, b"s%d" % k, 3000 - 38 if k == 12 else 0) for k in range(30)]
    big = len(recs[12])
    assert big + per > 2000 >= 30 * survey_per
    e = refused(gpu_lib, srm.bam_of_records(list(reversed(recs))), tmp_path, 2000)
    assert e.code == ffi.ERR_LIMIT
    assert e.message == f"{CTX}record 12 (0-based) of the sorted output alone takes {big + per} bytes of device memory, 2000 allowed"


def test_a_record_the_index_cannot_hold_is_refused_before_the_first_byte(gpu_lib, tmp_path):
    per, _ = constants(gpu_lib)
    refs = [(b"big", 1 << 29), (b"mid", 100_000)]
    recs = [rec(0, 1000 + 50 * k, name=b"a%d" % k) for k in range(300)] + [rec(1, 10 * k, name=b"b%d" % k) for k in range(100)]
    recs[250] = rec(0, (1 << 29) - 5, ((10, M),), name=b"beyond")               # ends behind 2^29
    recs[260] = rec(1, 2_000_000, name=b"far")                                    # more than 1 Mbp behind its sequence's end: a later rank
    bam = bam_with(refs, srm.shuffled(recs, 36))
    src, out = str(tmp_path / "m.in.bam"), str(tmp_path / "m.bam")
    open(src, "wb").write(bam)
    with pytest.raises(host.NgsqError) as e:
        host.bam_to_sorted_bam(src, out, lib=gpu_lib, bai_path=out + ".bai")
    assert e.value.message == f"{CTX}record 298 (0-based) of the sorted output {LIMIT_TEXT}"
    budget = srm.budget_for(srm.records_of(bam), per, 3)
    assert len(srm.plan_of(bam, budget, per)) == 3 and budget >= 400 * gpu_lib.ngsq_sort_survey_bytes_per_record()
    got = refused(gpu_lib, bam, tmp_path, budget, bai=True, batch_records=90)
    assert (got.code, got.message) == (ffi.ERR_LIMIT, e.value.message)
    in_rounds(gpu_lib, bam, tmp_path, budget, batch_records=90)                   # without the index the file converts, in rounds


def test_a_truncated_input_is_refused_with_the_ingests_message(gpu_lib, tmp_path, monkeypatch):
    stream = tm.bam_stream((HEAD + "".join(line(f0=f"q{k}", f3=str(60000 - k), f5="*", f9="ACGT" * 100, f10="*") for k in range(4000))).encode())
    good = b"".join(bamio.bgzf_block(stream[k:k + 3000], level=0) for k in range(0, len(stream), 3000)) + bamio.EOF_BLOCK
    cut = good[:len(good) * 3 // 4 + 7]
    src = str(tmp_path / "cut.in.bam")
    open(src, "wb").write(cut)
    said = ingest_message(gpu_lib, src, tmp_path)
    assert "truncated" in said
    monkeypatch.setenv("NGSQ_INGEST_RAW_MB", "1")                                 # the attempt overflows in the first chunk, the cut lies in a later one
    e = refused(gpu_lib, cut, tmp_path, 256 << 10, name="cut", bai=True, batch_records=500)
    assert e.message == CTX + said


# ---- 10. the command line -------------------------------------------------------------------------------------------------------------
def test_sort_memory_through_the_command_line(gpu_lib, ngs, tmp_path):
    def run(*args):
        return subprocess.run([ngs, *args], capture_output=True, timeout=300)
    bam = bam_of(random_sam(176, 2000, tmp_path), 7000)
    src, out, plain = str(tmp_path / "in.bam"), str(tmp_path / "out.bam"), str(tmp_path / "plain.bam")
    open(src, "wb").write(bam)
    per, survey_per = constants(gpu_lib)
    plan = srm.plan_of(bam, 64 << 10, per)
    r = run("convert", "--gzip", "device", "--sort", "coordinate", "--sort-memory", "64K", "--write-index", "-v", src, out)
    assert r.returncode == 0, r.stderr
    err = r.stderr.decode()
    assert "[ngs] convert: 2000 records in 1 batches and 1 slabs sorted in " in err
    assert (f"[ngs] convert: {len(plan)} rounds over {srm.walks(len(plan))} walks of the input, budget 65536 bytes, survey {2000 * survey_per} bytes in "
            in err) and len(plan) >= 2
    assert gzip.decompress(open(out, "rb").read()) == bsm.bam_stream(bam)
    bai = open(out + ".bai", "rb").read()
    os.rename(out + ".bai", out + ".kept")
    r = run("index", out)
    assert r.returncode == 0, r.stderr
    assert open(out + ".bai", "rb").read() == bai
    query = "chr1:1000-200000"
    r = run("view", "-m", "records-only", out, query)
    assert r.returncode == 0 and r.stdout == vm.expected_view(out, query, "records-only", bai) and r.stdout.count(b"\n") > 10
    r = run("convert", "--gzip", "device", "--sort", "coordinate", "--write-index", "-v", src, plain)
    assert r.returncode == 0, r.stderr
    assert " rounds over " not in r.stderr.decode() and "[ngs] convert: 2000 records in 1 batches and 1 slabs sorted in " in r.stderr.decode()
    assert open(plain, "rb").read() == open(out, "rb").read() and open(plain + ".bai", "rb").read() == bai
    sam = str(tmp_path / "in.sam")
    open(sam, "wb").write(random_sam(177, 50, tmp_path))
    r = run("convert", "--gzip", "device", "--sort", "coordinate", "--sort-memory", "1K", sam, str(tmp_path / "s.bam"))
    assert r.returncode == 1 and b"--sort coordinate holds the records in device memory: " in r.stderr and b" bytes needed, 1024 allowed" in r.stderr


# ---- 11. a random sweep ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_random_mixes(gpu_lib, tmp_path, seed):
    per, survey_per = constants(gpu_lib)
    rng = np.random.default_rng(9700 + seed)
    n = int(rng.integers(200, 2500))
    lens = [300_000, 70_000, 5_000]
    hb = random_batch(rng, n, lens, max_len=int(rng.integers(1, 400)))
    aux = [bamio.aligner_aux(rng, int(hb.cols["l_seq"][i])) if rng.random() < 0.7 else b"" for i in range(hb.n)]
    qn = [b"r" * int(rng.integers(1, 40)) + b"%d" % i for i in range(hb.n)]
    src = str(tmp_path / "r.bam")
    bamio.write_bam(src, hb, NAMES, lens, block_payload=int(rng.integers(500, 60000)), with_index=False, sort_order="unknown", names=qn, aux=aux,
                    level=int(rng.integers(0, 7)))
    bam = open(src, "rb").read()
    recs = srm.records_of(bam)
    want = 1 + seed % 8
    budget = max(srm.budget_for(recs, per, want), n * survey_per)
    batch = int(rng.choice([0, 63, 64, 65, int(rng.integers(20, n + 2))]))
    piece = int(rng.choice([0, 777, 4096, 65536, int(rng.integers(100, 200000))]))
    _, rep, rr, _, plan = in_rounds(gpu_lib, bam, tmp_path, budget, bai=True, batch_records=batch, piece_bytes=piece, tile=int(rng.choice([0, 100])))
    assert rep["records"] == n and rr["rounds"] == len(plan) <= want
