"""The device FASTA conversion at its chunk, tile and piece edges (tests/fasta_cases.py; the same inputs are held to their edges
without a GPU in tests/test_reference.py): file -> pinned pieces -> k_fasta_count / k_fasta_scan / k_fasta_emit -> the packed
copies -> Edits kernels, judged position by position with probe reads whose SEQ is the model's codes.

Equal codes count as `refs` for all sixteen codes, '=' and N included: the small cases run the oracle (fed
oracle_mod.fasta_codes of the text parsed in Python) on the same probes and it agrees, so the analytic rule stands for every
letter and is not narrowed to ACGT."""
import time

import pytest

from ngs_amd import ffi, host
from tests import fasta_cases as fc
from tests import generate_model as gm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T(gpu_lib):
    return int(gpu_lib.ngsq_fasta_tile_bytes())


def written(tmp_path, case, name="case.fa"):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(case.text)
    return p


def small_cases(T):
    yield "a", fc.case_thread_phases(T)
    for ending in fc.LAST_RECORDS:
        for residue in (0, 1):
            yield f"b_{ending}_{residue}", fc.case_tile_edges(T, ending, residue)
    yield "c", fc.case_thin_tiles(T)


SMALL = ["a"] + [f"b_{e}_{r}" for e in fc.LAST_RECORDS for r in (0, 1)] + ["c"]


@pytest.mark.parametrize("which", SMALL)
def test_terminators_record_ends_and_thin_tiles(gpu_lib, oracle_mod, tmp_path, T, which):
    """a, b, c with one-base probes: refs[p] == 0 exactly where byte p - 1 of the sequence is refused (a kept '\\r')"""
    case = dict(small_cases(T))[which]
    assert len(case.text) < 200_000
    st = fc.run_probes(gpu_lib, written(tmp_path, case), case, 1, "rows", oracle_mod=oracle_mod)
    want_cr = {"a": 32, "c": 0}.get(which, 2)                             # the lone '\r's and the first of each "\r\r\n"
    assert st["invalid_bytes"] == want_cr


@pytest.mark.parametrize("layout", ["rows", "offsets"])
def test_every_byte_value_on_the_device(gpu_lib, oracle_mod, tmp_path, T, layout):
    """d: the device's copy of the base table over all 255 values a sequence byte can have, and the sixteen letters in both
    cases on the window lanes"""
    case = fc.case_every_byte(T)
    st = fc.run_probes(gpu_lib, written(tmp_path, case), case, 1, layout, oracle_mod=oracle_mod)
    assert st["invalid_bytes"] == 3 * 224
    # the letters record alone, in reads of 7: no refused byte in the context, nothing takes the walk for one
    only = fc.Case(case.text, case.holds, names=["letters"])
    fc.run_probes(gpu_lib, written(tmp_path, case), only, 7, layout, oracle_mod=oracle_mod)


def test_many_records_with_empty_ones_between(gpu_lib, oracle_mod, tmp_path, T):
    """e: 1500 wanted records of 3000, empty ones in runs between them, LN below and above the records' lengths"""
    case = fc.case_many_records(T)
    st = fc.run_probes(gpu_lib, written(tmp_path, case), case, 1, "rows", oracle_mod=oracle_mod)
    assert (st["sequences"], st["shorter"], st["longer"]) == (1500, 40, 40)


@pytest.mark.parametrize("extra", [1, 100])
@pytest.mark.parametrize("W,layout", [(150, "rows"), (149, "offsets")])
def test_a_record_of_1025_tiles(gpu_lib, tmp_path, T, W, layout, extra):
    """f: the second round of k_fasta_scan and its carry: 1024 T + 1 bytes of text, whose tile 1024 holds only the last newline,
    and 1024 T + 100, whose tile 1024 holds 98 bases that go where the carry says"""
    case = fc.case_scan_rounds(T, extra)
    st = fc.run_probes(gpu_lib, written(tmp_path, case), case, W, layout)
    assert st["text_bytes"] == 1024 * T + extra + 2 * 710


@pytest.fixture(scope="module")
def two_pieces(tmp_path_factory, T):
    case = fc.case_two_pieces(T)
    path = written(tmp_path_factory.mktemp("g"), case)
    return case, path, fc.model_of(case)


@pytest.mark.parametrize("threads", [1, 4])
def test_two_pieces_and_two_turns_of_the_grid(gpu_lib, two_pieces, T, threads):
    """g: a record in two upload pieces whose tiles outnumber the grid (16 blocks on each compute unit; the library does not
    report the device's count, so the bound is the 256 of an MI355X)"""
    case, path, model = two_pieces
    assert -(-case.holds["text_bytes"] // T) > 16 * 256 and case.holds["text_bytes"] > fc.PIECE
    t0 = time.time()
    st = fc.run_probes(gpu_lib, path, case, 150, "rows", fasta_threads=threads, model=model)
    print(f"case g, fasta_threads {threads}: {time.time() - t0:.2f} s (load {st['total_s']:.3f} s, kernels {st['device_s'] * 1e3:.2f} ms)")
    assert st["text_bytes"] == case.holds["text_bytes"] + 2 * 710


def test_refused_bytes_at_the_lists_capacity(gpu_lib, oracle_mod, tmp_path, T):
    """h: exactly 65 536 refused bytes load, and each is found again"""
    case = fc.case_refused_capacity(T, fc.BAD_CAP)
    refused = [1, 2 * 20_000 + 1, 2 * 32_768 + 1, 2 * 50_001 + 1, 2 * fc.BAD_CAP - 1]   # the first, three in the middle, the last
    only = sorted([(0, p) for p in refused] + [(0, p - 1) for p in refused])             # and the base in front of each
    st = fc.run_probes(gpu_lib, written(tmp_path, case), case, 1, "rows", oracle_mod=oracle_mod, only=only)
    assert st["invalid_bytes"] == fc.BAD_CAP == 65536


def test_one_refused_byte_more_than_the_list_holds(gpu_lib, tmp_path, T):
    """h: 65 537 refused bytes: the load fails on the host after the kernels, with both numbers, and so does a batch after it"""
    case = fc.case_refused_capacity(T, fc.BAD_CAP + 1)
    names, lens, seqs, codes, _ = fc.model_of(case)
    hb = fc.probe_batch(codes, 1, "rows", only=[(0, 0)])[0]
    with host.QcContext(lens, facets=ffi.FACET_EDITS, ref_fasta=written(tmp_path, case), ref_names=names, lib=gpu_lib) as gpu:
        with pytest.raises(host.NgsqError) as e:
            gpu.reference_wait()
        assert e.value.code == ffi.ERR_LIMIT
        assert "the reference FASTA holds 65537 bytes that are no base letters; the loader keeps the positions of 65536" in str(e.value)
        with pytest.raises(host.NgsqError) as e:
            gpu.process_batch(hb)
        assert e.value.code == ffi.ERR_LIMIT and "65537" in str(e.value)


@pytest.mark.parametrize("which", SMALL)
def test_raw_mode_keeps_the_letters_of_the_same_files(gpu_lib, tmp_path, T, which):
    """i: k_fasta_emit<RAW> on the files of a, b and c (base letters in mixed case) through `ngs generate` without
    substitutions: 2000 pairs of 20-base reads, byte for byte the model's.  Fragments are 42 bases, the shortest a record must
    have, so that one can end on a record's last base."""
    from tests.test_generate_gpu import check_against_model
    case = dict(small_cases(T))[which]
    path = written(tmp_path, case, f"{which}.fa")
    want, _ = check_against_model(gpu_lib, [(path, 10 ** 9, 2.0, 0.0, 20, 1)], tmp_path, seed=31, n=2000)
    picked = {gm.parse_fasta(case.text)[s][0].decode() for _, s, _, _ in want.picks}
    eligible = {nm for nm, s in fc.sequences(case.text).items() if len(s) >= 42}
    assert picked == eligible and len(eligible) >= 4                     # every record long enough was drawn from
