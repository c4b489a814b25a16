"""`ngs index` on the GPU: the device-built BAI equals the test-side model (tests/bai_model.py)
byte for byte, equals the synthetic writer's own index once the pseudo-bin is removed, is accepted by the project's
index reader, and `ngs qc` gives the same documents with it as with the writer's index.  Both sides of what a BAI can hold
(the last kept window of a sequence, position 2^29, the header's sequence ids), and empty BGZF members at the ends of ingest
chunks."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from ngs_amd import build, ffi, host
from ngs_amd.genome_shape import grch38_no_alt
from tests import bai_model as bm
from tests import bamio
from tests.test_index import LENS, NAMES, index_sorted_batch, reorder
from tests.util import batch_from_records, json_equal

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GENOME = "GRCh38_no_alt_AnalysisSet"


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def run(ngs, *args, env=None):
    return subprocess.run([ngs, *args], capture_output=True, text=True, env=env, timeout=900)


@pytest.mark.parametrize("seed,n,payload", [(11, 5000, 60000), (12, 20000, 3000), (13, 3000, 500), (14, 1, 60000)])
def test_bamio_files_equal_the_model(gpu_lib, tmp_path, seed, n, payload):
    hb = index_sorted_batch(seed, n)
    path = str(tmp_path / "r.bam")
    bamio.write_bam(path, hb, NAMES, LENS, block_payload=payload, with_index=False)
    rep = host.build_bam_index(path, lib=gpu_lib)
    got = open(path + ".bai", "rb").read()
    assert got == bm.expected_bai(path)
    assert rep["records"] == n
    c = hb.cols
    assert rep["n_no_coor"] == int(((c["ref_id"] < 0) | (c["pos"] < 0)).sum())
    assert gpu_lib.ngsq_bam_check_index(path.encode()) == 0


def test_empty_file(gpu_lib, tmp_path):
    hb = index_sorted_batch(15, 3)
    path = str(tmp_path / "e.bam")
    bamio.write_bam(path, hb.slice(0, 0), NAMES, LENS, with_index=False)
    rep = host.build_bam_index(path, lib=gpu_lib)
    assert rep["records"] == 0
    assert open(path + ".bai", "rb").read() == bm.expected_bai(path)


@pytest.mark.parametrize("name", ["hand_spec.bam", "hand_longcigar.bam"])
def test_hand_files_equal_the_model(gpu_lib, tmp_path, name):
    """An empty member between records, records straddling blocks, an unplaced record; a 70 000-op CIGAR in a CG tag."""
    path = str(tmp_path / name)
    shutil.copy(os.path.join(GOLDEN, name), path)
    host.build_bam_index(path, lib=gpu_lib)
    assert open(path + ".bai", "rb").read() == bm.expected_bai(path)


def write_genome_file(lib, path, n, style=ffi.SYNTH_FILE_ALIGNER):
    names, lens, _ = grch38_no_alt()
    cfg = host.synth_config(n, read_len=150, genome=lens, file_style=style, lib=lib)
    arr = (C.c_char_p * len(names))(*[x.encode() for x in names])
    assert lib.ngsq_synth_write_bam_named(C.byref(cfg), arr, path.encode(), n, 1, 0) == 0, lib.ngsq_bam_last_error()
    return names, lens


def test_genome_file_over_several_chunks(gpu_lib, tmp_path, monkeypatch):
    """The 195-sequence header, records over all of it, 16 MiB ingest chunks: the index carries across batches and chunks."""
    monkeypatch.setenv("NGSQ_INGEST_RAW_MB", "16")
    path = str(tmp_path / "g.bam")
    names, _ = write_genome_file(gpu_lib, path, 300_000)
    writer = open(path + ".bai", "rb").read()
    os.remove(path + ".bai")
    rep = host.build_bam_index(path, lib=gpu_lib)
    got = open(path + ".bai", "rb").read()
    assert rep["records"] == 300_000
    assert os.path.getsize(path) > 3 * (4 << 20)           # several compressed chunks (a quarter of the raw size each)
    assert got == bm.expected_bai(path)
    assert bm.strip_meta(got) == writer
    assert gpu_lib.ngsq_bam_check_index(path.encode()) == 0
    starts = np.zeros(len(names), dtype=np.uint64)
    n_bins = C.c_uint64()
    assert gpu_lib.ngsq_bam_index_ref_starts(path.encode(), len(names), starts.ctypes.data_as(ffi.u64p), C.byref(n_bins)) == 0
    refs, _ = bm.parse(got)
    assert n_bins.value == sum(len([b for b in bins if b != bm.META_BIN]) for bins, _ in refs)


def test_out_of_order_records_fail_and_leave_nothing(gpu_lib, ngs, tmp_path):
    hb = index_sorted_batch(16, 4000, weird=False)
    order = np.arange(hb.n)
    order[[1500, 2500]] = order[[2500, 1500]]
    path = str(tmp_path / "u.bam")
    bamio.write_bam(path, reorder(hb, order), NAMES, LENS, with_index=False)
    with pytest.raises(host.NgsqError) as e:
        host.build_bam_index(path, lib=gpu_lib)
    assert e.value.code == ffi.ERR_UNSORTED
    try:
        bm.expected_bai(path)
        want = None
    except bm.Unsorted as u:
        want = u.index
    assert f"record {want} (0-based)" in str(e.value)
    assert not os.path.exists(path + ".bai")
    r = run(ngs, "index", path)
    assert r.returncode == 1 and "out of coordinate order" in r.stderr
    assert not os.path.exists(path + ".bai")
    assert not [f for f in os.listdir(tmp_path) if f.startswith("u.bam.bai")]


def limit_file(path, case, over):
    """A sorted file whose record `at` reaches the edge the case names (over: one base beyond it) with an N skip: (at, header
    names, lengths).  `window`: on sequence 0 of the three, the last base of the last window the index keeps for it, with
    records of sequence 1 behind it; `2^29`: on a sequence of that length; `ref_id`: the id one behind the header's last."""
    rec = lambda ref, pos, cigar="4M", flag=0: dict(flag=flag, mapq=60, ref_id=ref, pos=pos, mate_ref_id=ref, tlen=0,  # noqa: E731
                                                    cigar=cigar, seq="ACGT", qual=[30, 31, 32, 33])
    if case == "window":
        names, lens = NAMES, LENS
        edge = bm.lin_cap(LENS[0]) * 16384                         # 83 windows: the first base that has none
        recs = [rec(0, 10 * k) for k in range(300)] + [rec(0, 200_000, "4M100000N"), rec(0, 299_990)]
        at = len(recs)
        recs.append(rec(0, 1_000_000, f"2M{edge - 1_000_000 - 4 + over}N2M"))
        recs += [rec(0, 1_000_000 + k) for k in range(1, 40)]
        recs += [rec(1, 7 * k, flag=4 * (k % 5 == 0)) for k in range(400)] + [rec(2, 4000), rec(-1, -1, "*", 4)]
    elif case == "2^29":
        names, lens = ["big", "small"], [1 << 29, 1000]
        recs = [rec(0, 10 * k) for k in range(100)]
        at = len(recs)
        recs.append(rec(0, (1 << 29) - 1000, f"3M{990 + over}N7M"))
        recs += [rec(1, k) for k in range(50)] + [rec(-1, -1, "*", 4)] * 3
    else:
        names, lens = NAMES, LENS
        recs = [rec(0, 10 * k) for k in range(100)] + [rec(1, k) for k in range(100)] + [rec(2, k) for k in range(100)]
        at = len(recs) - (0 if over else 1)
        if over:
            recs.append(rec(len(NAMES), 5))
        recs += [rec(-1, -1, "*", 4)] * 2
    bamio.write_bam(path, batch_from_records(recs), names, lens, block_payload=3000, with_index=False)
    return at, names, lens


@pytest.mark.parametrize("case", ["window", "2^29", "ref_id"])
def test_the_last_record_a_bai_can_hold(gpu_lib, tmp_path, case):
    path = str(tmp_path / "ok.bam")
    at, names, lens = limit_file(path, case, 0)
    host.build_bam_index(path, lib=gpu_lib)
    got, want = open(path + ".bai", "rb").read(), bm.expected_bai(path)
    refs, _ = bm.parse(got)
    wrefs, _ = bm.parse(want)
    recs, _, _ = bm.read_records(path)
    if case == "window":      # the last window of sequence 0's slice is the record's; the slice of sequence 1 lies right behind it
        assert len(refs[0][1]) == bm.lin_cap(lens[0]) == 83 and refs[0][1][82] == recs[at].v0
        assert refs[1][1] == wrefs[1][1] and len(refs[1][1]) == 1 and refs[1][1][0] > recs[at].v0
        assert refs[1][0][bm.META_BIN] == wrefs[1][0][bm.META_BIN]
    if case == "2^29":
        assert len(refs[0][1]) == 32768 and refs[0][1][32767] == recs[at].v0 and 4681 + 32767 in refs[0][0]
    assert got == want
    assert gpu_lib.ngsq_bam_check_index(path.encode()) == 0


@pytest.mark.parametrize("case", ["window", "2^29", "ref_id"])
def test_one_base_further_is_refused_and_leaves_nothing(gpu_lib, ngs, tmp_path, case):
    path = str(tmp_path / "over.bam")
    at, _, _ = limit_file(path, case, 1)
    with pytest.raises(bm.Limit) as want:
        bm.expected_bai(path)
    assert want.value.index == at
    with pytest.raises(host.NgsqError) as e:
        host.build_bam_index(path, lib=gpu_lib)
    assert e.value.code == ffi.ERR_LIMIT
    assert f"record {at} (0-based)" in str(e.value) and str(want.value) in str(e.value)
    assert not os.path.exists(path + ".bai")
    r = run(ngs, "index", path)
    assert r.returncode == 1 and f"record {at} (0-based) cannot be held by a BAI" in r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("over.bam.bai")]


def test_empty_members_at_the_ends_of_ingest_chunks(gpu_lib, tmp_path, monkeypatch):
    """Every third record is followed by an empty member, and a 1 MiB ingest buffer makes chunks of at most half of it
    (`out_limit` of reader_main, bam_device_reader.cpp): the position behind a record that ends its block is the empty
    member's, also where that member is the first of the next chunk or the last of its own."""
    monkeypatch.setenv("NGSQ_INGEST_RAW_MB", "1")
    hb = index_sorted_batch(17, 20000)
    path = str(tmp_path / "e.bam")
    bamio.write_bam(path, hb, NAMES, LENS, block_payload=3000, with_index=False, empty_members=0.3, rng=np.random.default_rng(18))
    blocks, data, _ = bm.read_blocks(path)
    assert sum(b.isize == 0 for b in blocks) > 5000 and len(data) > 3 << 19          # (several chunks)
    rep = host.build_bam_index(path, lib=gpu_lib)
    assert rep["records"] == 20000
    assert open(path + ".bai", "rb").read() == bm.expected_bai(path)
    assert gpu_lib.ngsq_bam_check_index(path.encode()) == 0


def test_cli_index_then_qc_gives_the_writer_s_documents(gpu_lib, ngs, tmp_path):
    """Round trip: the synthetic writer's file with its own index, and a copy whose index `ngs index` wrote."""
    src = str(tmp_path / "a" / "s.bam")
    os.makedirs(os.path.dirname(src))
    write_genome_file(gpu_lib, src, 200_000, style=ffi.SYNTH_FILE_REALISTIC)
    copy = str(tmp_path / "b" / "s.bam")
    os.makedirs(os.path.dirname(copy))
    shutil.copy(src, copy)
    r = run(ngs, "index", copy)
    assert r.returncode == 0, r.stderr
    assert bm.strip_meta(open(copy + ".bai", "rb").read()) == open(src + ".bai", "rb").read()
    for k, extra in enumerate(([], ["-n", "50000"], ["--gpus", "2", "--same-device"])):
        docs = []
        for bam in (src, copy):
            out = tmp_path / f"o{k}_{os.path.basename(os.path.dirname(bam))}"
            r = run(ngs, "qc", bam, GENOME, "-o", str(out), *extra)
            assert r.returncode == 0, r.stderr[-2000:]
            docs.append(json.load(open(out / "s.bam.results.json")))
        json_equal(docs[1], docs[0])
