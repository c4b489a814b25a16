"""`ngs index` on the GPU: the device-built BAI equals the test-side model (tests/bai_model.py)
byte for byte, equals the synthetic writer's own index once the pseudo-bin is removed, is accepted by the project's
index reader, and `ngs qc` gives the same documents with it as with the writer's index."""
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
from tests.util import json_equal

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
