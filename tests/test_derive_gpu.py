"""`ngs derive instrument` on the GPU: the two sets the device collects equal the test-side model's
(tests/derive_model.py) exactly -- one name over many batches, thousands of records from dozens of instruments and flowcells
with absent names, empty segments and the longest names, a table too small for them, thousands of names that are all new in
one batch -- the first bad name is the one reported, the `-n` rule, an empty file, the hand-assembled files, a synthetic
file, and the command line prints the model's document byte for byte.  Files of several ingest chunks (the name of the record
a chunk's end cuts is read from the carried bytes, a bad one copied out of them), and names first seen in the last lane of a
launch, the first lane of the next, and both."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from ngs_amd import build, ffi, host
from tests import bamio
from tests import derive_model as dm
from tests import sam_model as sm
from tests.util import derive_check as check
from tests.util import illumina, random_batch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["chr1", "chr2", "chr3"]
LENS = [300_000, 70_000, 5_000]
NO_MATCH = {"succeeded": False, "instruments": None, "confidence": "unknown", "evidence": None,
            "comment": "no matching instruments were found"}
NOVASEQ_HIGH = {"succeeded": True, "instruments": ["NovaSeq"], "confidence": "high", "evidence": "instrument and flowcell id",
                "comment": None}


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def run(ngs, *args):
    return subprocess.run([ngs, *args], capture_output=True, timeout=900)


def write(path, names, seed=1, block_payload=60000):
    hb = random_batch(np.random.default_rng(seed), max(len(names), 1), LENS, max_len=40).slice(0, len(names))
    bamio.write_bam(path, hb, NAMES, LENS, block_payload=block_payload, names=names)
    return path


def test_one_instrument_over_many_batches(gpu_lib, tmp_path):
    rng = np.random.default_rng(31)
    path = write(str(tmp_path / "a.bam"), [bamio.aligner_name(rng) for _ in range(3000)])
    doc, rep = check(gpu_lib, path, batch_records=97)
    assert doc == NOVASEQ_HIGH
    assert rep["batches"] == (3000 + 96) // 97
    # both names are new in the first batch only: its waves append them, the other batches find them and append nothing
    assert rep["entries"] <= 2 * 2


def mixed_names(rng, n):
    """n names drawn from 40 instruments x 50 flowcells, with 5-segment names, absent names, empty segments, an instrument of 200
    bytes and, at index 7, the longest name: 254 bytes."""
    ins = [b"A%05d" % rng.integers(0, 100000) for _ in range(30)] + [b"HWI-ST%d" % rng.integers(100, 100000) for _ in range(9)] + [b"x" * 200]
    fcs = [b"H" + bytes(rng.choice(list(b"ABCXYZ0123456789"), 5).tolist()) + b"SXX" for _ in range(49)] + [b""]
    names = []
    for _ in range(n):
        r = rng.random()
        if r < 0.02:
            names.append(b"*")
        elif r < 0.03:
            names.append(b"::::" if r < 0.025 else b"::::::")
        elif r < 0.2:
            names.append(illumina(rng, ins[rng.integers(0, 40)]))
        else:
            names.append(illumina(rng, ins[rng.integers(0, 40)], fcs[rng.integers(0, 50)]))
    names[7] = (b"K00321:9:" + b"F" * 254)[:254 - 8] + b":1:2:3:4"
    return names


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    """20 000 records drawn from 40 instruments x 50 flowcells, with 5-segment names, absent names, empty segments, a 254-byte
    name and an instrument of 200 bytes."""
    rng = np.random.default_rng(32)
    names = mixed_names(rng, 20000)
    names[12345] = b"y" * 200 + b":1:2:3:" + b"9" * 47                            # 254 bytes again, 5 segments
    assert len(names[7]) == 254 and len(names[12345]) == 254 and names[7].count(b":") == 6
    path = str(tmp_path_factory.mktemp("derive") / "mixed.bam")
    return write(path, names, seed=33, block_payload=7000)


def test_mixed_names_equal_the_model(gpu_lib, mixed):
    doc, rep = check(gpu_lib, mixed, batch_records=333)
    assert rep["instruments"] >= 40 and rep["flowcells"] >= 48 and rep["skipped"] > 100
    assert rep["batches"] == (20000 + 332) // 333


def test_a_table_too_small_for_the_names(gpu_lib, mixed):
    """16 slots for some 45 instruments and 52 flowcells: most names never get a slot and are appended again by every wave
    that meets them.  The sets are the same."""
    _, small = check(gpu_lib, mixed, batch_records=333, table_slots=16)
    _, default = check(gpu_lib, mixed, batch_records=333)
    assert small["candidates"] > 0 and small["entries"] > default["entries"]
    _, two = check(gpu_lib, mixed, batch_records=4096, table_slots=2)
    assert two["candidates"] > 0
    with pytest.raises(host.NgsqError) as e:
        host.derive_instrument(mixed, table_slots=24, lib=gpu_lib)
    assert e.value.code == ffi.ERR_INVALID_ARGUMENT and "power of two" in str(e.value)


def test_thousands_of_names_new_in_one_batch(gpu_lib, tmp_path):
    """5 000 distinct instruments, all first seen in batch 0 (every lane of every wave claims a slot or appends a candidate at
    once), then repeated in the later batches, which find them."""
    rng = np.random.default_rng(34)
    ins = [b"M%05d" % k for k in rng.permutation(100000)[:5000]]
    names = [illumina(rng, x, b"A0B1C") for x in ins]
    names += [illumina(rng, ins[rng.integers(0, 5000)], b"A0B1C") for _ in range(7000)]
    path = write(str(tmp_path / "d.bam"), names, seed=35, block_payload=20000)
    doc, rep = check(gpu_lib, path, batch_records=5000)
    assert rep["instruments"] == 5000 and rep["flowcells"] == 1 and rep["batches"] == 3
    assert doc == {"succeeded": True, "instruments": ["MiSeq"], "confidence": "high", "evidence": "instrument and flowcell id", "comment": None}
    _, rep = check(gpu_lib, path, batch_records=5000, table_slots=1024)     # fewer slots than names
    assert rep["candidates"] > 0


@pytest.mark.parametrize("first,second,batch", [(1203, 1300, 500), (700, 2500, 500), (0, 2999, 1000), (2999, 2999, 64)])
def test_the_first_bad_name_is_reported(gpu_lib, tmp_path, first, second, batch):
    """Names of 1, 6 and 8 segments, two in one batch or in different batches: the message names the first in file order, and
    `-n` short of it succeeds."""
    rng = np.random.default_rng(36)
    names = [bamio.aligner_name(rng) for _ in range(3000)]
    bad = [b"read/1", b"A00741:215:HG7WKDSXX:1:1101:1000", b"A00741:215:HG7WKDSXX:1:1101:1000:2000:extra"]
    names[first] = bad[first % 3]
    names[second] = bad[(first + 1) % 3] if second != first else names[first]
    path = write(str(tmp_path / "e.bam"), names, seed=37, block_payload=9000)
    with pytest.raises(dm.BadName) as want:
        dm.expected(path)
    assert want.value.name == names[first]
    with pytest.raises(host.NgsqError) as e:
        host.derive_instrument(path, batch_records=batch, lib=gpu_lib)
    assert e.value.code == ffi.ERR_INVALID_ARGUMENT
    assert str(e.value).endswith("Could not parse Illumina-formatted query names for read: " + names[first].decode())
    with pytest.raises(host.NgsqError) as e:       # -n first: records 0 .. first are examined
        host.derive_instrument(path, batch_records=batch, max_records=first + 1, lib=gpu_lib)
    assert str(e.value).endswith("for read: " + names[first].decode())
    if first:                                      # -n first - 1: the bad name is the record behind the last one examined
        doc, rep = check(gpu_lib, path, n=first - 1, batch_records=batch) if first > 1 else (None, None)
        got = host.derive_instrument(path, batch_records=batch, max_records=first, lib=gpu_lib)
        assert got[2] == NOVASEQ_HIGH and got[3]["records"] == first


def test_num_records_examines_one_more(gpu_lib, tmp_path):
    """A new instrument at index N is seen with -n N; at index N + 1 it is not."""
    rng = np.random.default_rng(38)
    names = [bamio.aligner_name(rng) for _ in range(2000)]
    N = 777
    names[N] = illumina(rng, b"D00123", b"HG7WKDSXX")
    names[N + 300] = illumina(rng, b"E00456")
    path = write(str(tmp_path / "f.bam"), names, seed=39, block_payload=5000)
    for batch in (100, 778, 4096):
        doc, _ = check(gpu_lib, path, n=N, batch_records=batch)
        assert doc["comment"] == "multiple instruments were detected in this file via the instrument id"
        doc, rep = check(gpu_lib, path, n=N - 1, batch_records=batch)
        assert doc == NOVASEQ_HIGH and rep["records"] == N and rep["instruments"] == 1
    _, rep = check(gpu_lib, path, n=5000)          # more than the file holds: all of them
    assert rep["records"] == 2000 and rep["instruments"] == 3
    _, rep = check(gpu_lib, path, n=1)
    assert rep["records"] == 2


def write_long(path, names, seed=43):
    """Records of 1 000 to 20 000 bases with an aligner's tags: 16 kB each, half a MiB of them per 1 MiB ingest buffer."""
    rng = np.random.default_rng(seed)
    hb = random_batch(rng, len(names), LENS, max_len=20_000, min_len=1000, weird=False)
    aux = [bamio.aligner_aux(rng, int(hb.cols["l_seq"][i])) for i in range(hb.n)]
    bamio.write_bam(path, hb, NAMES, LENS, names=names, aux=aux, with_index=False)
    return path


@pytest.fixture(scope="module")
def mixed_long(tmp_path_factory):
    names = mixed_names(np.random.default_rng(42), 260)
    return write_long(str(tmp_path_factory.mktemp("derive_long") / "long.bam"), names), names


def batch_sizes(lib, path):
    """The records of the device ingest's successive batches, each as large as the chunk allows."""
    sizes = []
    with host._reader_and_plain_context(lib, path, 0) as (bam, ctx):
        while True:
            bt = ffi.Batch()
            assert lib.ngsq_bam_next_batch_device(bam, ctx, 1 << 22, C.byref(bt)) == 0, lib.ngsq_bam_last_error()
            if not bt.n_records:
                return sizes
            sizes.append(int(bt.n_records))


def test_files_of_several_ingest_chunks(gpu_lib, mixed_long, monkeypatch):
    monkeypatch.setenv("NGSQ_INGEST_RAW_MB", "1")
    path, names = mixed_long
    inflated = len(dm.bai_model.read_blocks(path)[1])
    assert inflated > 7 << 19
    _, rep = check(gpu_lib, path)
    assert rep["batches"] >= inflated // 2 ** 20 and rep["batches"] >= 4 and rep["records"] == len(names)
    _, two = check(gpu_lib, path, table_slots=2)
    assert two["batches"] == rep["batches"] and two["candidates"] > 0


@pytest.mark.parametrize("which", [1, -1])
def test_a_bad_name_in_the_record_a_chunk_s_end_cuts(gpu_lib, mixed_long, tmp_path, monkeypatch, which):
    """The first record of every batch but the first is the one the end of the chunk in front cut: its bytes lie in front of
    the chunk's own, and the message's name is copied out of them."""
    monkeypatch.setenv("NGSQ_INGEST_RAW_MB", "1")
    path, names = mixed_long
    sizes = batch_sizes(gpu_lib, path)
    assert len(sizes) >= 4 and sum(sizes) == len(names)
    cut = np.cumsum(sizes)[:-1]                                   # the first record of batches 1 ..
    at = int(cut[0 if which > 0 else -1])
    # the record does straddle a block boundary (a chunk ends on one): it is the cut record, not one that happens to come first
    blocks, stream, _ = dm.bai_model.read_blocks(path)
    _, _, _, p = sm.read_bam(path)
    for _ in range(at):
        p += 4 + struct.unpack_from("<I", stream, p)[0]
    end = p + 4 + struct.unpack_from("<I", stream, p)[0]
    assert any(p < b.out < end for b in blocks)
    bad = list(names)
    bad[at] = b"x" if names[at] == b"*" else names[at].replace(b":", b"_")       # one segment, as many bytes: the same chunks
    planted = write_long(str(tmp_path / "cut.bam"), bad)
    assert batch_sizes(gpu_lib, planted) == sizes
    with pytest.raises(dm.BadName) as want:
        dm.expected(planted)
    assert want.value.name == bad[at]
    with pytest.raises(host.NgsqError) as e:
        host.derive_instrument(planted, lib=gpu_lib)
    assert e.value.code == ffi.ERR_INVALID_ARGUMENT and str(e.value).endswith(str(want.value))
    got = host.derive_instrument(planted, max_records=at, lib=gpu_lib)           # short of it: fine
    assert got[3]["records"] == at


@pytest.mark.parametrize("B", [63, 64, 65, 255, 256, 257])
def test_names_first_seen_at_the_edges_of_waves_blocks_and_launches(gpu_lib, tmp_path, B):
    """Batches of B records: a new instrument in the last lane of the first launch, another in the first lane of the second, a
    fourth in the last lane of the second and the first lane of the third at once."""
    rng = np.random.default_rng(44)
    names = [illumina(rng, b"A00741", b"HG7WKDSXX") for _ in range(4 * B)]
    names[B - 1] = illumina(rng, b"D00123", b"HG7WKDSXX")
    names[B] = illumina(rng, b"E00456", b"HG7WKDSXX")
    names[2 * B - 1] = illumina(rng, b"M01234", b"HG7WKDSXX")
    names[2 * B] = illumina(rng, b"M01234", b"HG7WKDSXX")
    path = write(str(tmp_path / "w.bam"), names, seed=45)
    _, rep = check(gpu_lib, path, batch_records=B)
    assert rep["records"] == 4 * B and rep["batches"] == 4
    assert rep["instruments"] == 4 and rep["flowcells"] == 1 and rep["entries"] >= 5


def test_header_only_file(gpu_lib, tmp_path):
    path = write(str(tmp_path / "g.bam"), [])
    doc, rep = check(gpu_lib, path)
    assert doc == NO_MATCH and rep["records"] == 0 and rep["batches"] == 0 and rep["entries"] == 0


@pytest.mark.parametrize("name", ["hand_spec.bam", "hand_longcigar.bam"])
def test_hand_files(gpu_lib, name):
    """Whatever the model says of them: their names are not Illumina names, so the first one is reported."""
    path = os.path.join(GOLDEN, name)
    try:
        dm.expected(path, lookup=lambda which, q: host.derive_lookup(which, q, gpu_lib))
    except dm.BadName as want:
        with pytest.raises(host.NgsqError) as e:
            host.derive_instrument(path, lib=gpu_lib)
        assert str(e.value).endswith(str(want))
    else:
        check(gpu_lib, path)


def test_synthetic_file_is_a_novaseq(gpu_lib, tmp_path):
    """The synthetic writer's aligner style carries Illumina names (its plain style says r0, r1, ...)."""
    path = str(tmp_path / "s.bam")
    n = 200_000
    cfg = host.synth_config(n, file_style=ffi.SYNTH_FILE_ALIGNER)
    assert gpu_lib.ngsq_synth_write_bam(C.byref(cfg), path.encode(), n, 1, 0) == 0, gpu_lib.ngsq_bam_last_error()
    ins, fcs, doc, rep = host.derive_instrument(path, batch_records=50_000, lib=gpu_lib)
    assert (ins, fcs) == ([b"A00741"], [b"HG7WKDSXX"]) and doc == NOVASEQ_HIGH
    # (batch_records is an upper bound: the ingest ends a batch early where a chunk of the file ends, so 4 is the fewest)
    assert rep["records"] == n and rep["skipped"] == 0 and rep["batches"] >= 4
    assert rep["kernel_ms"] > 0 and rep["total_ms"] >= rep["scan_ms"] > 0


def test_a_reader_that_has_been_read_from_is_refused(gpu_lib, tmp_path):
    rng = np.random.default_rng(40)
    path = write(str(tmp_path / "r.bam"), [bamio.aligner_name(rng) for _ in range(100)])
    with host._reader_and_plain_context(gpu_lib, path, 0) as (bam, ctx):
        bt = ffi.Batch()
        assert gpu_lib.ngsq_bam_next_batch_device(bam, ctx, 10, C.byref(bt)) == 0
        names = C.c_void_p()
        assert gpu_lib.ngsq_bam_derive_instrument(bam, ctx, 0, 0, 0, C.byref(names), None) == ffi.ERR_STATE
        assert not names.value


def test_command_line(gpu_lib, ngs, mixed, tmp_path):
    """stdout is the model's document byte for byte, without a final newline; a bad name is `Error: ...` and exit 1."""
    lookup = lambda which, q: host.derive_lookup(which, q, gpu_lib)  # noqa: E731
    r = run(ngs, "derive", "instrument", mixed)
    assert r.returncode == 0, r.stderr
    assert r.stdout == dm.document(dm.expected(mixed, 0, lookup)[3]).encode()
    r = run(ngs, "-q", "derive", "instrument", "-n", "5", "-t", "2", mixed)
    assert r.returncode == 0 and r.stdout == dm.document(dm.expected(mixed, 5, lookup)[3]).encode()
    rng = np.random.default_rng(41)
    names = [bamio.aligner_name(rng) for _ in range(300)]
    path = write(str(tmp_path / "ok.bam"), names)
    r = run(ngs, "derive", "instrument", "--device", "0", path)
    assert r.returncode == 0 and r.stdout == dm.document(NOVASEQ_HIGH).encode() and not r.stdout.endswith(b"\n")
    names[200] = b"not an illumina name"
    path = write(str(tmp_path / "bad.bam"), names)
    r = run(ngs, "derive", "instrument", path)
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.endswith(b"Error: Could not parse Illumina-formatted query names for read: not an illumina name\n")
    r = run(ngs, "derive", "instrument", "-n", "199", path)
    assert r.returncode == 0 and r.stdout == dm.document(NOVASEQ_HIGH).encode()
    r = run(ngs, "derive", "instrument", "-n", "200", path)
    assert r.returncode == 1
