"""`ngs convert <BAM> <SAM>` on the GPU: the text the device formats equals the test-side model
(tests/sam_model.py) byte for byte -- on the hand-assembled files, synthetic files over hundreds of batches, adversarial tag
data, 100 kb reads, 70 000-operation CIGARs, float arrays of random bit patterns, an empty file and every `-n` case -- the
command line writes what the library writes, and every kind of record without SAM text ends the run with its message."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from ngs_amd import build, ffi, host
from ngs_amd.genome_shape import grch38_no_alt
from tests import bamio
from tests import sam_model as sm
from tests.util import batch_from_records, random_batch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["chr1", "chr2", "chr3"]
LENS = [300_000, 70_000, 5_000]


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def run(ngs, *args):
    return subprocess.run([ngs, *args], capture_output=True, text=True, timeout=900)


def convert(lib, path, out, **kw):
    rep = host.bam_to_sam(path, out, lib=lib, **kw)
    return open(out, "rb").read(), rep


def assert_same(got: bytes, want: bytes):
    if got != want:  # the first differing line, not two megabytes of text
        gl, wl = got.split(b"\n"), want.split(b"\n")
        for k, (a, b) in enumerate(zip(gl, wl)):
            assert a == b, f"line {k}:\n got  {a[:400]!r}\n want {b[:400]!r}"
        assert len(gl) == len(wl), f"{len(gl)} lines, want {len(wl)}"


@pytest.mark.parametrize("name", ["hand_spec.bam", "hand_longcigar.bam"])
def test_hand_files(gpu_lib, tmp_path, name):
    got, rep = convert(gpu_lib, os.path.join(GOLDEN, name), str(tmp_path / "o.sam"))
    assert_same(got, sm.expected_sam(os.path.join(GOLDEN, name)))
    if name == "hand_spec.bam":
        assert got == open(os.path.join(GOLDEN, "hand_spec.sam"), "rb").read()
    assert rep["records"] == sm.count_records(os.path.join(GOLDEN, name))
    assert rep["header_bytes"] + rep["text_bytes"] == len(got)


def write_synth(lib, path, n, aligner):
    if aligner:
        names, lens, _ = grch38_no_alt()
        cfg = host.synth_config(n, read_len=150, genome=lens, file_style=ffi.SYNTH_FILE_REALISTIC,
                                seq_model=ffi.SYNTH_SEQ_FROM_REFERENCE, lib=lib)
        arr = (C.c_char_p * len(names))(*[x.encode() for x in names])
        rc = lib.ngsq_synth_write_bam_named(C.byref(cfg), arr, path.encode(), n, 1, 0)
    else:
        rc = lib.ngsq_synth_write_bam(C.byref(host.synth_config(n)), path.encode(), n, 1, 0)
    assert rc == 0, lib.ngsq_bam_last_error()


@pytest.mark.parametrize("aligner,n,batch", [(False, 200_000, 997), (True, 200_000, 640)])
def test_synthetic_files_over_hundreds_of_batches(gpu_lib, tmp_path, aligner, n, batch):
    path = str(tmp_path / "s.bam")
    write_synth(gpu_lib, path, n, aligner)
    got, rep = convert(gpu_lib, path, str(tmp_path / "s.sam"), batch_records=batch)
    assert rep["records"] == n
    assert rep["batches"] >= n // batch
    assert_same(got, sm.expected_sam(path))


def test_adversarial_aux(gpu_lib, tmp_path):
    """Tag data that reads as record heads (B:C arrays and Z strings of fake records), next to random records of every shape."""
    rng = np.random.default_rng(21)
    hb = random_batch(rng, 6000, LENS, max_len=200)
    aux = [bamio.adversarial_aux(rng, len(NAMES)) if rng.random() < 0.5 else bamio.aligner_aux(rng, int(hb.cols["l_seq"][i]))
           for i in range(hb.n)]
    names = [bamio.aligner_name(rng) for _ in range(hb.n)]
    path = str(tmp_path / "a.bam")
    bamio.write_bam(path, hb, NAMES, LENS, block_payload=7000, with_index=False, names=names, aux=aux)
    got, _ = convert(gpu_lib, path, str(tmp_path / "a.sam"), batch_records=333)
    assert_same(got, sm.expected_sam(path))


def test_long_reads_and_long_cigars(gpu_lib, tmp_path):
    """100 kb reads (with and without qualities), a 70 000-operation CIGAR (its CG tag is not written), a B array of
    thousands of integers."""
    rng = np.random.default_rng(22)
    recs = []
    for k in range(12):
        L = 100_000 + k
        seq = "".join(rng.choice(list("ACGTN"), L))
        recs.append(dict(flag=0, mapq=60, ref_id=0, pos=1000 * k, mate_ref_id=0, tlen=0, cigar=f"{L}M", seq=seq,
                         qual=None if k % 3 == 0 else rng.integers(0, 94, L).tolist()))
    ops = [(int(rng.integers(1, 30)) << 4) | int(rng.choice([0, 1, 2, 7, 8])) for _ in range(70_000)]
    q_len = sum(o >> 4 for o in ops if (o & 15) in (0, 1, 7, 8))
    recs.append(dict(flag=0, mapq=30, ref_id=1, pos=50, mate_ref_id=-1, tlen=0, cigar=ops, seq="A" * q_len, qual=[30] * q_len))
    recs.append(dict(flag=4, mapq=0, ref_id=-1, pos=-1, mate_ref_id=-1, tlen=0, cigar="*", seq="", qual=None))
    hb = batch_from_records(recs)
    aux = [b""] * hb.n
    aux[3] = bamio.aux_array(b"XB", b"i", rng.integers(-2 ** 31, 2 ** 31, 5000).astype("<i4").tobytes())
    aux[12] = bamio.aux_z(b"RG", b"g") + bamio.aux_array(b"XC", b"S", rng.integers(0, 65536, 3000).astype("<u2").tobytes())
    path = str(tmp_path / "l.bam")
    bamio.write_bam(path, hb, NAMES, LENS, with_index=False, aux=aux)
    got, rep = convert(gpu_lib, path, str(tmp_path / "l.sam"), batch_records=5)
    assert rep["records"] == hb.n
    want = sm.expected_sam(path)
    assert b"CG:B" not in want and b"\tXB:B:i," in want
    assert_same(got, want)


def test_float_tags_of_random_bit_patterns(gpu_lib, tmp_path):
    """B:f and f values: >= 10^5 random f32 bit patterns, NaNs, infinities, zeros, subnormals, FLT_MAX, ties."""
    rng = np.random.default_rng(23)
    special = np.array([0, 0x80000000, 1, 0x80000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000,
                        0x7FC00000, 0xFFC00001, 0x7F800001, 0x3F800000, 0x40600000, 0x3DCCCCCD, 0x60AD78EC, 0x4A000001], dtype=np.uint32)
    bits = np.concatenate([special, rng.integers(0, 2 ** 32, 120_000, dtype=np.uint64).astype(np.uint32)])
    n = 40
    hb = random_batch(rng, n, LENS, max_len=60, min_len=10, weird=False)
    per = len(bits) // n + 1
    aux = []
    for i in range(n):
        chunk = bits[i * per:(i + 1) * per]
        a = bamio.aux_array(b"ZF", b"f", chunk.astype("<u4").tobytes())
        if len(chunk):
            a += b"Xff" + struct.pack("<I", int(chunk[0]))
        aux.append(a)
    path = str(tmp_path / "f.bam")
    bamio.write_bam(path, hb, NAMES, LENS, with_index=False, aux=aux)
    got, _ = convert(gpu_lib, path, str(tmp_path / "f.sam"), batch_records=7)
    assert_same(got, sm.expected_sam(path))


def test_empty_file(gpu_lib, ngs, tmp_path):
    hb = random_batch(np.random.default_rng(24), 2, LENS)
    path = str(tmp_path / "e.bam")
    bamio.write_bam(path, hb.slice(0, 0), NAMES, LENS, with_index=False)
    got, rep = convert(gpu_lib, path, str(tmp_path / "e.sam"))
    assert rep["records"] == 0 and rep["batches"] == 0
    assert got == sm.expected_sam(path) and got.startswith(b"@HD\t")
    r = run(ngs, "convert", path, str(tmp_path / "e2.sam"))
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "e2.sam", "rb").read() == got


@pytest.fixture(scope="module")
def numbered_file(tmp_path_factory):
    rng = np.random.default_rng(25)
    hb = random_batch(rng, 5000, LENS, max_len=120)
    path = str(tmp_path_factory.mktemp("n") / "n.bam")
    bamio.write_bam(path, hb, NAMES, LENS, block_payload=9000, with_index=False,
                    aux=[bamio.aligner_aux(rng, int(hb.cols["l_seq"][i])) for i in range(hb.n)])
    return path, hb.n


@pytest.mark.parametrize("m", [1, 2, 999, 1000, 1001, 2000, 4999, 5000, 5001, 10 ** 9])
def test_max_records_inside_and_on_batch_boundaries(gpu_lib, tmp_path, numbered_file, m):
    path, n = numbered_file
    got, rep = convert(gpu_lib, path, str(tmp_path / "m.sam"), max_records=m, batch_records=1000)
    assert rep["records"] == min(m, n)
    assert_same(got, sm.expected_sam(path, min(m, n)))


def test_cli_equals_library_and_follows_the_counter(gpu_lib, ngs, tmp_path, numbered_file):
    path, n = numbered_file
    full, _ = convert(gpu_lib, path, str(tmp_path / "lib.sam"))
    out = str(tmp_path / "cli.sam")
    r = run(ngs, "convert", path, out)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == full
    for num in (0, 1, 37, n - 1, n, n + 5):
        open(out, "wb").write(b"stale text that the command truncates\n" * 1000)
        r = run(ngs, "-q", "convert", "-n", str(num), "-c", "best", "-r", "unused.fa", path, out)
        assert r.returncode == 0, r.stderr
        assert open(out, "rb").read() == sm.expected_sam(path, sm.records_written(n, num)), num


def test_processed_lines_once_per_million(gpu_lib, ngs, tmp_path):
    path = str(tmp_path / "p.bam")
    write_synth(gpu_lib, path, 2_100_000, False)
    out = str(tmp_path / "p.sam")
    os.symlink("/dev/null", out)      # (a gigabyte of text nobody reads)
    r = run(ngs, "convert", path, out)
    assert r.returncode == 0, r.stderr
    assert r.stderr.count("  [*] Processed ") == 2
    assert "  [*] Processed 1,000,000 records." in r.stderr and "  [*] Processed 2,000,000 records." in r.stderr
    r = run(ngs, "convert", "-n", "1500000", path, out)
    assert r.returncode == 0 and r.stderr.count("  [*] Processed ") == 1


def plant(rng, kind):
    """(record dict overrides, aux bytes) of one record without SAM text, and the error code the model gives it."""
    if kind == "tag_type":
        return {}, b"NMC\x01XXq\x01\x02\x03", sm.E_TAG_TYPE
    if kind == "z_nul":
        return {}, b"NMC\x01XZZno terminator", sm.E_STR_NUL
    if kind == "h_nul":
        return {}, b"XHH0AFF", sm.E_STR_NUL
    if kind == "b_sub":
        return {}, b"XBBq" + struct.pack("<I", 1) + b"\0", sm.E_B_SUB
    if kind == "b_count":
        return {}, b"XBBi" + struct.pack("<I", 1000) + b"\0" * 16, sm.E_OVERRUN
    if kind == "qual":
        return {"qual": [30, 40, 94, 20]}, b"", sm.E_QUAL
    if kind == "cigar_op":
        return {"cigar": [(2 << 4) | 0, (2 << 4) | 9]}, b"", sm.E_CIGAR_OP
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["tag_type", "z_nul", "h_nul", "b_sub", "b_count", "qual", "cigar_op"])
def test_each_error_class_exits_1_with_its_message(gpu_lib, ngs, tmp_path, kind):
    rng = np.random.default_rng(26)
    good = dict(flag=0, mapq=60, ref_id=0, mate_ref_id=0, tlen=0, cigar="4M", seq="ACGT", qual=[30, 31, 32, 33])
    recs = [dict(good, pos=10 * i) for i in range(3000)]
    bad_at = 1234
    over, bad_aux, code = plant(rng, kind)
    recs[bad_at] = dict(recs[bad_at], **over)
    hb = batch_from_records(recs)
    aux = [bamio.aux_z(b"RG", b"g1")] * hb.n
    aux[bad_at] = bad_aux
    path = str(tmp_path / "bad.bam")
    bamio.write_bam(path, hb, NAMES, LENS, with_index=False, aux=aux)
    with pytest.raises(sm.SamError) as want:
        sm.expected_sam(path)
    assert (want.value.index, want.value.code) == (bad_at, code)
    with pytest.raises(host.NgsqError) as e:
        host.bam_to_sam(path, str(tmp_path / "bad.sam"), lib=gpu_lib, batch_records=500)
    assert want.value.message in str(e.value)
    r = run(ngs, "convert", path, str(tmp_path / "bad2.sam"))
    assert r.returncode == 1
    assert r.stderr.strip().endswith("Error: " + want.value.message), r.stderr[-600:]
    # the records in front of the bad one are fine: -n stops before it
    got, _ = convert(gpu_lib, path, str(tmp_path / "ok.sam"), max_records=bad_at)
    assert got == sm.expected_sam(path, bad_at)


def test_hand_file_through_the_cli(gpu_lib, ngs, tmp_path):
    src = str(tmp_path / "h.bam")
    shutil.copy(os.path.join(GOLDEN, "hand_spec.bam"), src)     # (no .bai beside it: IndexCheck::None)
    out = str(tmp_path / "h.sam")
    r = run(ngs, "convert", src, out)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == open(os.path.join(GOLDEN, "hand_spec.sam"), "rb").read()
