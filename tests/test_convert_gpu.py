"""`ngs convert <BAM> <SAM>` on the GPU: the text the device formats equals the test-side model
(tests/sam_model.py) byte for byte -- on the hand-assembled files, synthetic files over hundreds of batches, adversarial tag
data, 100 kb reads, 70 000-operation CIGARs, float arrays of random bit patterns, an empty file and every `-n` case -- the
command line writes what the library writes, and every kind of record without SAM text ends the run with its message.
The edges of the kernel's own steps: CIGARs, strings and arrays of 63 / 64 / 65 ... 193 items (a wave takes 64 at a time), the
extremes of every fixed field, two defects in one record, batch or file, more float records than one turn of the float
kernels, and files of several ingest chunks (the record a chunk's end cuts is read from the carried bytes)."""
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
from tests.util import batch_from_records, plant, random_batch

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


def write_adversarial(path):
    rng = np.random.default_rng(21)
    hb = random_batch(rng, 6000, LENS, max_len=200)
    aux = [bamio.adversarial_aux(rng, len(NAMES)) if rng.random() < 0.5 else bamio.aligner_aux(rng, int(hb.cols["l_seq"][i]))
           for i in range(hb.n)]
    names = [bamio.aligner_name(rng) for _ in range(hb.n)]
    bamio.write_bam(path, hb, NAMES, LENS, block_payload=7000, with_index=False, names=names, aux=aux)
    return path


def test_adversarial_aux(gpu_lib, tmp_path):
    """Tag data that reads as record heads (B:C arrays and Z strings of fake records), next to random records of every shape."""
    path = write_adversarial(str(tmp_path / "a.bam"))
    got, _ = convert(gpu_lib, path, str(tmp_path / "a.sam"), batch_records=333)
    assert_same(got, sm.expected_sam(path))


def write_long_reads(path):
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
    bamio.write_bam(path, hb, NAMES, LENS, with_index=False, aux=aux)
    return hb.n


def test_long_reads_and_long_cigars(gpu_lib, tmp_path):
    """100 kb reads (with and without qualities), a 70 000-operation CIGAR (its CG tag is not written), a B array of
    thousands of integers."""
    path = str(tmp_path / "l.bam")
    n = write_long_reads(path)
    got, rep = convert(gpu_lib, path, str(tmp_path / "l.sam"), batch_records=5)
    assert rep["records"] == n
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


@pytest.mark.parametrize("kind", ["tag_type", "z_nul", "h_nul", "b_sub", "b_count", "qual", "cigar_op",
                                  "ref:id_n_refs", "ref:id_minus_2", "ref:mate_n_refs", "ref:mate_int_max"])
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


GOOD = dict(flag=0, mapq=60, ref_id=0, mate_ref_id=0, tlen=0, cigar="4M", seq="ACGT", qual=[30, 31, 32, 33])
FLOAT_TAG = b"Xff" + struct.pack("<f", 0.1) + bamio.aux_array(b"ZF", b"f", struct.pack("<3f", 1.5, -2.25, 1e-7))
TWO_ERRORS = {
    # name: {record index: (plant kind or (record overrides, aux))}, with batches of 500 records (four records share a block)
    "ref_and_cigar_op_in_one_record": {1234: ({"ref_id": 3, "cigar": [(2 << 4) | 0, (2 << 4) | 9]}, b"")},
    "qual_and_tag_type_in_one_record": {1234: ({"qual": [30, 40, 94, 20]}, b"NMC\x01XXq\x01")},
    "str_nul_behind_b_sub_in_one_record": {1234: ({}, b"XBBq" + struct.pack("<I", 1) + b"\0XZZno terminator")},
    "two_waves_of_one_block": {1001: "b_count", 1002: "ref:id_n_refs"},
    "two_blocks_of_one_batch": {1003: "b_count", 1300: "ref:id_n_refs"},
    "last_and_first_of_two_batches": {1499: "z_nul", 1500: "cigar_op"},
    "two_batches": {1234: "b_count", 2234: "ref:mate_n_refs"},
    "bad_tag_behind_a_float_tag": {1234: ({}, FLOAT_TAG + b"XXq\x01")},
    "float_record_in_front_of_a_plain_bad_one": {1233: ({}, FLOAT_TAG + b"XZZno terminator"), 1234: "qual"},
    "plain_record_in_front_of_a_float_bad_one": {1233: "cigar_op", 1234: ({"ref_id": -2}, FLOAT_TAG)},
}


@pytest.mark.parametrize("case", sorted(TWO_ERRORS))
def test_of_two_errors_the_first_record_s_smallest_code_is_reported(gpu_lib, tmp_path, case):
    """The smaller code of a record with two defects; the smaller index of two bad records, whichever wave, block, batch or
    pass (the plain one or the float records' second one) meets them, and whatever their codes."""
    rng = np.random.default_rng(27)
    recs = [dict(GOOD, pos=10 * i) for i in range(3000)]
    aux = [bamio.aux_z(b"RG", b"g1")] * len(recs)
    for at, what in TWO_ERRORS[case].items():
        over, bad_aux = plant(rng, what)[:2] if isinstance(what, str) else what
        recs[at] = dict(recs[at], **over)
        aux[at] = bad_aux
    path = str(tmp_path / "bad.bam")
    bamio.write_bam(path, batch_from_records(recs), NAMES, LENS, with_index=False, aux=aux)
    with pytest.raises(sm.SamError) as want:
        sm.expected_sam(path)
    first = min(TWO_ERRORS[case])
    assert want.value.index == first
    if case == "ref_and_cigar_op_in_one_record":
        assert want.value.code == sm.E_REF
    if case == "qual_and_tag_type_in_one_record":
        assert want.value.code == sm.E_QUAL
    with pytest.raises(host.NgsqError) as e:
        host.bam_to_sam(path, str(tmp_path / "bad.sam"), lib=gpu_lib, batch_records=500)
    assert want.value.message in str(e.value)
    got, _ = convert(gpu_lib, path, str(tmp_path / "ok.sam"), max_records=first, batch_records=500)
    assert got == sm.expected_sam(path, first)


LADDER = [0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193]      # items of a record's CIGAR, bases, string or array: a wave takes 64 at a time
LADDER_NAMES = ["x", "L" * 300, "chr3"]
INT_RANGE = {b"c": (-128, 127, "<i1"), b"C": (0, 255, "<u1"), b"s": (-32768, 32767, "<i2"), b"S": (0, 65535, "<u2"),
             b"i": (-2 ** 31, 2 ** 31 - 1, "<i4"), b"I": (0, 2 ** 32 - 1, "<u4")}
OP_LENGTHS = [1, 12, 123, 1234, 12345, 123456, 1234567, 12345678, 123456789, 2 ** 28 - 1, 9, 99999, 100000]   # 1-9 decimal digits


def ladder_cigar(K):
    """K operations: every second one consumes no bases and takes the long lengths (N D H P), the others 1-2 digit lengths
    of M I S = X; the bases they consume."""
    ops, l_seq = [], 0
    for j in range(K):
        if j % 2:
            ops.append((OP_LENGTHS[(j // 2) % len(OP_LENGTHS)] << 4) | (3, 2, 5, 6)[(j // 2) % 4])
        else:
            n = 1 + (7 * j) % 23
            ops.append((n << 4) | (0, 1, 4, 7, 8)[(j // 2) % 5])
            l_seq += n
    return ops, l_seq


@pytest.fixture(scope="module")
def ladder_file(tmp_path_factory):
    """One record per K of LADDER and kind of item, each with a tag behind the item that moves if the cursor is wrong; read
    names of 1 to 254 bytes; @SQ names of 1 and 300 characters; every integer type's extremes, scalar and in arrays."""
    rng = np.random.default_rng(28)
    recs, aux, names = [], [], []
    tail = bamio.aux_int(b"ZZ", 7)

    def add(tag_bytes=b"", name=None, **over):
        recs.append(dict(GOOD, pos=len(recs), ref_id=len(recs) % 3, mate_ref_id=(len(recs) // 3) % 3, **over))
        aux.append(tag_bytes)
        names.append(name if name is not None else b"q%d" % len(names))

    for K in LADDER:
        ops, l_seq = ladder_cigar(K)
        seq = "".join(rng.choice(list("ACGTN"), l_seq)) if l_seq else "ACGT"
        add(tail, cigar=ops, seq=seq, qual=rng.integers(0, 94, len(seq)).tolist())
        bases = "".join(rng.choice(list("ACGTNRY="), K))
        add(tail, cigar=f"{K}M" if K else "*", seq=bases, qual=rng.integers(0, 94, K).tolist())
        add(tail, cigar=f"{K}M" if K else "*", seq=bases, qual=None)
        add(bamio.aux_z(b"XZ", bytes(rng.integers(1, 256, K, dtype=np.uint8).tolist())) + tail)
        add(b"XHH" + bytes(rng.choice(list(b"0123456789ABCDEF"), K).tolist()) + b"\0" + tail)
        for sub, (lo, hi, dt) in INT_RANGE.items():
            v = rng.integers(lo, hi + 1, K, dtype=np.int64)
            v[:1], v[-1:] = lo, hi                           # (K == 1: the maximum; the minimum is in every longer array)
            if K > 2:
                v[K // 2] = lo if K % 2 else hi              # an extreme in the middle, one in the last lane of a full step
                v[min(K - 1, 63)] = lo
            add(bamio.aux_array(b"XB", sub, v.astype(dt).tobytes()) + tail)
        bits = rng.integers(0, 2 ** 32, K, dtype=np.uint64).astype("<u4")
        bits[:3] = np.array([0x7F7FFFFF, 0x80000001, 0xFF800000], dtype="<u4")[:K]
        add(bamio.aux_array(b"XB", b"f", bits.tobytes()) + tail)
    for lo_hi in (0, 1):                                       # the scalars' extremes
        add(b"".join(b"X" + sub + sub + np.array([rg[lo_hi]]).astype(rg[2]).tobytes() for sub, rg in INT_RANGE.items()) + tail)
    for n in (1, 63, 64, 65, 254):
        add(tail, name=bytes(rng.choice(list(b"abcXYZ019:/_"), n).tolist()))
    path = str(tmp_path_factory.mktemp("ladder") / "ladder.bam")
    bamio.write_bam(path, batch_from_records(recs), LADDER_NAMES, LENS, block_payload=5000, with_index=False, names=names, aux=aux)
    want = sm.expected_sam(path)
    # the model's text holds what the ladder is for
    assert b"268435455D" in want and b"123456789N" in want and b"XB:B:I,0," in want and b",4294967295\tZZ:i:7" in want and b"XB:B:i,-2147483648" in want
    assert b"Xc:i:-128\tXC:i:0\tXs:i:-32768\tXS:i:0\tXi:i:-2147483648\tXI:i:0\t" in want
    assert b"Xc:i:127\tXC:i:255\tXs:i:32767\tXS:i:65535\tXi:i:2147483647\tXI:i:4294967295\t" in want
    assert b"\t" + b"L" * 300 + b"\t" in want and sm.count_records(path) == len(recs)
    return path, want, len(recs)


@pytest.mark.parametrize("batch", [1, 3, 4, 5, 0])
def test_lane_ladder(gpu_lib, tmp_path, ladder_file, batch):
    path, want, n = ladder_file
    got, rep = convert(gpu_lib, path, str(tmp_path / "k.sam"), batch_records=batch)
    assert rep["records"] == n
    assert_same(got, want)
    assert got == want


def test_fixed_field_extremes(gpu_lib, tmp_path):
    """POS and PNEXT of -1, 0 and 2^31 - 1 (2147483648 in the text), TLEN at both ends of its type, FLAG 65535, MAPQ 255, and
    every RNEXT case."""
    edge = [-1, 0, 2 ** 31 - 1]
    recs, mate_pos = [], []
    for pos in edge:
        for npos in edge:
            for tlen in (-2 ** 31, 2 ** 31 - 1):
                recs.append(dict(GOOD, pos=pos, tlen=tlen, flag=65535, mapq=255))
                mate_pos.append(npos)
    for ref, mate in ((0, 0), (2, 2), (0, 1), (1, 0), (-1, -1), (-1, 1), (2, -1), (0, -1)):      # = = name name * name * *
        recs.append(dict(GOOD, pos=5, ref_id=ref, mate_ref_id=mate, flag=0, mapq=0))
        mate_pos.append(7)
    path = str(tmp_path / "x.bam")
    bamio.write_bam(path, batch_from_records(recs), NAMES, LENS, with_index=False, mate_pos=mate_pos)
    want = sm.expected_sam(path)
    assert b"\t65535\tchr1\t2147483648\t255\t4M\t=\t2147483648\t-2147483648\t" in want
    assert b"\t65535\tchr1\t0\t255\t4M\t=\t0\t2147483647\t" in want
    assert [l.split(b"\t")[6] for l in want.split(b"\n")[-9:-1]] == [b"=", b"=", b"chr2", b"chr1", b"*", b"chr2", b"*", b"*"]
    for batch in (0, 1):
        got, rep = convert(gpu_lib, path, str(tmp_path / "x.sam"), batch_records=batch)
        assert rep["records"] == len(recs)
        assert_same(got, want)
        assert got == want


@pytest.fixture(scope="module")
def many_floats_file(tmp_path_factory):
    """9 000 short records, every second one with an `f` tag and a B:f array of three."""
    rng = np.random.default_rng(29)
    hb = random_batch(rng, 9000, LENS, max_len=40, min_len=10, weird=False)
    bits = rng.integers(0, 2 ** 32, (9000, 4), dtype=np.uint64).astype("<u4")
    aux = [b"Xff" + bits[i, :1].tobytes() + bamio.aux_array(b"ZF", b"f", bits[i, 1:].tobytes()) if i % 2 else bamio.aux_int(b"NM", i)
           for i in range(hb.n)]
    path = str(tmp_path_factory.mktemp("floats") / "f.bam")
    bamio.write_bam(path, hb, NAMES, LENS, with_index=False, aux=aux)
    return path, sm.expected_sam(path)


@pytest.mark.parametrize("batch", [0, 4097])
def test_more_float_records_than_one_turn_of_the_float_kernels(gpu_lib, tmp_path, many_floats_file, batch):
    """4 500 marked records in one batch (the float kernels' grid holds 4 096 waves: a second turn of their loop), and two
    batches cut at 4 097, whose lists of marked records follow each other on the stream."""
    path, want = many_floats_file
    got, rep = convert(gpu_lib, path, str(tmp_path / "f.sam"), batch_records=batch)
    assert rep["records"] == 9000 and rep["batches"] == (1 if batch == 0 else 3)
    assert_same(got, want)
    assert got == want


@pytest.mark.parametrize("which", ["long_reads", "adversarial"])
def test_files_of_several_ingest_chunks(gpu_lib, tmp_path, monkeypatch, which):
    """1 MiB ingest buffers: a chunk is as many blocks as inflate to half the buffer (`out_limit` of reader_main,
    bam_device_reader.cpp), every chunk's end cuts a record (a 100 kb read; a record whose tag data reads as record heads),
    and the next batch reads it from the bytes carried in front of its chunk."""
    monkeypatch.setenv("NGSQ_INGEST_RAW_MB", "1")
    path = str(tmp_path / "c.bam")
    if which == "long_reads":
        write_long_reads(path)
    else:
        write_adversarial(path)
    want = sm.expected_sam(path)
    inflated = sum(b.isize for b in sm.bm.read_blocks(path)[0])
    got, rep = convert(gpu_lib, path, str(tmp_path / "c.sam"))
    assert inflated > 3 << 19 and rep["batches"] >= inflated // 2 ** 20 and rep["batches"] >= 2
    assert_same(got, want)
    assert got == want


def test_hand_file_through_the_cli(gpu_lib, ngs, tmp_path):
    src = str(tmp_path / "h.bam")
    shutil.copy(os.path.join(GOLDEN, "hand_spec.bam"), src)     # (no .bai beside it: IndexCheck::None)
    out = str(tmp_path / "h.sam")
    r = run(ngs, "convert", src, out)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == open(os.path.join(GOLDEN, "hand_spec.sam"), "rb").read()
