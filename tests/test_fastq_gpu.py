"""`ngs fastq` on the GPU (include/ngsq_fastq.h): every output the device writes equals the test-side model
(tests/fastq_model.py) byte for byte -- on the hand-assembled files, on reads whose lengths sit on the edges of a wave's turn
(a lane takes two bases: 128 a turn) and of the nibble shift of a reversed odd read, on 100 kb reads, over batches of 1 to
20 000 records and ingest chunks that cut records, on files that give an output nothing, with the error of a score above 93,
through both compressors, through the command line, around `ngs generate` and `ngs convert`, and on a slice of the randomised
sweep of tools/fuzz_fastq.py."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from ngs_amd import build, ffi, host
from tests import bamio
from tests import fastq_model as fm
from tests import generate_model as gm
from tests.util import batch_from_records, random_batch
from tools.fuzz_fastq import EOF, FLAG_CYCLE, LENS, NAMES, check, convert, fastq_sweep, model, read_batch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = [dict(), dict(two_files=True), dict(two_files=True, other=True)]


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def run(ngs, *args):
    return subprocess.run([ngs, *args], capture_output=True, text=True, timeout=300)


# ---- 1. hand files ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hand_spec.bam", "hand_longcigar.bam"])
def test_hand_files(gpu_lib, tmp_path, name):
    path = os.path.join(GOLDEN, name)
    for mode in MODES:
        got, rep = check(gpu_lib, path, str(tmp_path), **mode)
        assert rep["records_scanned"] == rep["excluded"] + rep["no_sequence"] + rep["reads_one"] + rep["reads_two"] + rep["reads_other"]
    assert check(gpu_lib, path, str(tmp_path), exclude_flags=0)[1]["excluded"] == 0


# ---- 2. lane and nibble edges -----------------------------------------------------------------------------------------------
EDGE_LENGTHS = [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1025]
EDGE_NAMES = [0, 1, 63, 64, 65, 254]


@pytest.fixture(scope="module")
def edge_file(tmp_path_factory):
    """Every length forward and reversed, each with QUAL present, missing and all 93; names and flags cycling."""
    rng = np.random.default_rng(31)
    l_seq, flags, kinds, names = [], [], [], []
    for L in EDGE_LENGTHS:
        for rev in (0, 0x10):
            for kind in (0, 1, 2):
                k = len(l_seq)
                l_seq.append(L)
                flags.append(FLAG_CYCLE[(k // 6 + k) % len(FLAG_CYCLE)] | rev)      # (every class once per length, on another strand and QUAL each time)
                kinds.append(kind)
                names.append(bytes(rng.integers(33, 127, EDGE_NAMES[(k // 2) % len(EDGE_NAMES)]).astype(np.uint8)))
    path = str(tmp_path_factory.mktemp("edge") / "edge.bam")
    bamio.write_bam(path, read_batch(rng, l_seq, flags, kinds), NAMES, LENS, with_index=False, names=names, sort_order="unsorted")
    return path


@pytest.mark.parametrize("suffix", [False, True])
@pytest.mark.parametrize("mode", range(3))
def test_lane_and_nibble_edges(gpu_lib, tmp_path, edge_file, mode, suffix):
    n = len(EDGE_LENGTHS) * 6
    got, rep = check(gpu_lib, edge_file, str(tmp_path), name_suffix=suffix, **MODES[mode])
    assert rep["records_scanned"] == n and rep["excluded"] == n // 3 and rep["no_sequence"] == 0
    assert rep["dropped_other"] == (n // 3 if mode == 1 else 0)
    # with the secondary and supplementary records too: every combination of length, strand and QUAL is written
    got, rep = check(gpu_lib, edge_file, str(tmp_path), name_suffix=suffix, exclude_flags=0, batch_records=5, **MODES[mode])
    assert rep["excluded"] == 0 and sum(x.count(b"\n") for x in got) == 4 * (n - rep["dropped_other"])


# ---- 3. long reads ----------------------------------------------------------------------------------------------------------
def test_long_reads(gpu_lib, tmp_path):
    """Twelve reads of 100 000 + k bases, as tests/test_convert_gpu.write_long_reads makes them, half of them reversed."""
    rng = np.random.default_rng(22)
    recs = []
    for k in range(12):
        L = 100_000 + k
        recs.append(dict(flag=(0x10 if k % 2 else 0) | (0x40, 0x80, 0)[k % 3], mapq=60, ref_id=0, pos=1000 * k, mate_ref_id=0, tlen=0, cigar=f"{L}M",
                         seq="".join(rng.choice(list("ACGTN"), L)), qual=None if k % 4 == 0 else rng.integers(0, 94, L).tolist()))
    path = str(tmp_path / "l.bam")
    bamio.write_bam(path, batch_from_records(recs), NAMES, LENS, with_index=False)
    for kw in (dict(batch_records=5), dict(two_files=True, other=True, name_suffix=True)):
        got, rep = check(gpu_lib, path, str(tmp_path), **kw)
        assert sum(rep["text_bytes"]) == sum(2 * (100_000 + k) + 6 + len(b"r%d" % k) for k in range(12)) + (2 * 8 if kw.get("name_suffix") else 0)


# ---- 4. batch edges ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_file(tmp_path_factory):
    d = tmp_path_factory.mktemp("rnd")
    rng = np.random.default_rng(32)
    hb = random_batch(rng, 20_000, LENS, max_len=160)
    hb.cols["flag"] = (hb.cols["flag"] & ~np.uint16(0x900) | np.where(rng.random(hb.n) < 0.1, 0x100, 0).astype(np.uint16)).astype(np.uint16)
    names = [bamio.aligner_name(rng) for _ in range(hb.n)]
    paths = [str(d / "r.bam"), str(d / "r7000.bam")]
    bamio.write_bam(paths[0], hb, NAMES, LENS, with_index=False, names=names)
    bamio.write_bam(paths[1], hb, NAMES, LENS, with_index=False, names=names, block_payload=7000)
    return paths, model(paths[0], two_files=True, other=True)


@pytest.mark.parametrize("batch", [1, 7, 64, 997, 0])
def test_batch_edges(gpu_lib, tmp_path, random_file, batch):
    """The same three outputs whatever the batch: each equals the model's, so all five are identical."""
    (path, _), want = random_file
    got, rep = convert(gpu_lib, path, str(tmp_path), two_files=True, other=True, batch_records=batch)
    assert got == list(want[:3])
    assert rep["records_scanned"] == 20_000 and all(rep[k] == v for k, v in want[3].items())
    assert rep["batches"] >= (-(-20_000 // batch) if batch else 1)       # (the batches were really that small)


def test_ingest_chunks_that_cut_records(gpu_lib, tmp_path, random_file):
    (_, path), want = random_file
    for batch in (997, 0):
        got, rep = convert(gpu_lib, path, str(tmp_path), two_files=True, other=True, batch_records=batch)
        assert got == list(want[:3]) and all(rep[k] == v for k, v in want[3].items())


# ---- 5. degenerate files ----------------------------------------------------------------------------------------------------
def test_degenerate_files(gpu_lib, tmp_path):
    rng = np.random.default_rng(33)
    hb = read_batch(rng, [50] * 40, [0x41] * 40, [0] * 40)
    empty, ones, none_kept = str(tmp_path / "e.bam"), str(tmp_path / "1.bam"), str(tmp_path / "x.bam")
    bamio.write_bam(empty, hb.slice(0, 0), NAMES, LENS, with_index=False)
    bamio.write_bam(ones, hb, NAMES, LENS, with_index=False)
    hb.cols["flag"][:] = 0x141
    bamio.write_bam(none_kept, hb, NAMES, LENS, with_index=False)
    for mask in (0, 7):
        got, rep = check(gpu_lib, empty, str(tmp_path), two_files=True, other=True, bgzf_mask=mask)      # no records at all
        assert rep["records_scanned"] == 0 and rep["batches"] == 0 and got == [b"", b"", b""]
        got, rep = check(gpu_lib, ones, str(tmp_path), two_files=True, other=True, bgzf_mask=mask)       # only read ones
        assert rep["reads_one"] == 40 and len(got[0]) and got[1:] == [b"", b""]
        got, rep = check(gpu_lib, none_kept, str(tmp_path), two_files=True, bgzf_mask=mask & 3)          # every record excluded
        assert rep["excluded"] == 40 and got == [b"", b"", b""]
    raw, rep = convert(gpu_lib, ones, str(tmp_path), two_files=True, bgzf_mask=2)
    assert raw[1] == EOF and rep["compressed_bytes"] == [0, 28, 0] and rep["blocks"] == 0                 # the EOF block alone
    for m in (1, 39, 40, 41):                                                                          # -n of 1 and the count +- 1
        got, rep = check(gpu_lib, ones, str(tmp_path), max_records=m)
        assert rep["records_scanned"] == min(m, 40) == rep["reads_one"]


def test_num_records_on_the_command_line(gpu_lib, ngs, tmp_path):
    """-n 0 examines nothing: empty files, one empty gzip member from the host, the EOF block alone from the device."""
    rng = np.random.default_rng(34)
    path = str(tmp_path / "n.bam")
    bamio.write_bam(path, read_batch(rng, [30] * 10, [0x41, 0x81] * 5, [0] * 10), NAMES, LENS, with_index=False)
    one, two, gz = str(tmp_path / "a.fastq"), str(tmp_path / "b.fq"), str(tmp_path / "c.fastq.gz")
    for num, kept in ((0, 0), (1, 1), (9, 9), (10, 10), (11, 10)):
        r = run(ngs, "-q", "fastq", "-n", str(num), path, one, two)
        assert r.returncode == 0, r.stderr
        w = model(path, two_files=True, max_records=num) if num else (b"", b"")
        assert (open(one, "rb").read(), open(two, "rb").read()) == (w[0], w[1]), num
    for where in ("host", "device"):
        r = run(ngs, "-q", "fastq", "-n", "0", "--gzip", where, path, gz)
        assert r.returncode == 0, r.stderr
        raw = open(gz, "rb").read()
        assert gzip.decompress(raw) == b"" and (raw == EOF if where == "device" else len(raw) > 0)


# ---- 6. the error -----------------------------------------------------------------------------------------------------------
def test_score_above_93(gpu_lib, tmp_path):
    rng = np.random.default_rng(35)
    hb = read_batch(rng, rng.integers(20, 120, 6000), [0x41, 0x91] * 3000, [0] * 6000)
    q, off = hb.cols["qual"], hb.cols["qual_off"]
    q[int(off[4321]) + 7] = 94
    q[int(off[5000]) + 1] = 200
    path = str(tmp_path / "bad.bam")
    bamio.write_bam(path, hb, NAMES, LENS, with_index=False)
    assert model(path) == fm.error_message(4321)
    for kw in (dict(), dict(batch_records=1000), dict(two_files=True, batch_records=4322), dict(batch_records=6000, bgzf_mask=1)):
        with pytest.raises(host.NgsqError) as e:
            convert(gpu_lib, path, str(tmp_path), **kw)
        assert e.value.code == ffi.ERR_INVALID_ARGUMENT and e.value.message == "writing FASTQ record: record 4321: quality score above 93"
    check(gpu_lib, path, str(tmp_path), max_records=4321)                  # the records in front of it are fine
    # the same bytes in records excluded by flag: no error
    hb.cols["flag"][4321] |= 0x100
    hb.cols["flag"][5000] |= 0x800
    bamio.write_bam(path, hb, NAMES, LENS, with_index=False)
    _, rep = check(gpu_lib, path, str(tmp_path), two_files=True)
    assert rep["excluded"] == 2
    with pytest.raises(host.NgsqError) as e:
        convert(gpu_lib, path, str(tmp_path), exclude_flags=0x800)
    assert e.value.message == fm.error_message(4321)


def test_a_failed_write_ends_the_call_with_its_message(gpu_lib, tmp_path, edge_file):
    """/dev/full refuses every write: the message names the output."""
    import faulthandler
    faulthandler.dump_traceback_later(120, exit=True)
    try:
        for k, what in enumerate(("read one file", "read two file", "other reads file")):
            p = [str(tmp_path / f"w{j}.fastq") for j in range(3)]
            p[k] = "/dev/full"
            with pytest.raises(host.NgsqError) as e:
                host.bam_to_fastq(edge_file, p[0], p[1], p[2], exclude_flags=0, batch_records=20, lib=gpu_lib)
            assert e.value.message == f"could not write record to {what}: No space left on device (os error 28)"
    finally:
        faulthandler.cancel_dump_traceback_later()


def test_bad_arguments_are_refused_before_anything_is_written(gpu_lib, tmp_path, edge_file):
    p = [str(tmp_path / f"a{j}.fastq") for j in range(3)]
    for kw, args in ((dict(exclude_flags=65536), p[:1]), (dict(require_flags=1 << 20), p[:1]), (dict(default_quality=94), p[:1]), (dict(bgzf_mask=2), p[:1]),
                     (dict(bgzf_mask=4), p[:2]), (dict(bgzf_mask=8), p), (dict(name_suffix=2), p[:1]), (dict(), [p[0], None, p[2]])):
        with pytest.raises(host.NgsqError) as e:
            host.bam_to_fastq(edge_file, *args, lib=gpu_lib, **kw)
        assert e.value.code == ffi.ERR_INVALID_ARGUMENT, kw
        assert all(os.path.getsize(x) == 0 for x in p if os.path.exists(x))


# ---- 7. compressed outputs --------------------------------------------------------------------------------------------------
def test_compressed_outputs(gpu_lib, ngs, tmp_path, edge_file):
    got, rep = check(gpu_lib, edge_file, str(tmp_path), two_files=True, other=True, bgzf_mask=7, exclude_flags=0)     # (gunzips, looks for the EOF block)
    assert rep["blocks"] >= 3 and all(c > 28 for c in rep["compressed_bytes"])
    high, rep_high = check(gpu_lib, edge_file, str(tmp_path), two_files=True, other=True, bgzf_mask=5, exclude_flags=0, effort="high")
    assert high == got and rep_high["compressed_bytes"][1] == 0
    # the command line: plain output is the library's, byte for byte; --gzip host and --gzip device gunzip to the same bytes
    p = [str(tmp_path / x) for x in ("c1.fastq", "c2.fq", "c3.fastq")]
    r = run(ngs, "fastq", "--exclude-flags", "0", edge_file, p[0], p[1], "--other", p[2])
    assert r.returncode == 0, r.stderr
    assert [open(x, "rb").read() for x in p] == got
    for where in ("host", "device"):
        z = [str(tmp_path / x) for x in (f"{where}1.fastq.gz", f"{where}2.fq.gz", f"{where}3.fastq")]
        r = run(ngs, "-v", "fastq", "--gzip", where, "--exclude-flags", "0", edge_file, z[0], z[1], "--other", z[2], "-t", "4")
        assert r.returncode == 0, r.stderr
        assert "[ngs] fastq: " in r.stderr
        raw = [open(x, "rb").read() for x in z]
        assert [gzip.decompress(raw[0]), gzip.decompress(raw[1]), raw[2]] == got
        assert (raw[0].endswith(EOF) and raw[1].endswith(EOF)) == (where == "device")


def test_command_line_messages(gpu_lib, ngs, tmp_path, edge_file):
    """At the default level: a line when the two files differ in number, a line when others were dropped."""
    a, b = str(tmp_path / "m1.fastq"), str(tmp_path / "m2.fastq")
    r = run(ngs, "fastq", edge_file, a, b, "--require-flags", "64")
    assert r.returncode == 0 and "do not pair line by line" in r.stderr and "were dropped" in r.stderr      # (0xC1 is an other that has 0x40)
    r = run(ngs, "fastq", edge_file, a, b, "--exclude-flags", "16", "--other", str(tmp_path / "m3.fastq"))
    c = model(edge_file, two_files=True, other=True, exclude_flags=16)[3]
    assert r.returncode == 0 and ("do not pair" in r.stderr) == (c["reads_one"] != c["reads_two"]) and "were dropped" not in r.stderr, r.stderr
    r = run(ngs, "-q", "fastq", edge_file, a, b)
    assert r.returncode == 0 and r.stderr == ""


# ---- 8. round trip with the project's own tools ------------------------------------------------------------------------------
def test_round_trip_through_generate_and_convert(gpu_lib, ngs, tmp_path):
    rng = np.random.default_rng(36)
    fa = str(tmp_path / "ref.fasta")
    open(fa, "wb").write(gm.fasta_text([(b"a", gm.random_letters(rng, 60_000)), (b"b", gm.random_letters(rng, 30_000))], 80))
    g1, g2 = str(tmp_path / "g_1.fastq"), str(tmp_path / "g_2.fastq")
    host.generate([(fa, 100, 300.0, 30.0, 101, 1)], g1, g2, 7, 3000, lib=gpu_lib)
    one, two = open(g1, "rb").read(), open(g2, "rb").read()
    r1, r2 = gm.parse_fastq(one), gm.parse_fastq(two)
    assert len(r1) == len(r2) == 3000
    comp = bytes.maketrans(b"ACGTN", b"TGCAN")
    for variant in ("forward", "every other pair reversed"):
        lines = [b"@HD\tVN:1.6\tSO:unsorted\n"]
        for k, (a, b) in enumerate(zip(r1, r2)):
            for flag, (name, seq, qual) in ((77, a), (141, b)):
                if variant != "forward" and k % 2:
                    flag, seq, qual = flag | 16, seq.translate(comp)[::-1], qual[::-1]
                lines.append(b"\t".join([name, b"%d" % flag, b"*", b"0", b"0", b"*", b"*", b"0", b"0", seq, qual]) + b"\n")
        sam, bam = str(tmp_path / "u.sam"), str(tmp_path / "u.bam")
        open(sam, "wb").write(b"".join(lines))
        assert host.sam_to_bam(sam, bam, lib=gpu_lib)["records"] == 6000
        o1, o2 = str(tmp_path / "back_1.fastq"), str(tmp_path / "back_2.fastq")
        r = run(ngs, "fastq", bam, o1, o2)
        assert r.returncode == 0, r.stderr
        assert "do not pair" not in r.stderr and "dropped" not in r.stderr
        assert open(o1, "rb").read() == one and open(o2, "rb").read() == two, variant
        # one file: the pairs interleaved
        got, _ = convert(gpu_lib, bam, str(tmp_path))
        assert gm.parse_fastq(got[0]) == [x for pair in zip(r1, r2) for x in pair]


# ---- 9. a slice of the randomised sweep ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 8, 16, 24])
def test_fuzz_slice(gpu_lib, base):
    fastq_sweep(gpu_lib, 8, base, verbose=False)
