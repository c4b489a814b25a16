"""`ngs fastq --collate` on the GPU (include/ngsq_collate.h): every output the device writes and every count
equals the test-side model (tests/fastq_collate_model.py) -- on the hand-worked files in every mode, with 0 to 2 kept records,
around the 64 lanes of a wave, on reads whose lengths sit on the edges of the formatter's turn, with names of 0 and 254
bytes, with the name hash cut to one and three bits so that unlike names share a run, at the run limit and one beyond it, over
batches and ingest chunks that cut records, over pieces that cut pairs, at the budget and one byte short of it, with -n around a
pair's second record, with the error of a score above 93, with a write that fails, through both compressors, through the
command line, around `ngs generate` and `ngs convert`, and on a slice of the randomised sweep of tools/fuzz_fastq_collate.py."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from ngs_amd import build, ffi, host
from tests import bamio
from tests import fastq_model as fm
from tests import generate_model as gm
from tests.test_fastq_collate import T_ORDER, hand_names, hand_order
from tools.fuzz_fastq import EOF, LENS, NAMES, random_names, read_batch
from tools.fuzz_fastq_collate import check, collate_sweep, convert, model, paired_reads

pytestmark = pytest.mark.gpu

# (two_files, other, singletons): every combination of outputs
MODES = [dict(), dict(singletons=True), dict(two_files=True), dict(two_files=True, singletons=True), dict(two_files=True, other=True),
         dict(two_files=True, other=True, singletons=True)]
ALL = dict(two_files=True, other=True, singletons=True)


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def run(ngs, *args):
    return subprocess.run([ngs, *args], capture_output=True, text=True, timeout=300)


def write(path, rng, names, flags, l_seq, kinds=None, **kw):
    n = len(names)
    bamio.write_bam(str(path), read_batch(rng, l_seq, flags, [0] * n if kinds is None else kinds), NAMES, LENS, with_index=False, names=names,
                    sort_order="unsorted", **kw)
    return str(path)


# ---- 1. hand files ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("suffix", [False, True])
def test_hand_files(gpu_lib, tmp_path, suffix):
    order, (names, _) = hand_order(tmp_path / "o.bam"), hand_names(tmp_path / "n.bam")
    for mode in MODES:
        check(gpu_lib, order, str(tmp_path), name_suffix=suffix, **mode)
        _, rep = check(gpu_lib, names, str(tmp_path), name_suffix=suffix, **mode)
        assert (rep["pairs"], rep["singletons"], rep["ambiguous"], rep["name_collisions"]) == (2, 9, 3, 0)
    got, rep = check(gpu_lib, order, str(tmp_path), two_files=True, singletons=True)
    assert got == [T_ORDER[4] + T_ORDER[1], T_ORDER[0] + T_ORDER[3], b"", T_ORDER[2]]      # (the literal bytes of the CPU test)
    assert check(gpu_lib, names, str(tmp_path), exclude_flags=0, **ALL)[1]["pairs"] == 3


# ---- 2. 0, 1 and 2 kept records, and the lanes of a wave ----------------------------------------------------------------------
def test_few_kept_records(gpu_lib, tmp_path):
    rng = np.random.default_rng(41)
    empty = write(tmp_path / "e.bam", rng, [], [], [])
    for mask in (0, 15):
        got, rep = check(gpu_lib, empty, str(tmp_path), bgzf_mask=mask, **ALL)
        assert got == [b""] * 4 and rep["records_scanned"] == 0 and rep["resident_records"] == 0 and rep["pieces"] == 0
    none_kept = write(tmp_path / "x.bam", rng, [b"a", b"a"], [0x141, 0x981], [10, 10])
    assert check(gpu_lib, none_kept, str(tmp_path), **ALL)[1]["excluded"] == 2
    for flags, pairs in (([0x41], 0), ([0x01], 0), ([0x41, 0x81], 1), ([0x81, 0x41], 1), ([0x41, 0x41], 0), ([0x41, 0x01], 0), ([0x41, 0x181], 0)):
        path = write(tmp_path / "k.bam", rng, [b"a"] * len(flags), flags, [7] * len(flags))
        for mode in (MODES[1], MODES[5]):
            assert check(gpu_lib, path, str(tmp_path), **mode)[1]["pairs"] == pairs


@pytest.mark.parametrize("n", [63, 64, 65])
def test_records_around_a_wave(gpu_lib, tmp_path, n):
    """n records with names: mates next to each other, and mates n // 2 apart."""
    rng = np.random.default_rng(42)
    h = n // 2
    for names, flags in (([b"r%d" % (k // 2) for k in range(n)], [0x41, 0x81] * n),
                         ([b"r%d" % (k % h) if k < 2 * h else b"odd" for k in range(n)], [0x41] * h + [0x81] * n)):
        path = write(tmp_path / "w.bam", rng, names, flags[:n], rng.integers(1, 70, n))
        _, rep = check(gpu_lib, path, str(tmp_path), **ALL)
        assert rep["pairs"] == n // 2 and rep["singletons"] == n % 2
        check(gpu_lib, path, str(tmp_path), singletons=True, piece_records=64)


# ---- 3. read lengths and names ------------------------------------------------------------------------------------------------
def test_read_lengths_as_pairs(gpu_lib, tmp_path):
    """Pairs of reads of 1, 127, 128, 129 and 1025 bases, forward and reversed, QUAL present, missing and all 93."""
    rng = np.random.default_rng(43)
    names, flags, l_seq, kinds = [], [], [], []
    for L in (1, 127, 128, 129, 1025):
        for k, (f1, f2) in enumerate(((0x41, 0x81), (0x51, 0x81), (0x41, 0x91), (0x51, 0x91))):
            names += [b"L%d_%d" % (L, k)] * 2
            flags += [f1, f2]
            l_seq += [L, L]
            kinds += [k % 3, (k + 1) % 3]
    order = rng.permutation(len(names))
    path = write(tmp_path / "l.bam", rng, [names[k] for k in order], np.array(flags)[order], np.array(l_seq)[order], np.array(kinds)[order])
    for kw in (dict(two_files=True), dict(name_suffix=True), dict(two_files=True, piece_records=3, default_quality=40)):
        _, rep = check(gpu_lib, path, str(tmp_path), **kw)
        assert rep["pairs"] == 20 and rep["singletons"] == 0


def test_names_of_0_and_254_bytes(gpu_lib, tmp_path):
    rng = np.random.default_rng(44)
    long_a = bytes(rng.integers(48, 123, 254).astype(np.uint8))
    long_b = long_a[:-1] + bytes([long_a[-1] ^ 1])                 # 254 bytes, the last one apart
    names = [long_a, b"", long_b, long_a[:253], long_a, b"", long_b]
    flags = [0x41, 0x81, 0x41, 0x41, 0x81, 0x41, 0x91]
    path = write(tmp_path / "n.bam", rng, names, flags, [30] * 7)
    for kw in (dict(), dict(hash_bits=1), dict(name_suffix=True, hash_bits=2)):
        _, rep = check(gpu_lib, path, str(tmp_path), two_files=True, singletons=True, **kw)
        assert rep["pairs"] == 3 and rep["singletons"] == 1


# ---- 4. collisions and the run limit -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs_file(tmp_path_factory):
    """1200 records: the first 1200 of 700 names' records, most of them pairs, the rest of every other make-up
    (tools/fuzz_fastq_collate.GROUPS), shuffled, so that some mates fall behind the cut; and the same
    records in BGZF blocks of 7000 bytes, so that ingest chunks cut records."""
    d = tmp_path_factory.mktemp("pairs")
    rng = np.random.default_rng(45)
    base = list(dict.fromkeys(random_names(rng, 800)))[:700]
    names, flags = paired_reads(rng, base)
    names, flags = names[:1200], flags[:1200]
    assert len(names) == 1200
    hb = read_batch(rng, rng.integers(1, 160, len(names)), flags, rng.choice([0, 0, 1, 2], len(names)))
    paths = [str(d / "p.bam"), str(d / "p7000.bam")]
    bamio.write_bam(paths[0], hb, NAMES, LENS, with_index=False, names=names, sort_order="unsorted")
    bamio.write_bam(paths[1], hb, NAMES, LENS, with_index=False, names=names, sort_order="unsorted", block_payload=7000)
    want = model(paths[0], **ALL)
    assert want[4]["pairs"] > 300 and want[4]["singletons"] > 50 and want[4]["ambiguous"] > 0 and want[4]["reads_other"] > 0
    return paths, want


def same_as(want, got, rep):
    assert got == list(want[:4])
    assert all(rep[k] == v for k, v in want[4].items()), {k: (rep[k], v) for k, v in want[4].items() if rep[k] != v}


@pytest.mark.parametrize("bits", [1, 3])
def test_unlike_names_in_one_run(gpu_lib, tmp_path, pairs_file, bits):
    (path, _), want = pairs_file
    got, rep = convert(gpu_lib, path, str(tmp_path), hash_bits=bits, **ALL)
    same_as(want, got, rep)
    assert rep["name_collisions"] > 0                                       # the collision path ran: every run holds many names
    got0, rep0 = convert(gpu_lib, path, str(tmp_path), **ALL)
    assert got0 == got and rep0["name_collisions"] == 0


def test_run_limit(gpu_lib, tmp_path):
    """1024 reads of one name are accepted (singletons, all ambiguous), others of that name beside them do not count, 1025 are
    refused before the search."""
    rng = np.random.default_rng(46)
    flags = [0x41, 0x81] * 512
    ok = write(tmp_path / "ok.bam", rng, [b"same"] * 1074, flags + [0x01] * 50, [5] * 1074)
    _, rep = check(gpu_lib, ok, str(tmp_path), **ALL)
    assert (rep["pairs"], rep["singletons"], rep["ambiguous"], rep["reads_other"]) == (0, 1024, 1024, 50)
    over = write(tmp_path / "over.bam", rng, [b"same"] * 1025, flags + [0x41], [5] * 1025)
    with pytest.raises(host.NgsqError) as e:
        convert(gpu_lib, over, str(tmp_path), **ALL)
    assert e.value.code == ffi.ERR_LIMIT and e.value.message == "fastq --collate: more than 1024 reads share a name or a name hash"
    assert all(os.path.getsize(os.path.join(tmp_path, f)) == 0 for f in os.listdir(tmp_path) if f.startswith("c_"))


# ---- 5. batches, chunks, pieces, the budget -------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 7, 64, 997, 0])
def test_batch_edges(gpu_lib, tmp_path, pairs_file, batch):
    (path, cut), want = pairs_file
    got, rep = convert(gpu_lib, path, str(tmp_path), batch_records=batch, **ALL)
    same_as(want, got, rep)
    assert rep["batches"] >= (-(-1200 // batch) if batch else 1)
    if batch in (997, 0):
        got, rep = convert(gpu_lib, cut, str(tmp_path), batch_records=batch, **ALL)
        same_as(want, got, rep)


@pytest.mark.parametrize("piece", [1, 3, 64])
def test_piece_edges(gpu_lib, tmp_path, pairs_file, piece):
    (path, _), want = pairs_file
    got, rep = convert(gpu_lib, path, str(tmp_path), piece_records=piece, **ALL)
    same_as(want, got, rep)
    c = want[4]
    assert rep["pieces"] == sum(-(-c[k] // piece) for k in ("pairs", "singletons", "reads_other"))
    got1, rep1 = convert(gpu_lib, path, str(tmp_path), piece_records=piece, singletons=True)      # the interleaved file across piece edges
    want1 = model(path, singletons=True)
    same_as(want1, got1, rep1)
    assert rep1["pieces"] == -(-c["pairs"] // piece) + -(-c["singletons"] // piece)


def test_budget(gpu_lib, tmp_path, pairs_file):
    (path, _), want = pairs_file
    _, rep = convert(gpu_lib, path, str(tmp_path), **ALL)
    need = rep["resident_bytes"]
    assert need > rep["resident_records"] * gpu_lib.ngsq_collate_bytes_per_record() and rep["resident_records"] == 1200 - want[4]["excluded"] - want[4]["no_sequence"]
    got, rep = convert(gpu_lib, path, str(tmp_path), memory_budget=need, **ALL)
    same_as(want, got, rep)
    with pytest.raises(host.NgsqError) as e:
        convert(gpu_lib, path, str(tmp_path), memory_budget=need - 1, **ALL)
    assert e.value.code == ffi.ERR_LIMIT
    assert e.value.message == f"fastq --collate holds the kept records in device memory: {need} bytes needed, {need - 1} allowed"
    assert all(os.path.getsize(os.path.join(tmp_path, f)) == 0 for f in os.listdir(tmp_path) if f.startswith("c_"))


def test_num_records_around_a_pairs_second_record(gpu_lib, tmp_path):
    path = hand_order(tmp_path / "o.bam")
    for m, pairs in ((1, 0), (3, 0), (4, 1), (5, 2), (6, 2)):
        _, rep = check(gpu_lib, path, str(tmp_path), max_records=m, **ALL)
        assert rep["pairs"] == pairs and rep["records_scanned"] == min(m, 5)


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------
def test_score_above_93(gpu_lib, tmp_path, pairs_file):
    """The smallest index, whatever becomes of the record (a dropped singleton, a dropped other), and not a byte in a text output."""
    rng = np.random.default_rng(47)
    n = 3000
    names = [b"q%d" % (k // 2) for k in range(n)]
    hb = read_batch(rng, rng.integers(20, 120, n), [0x41, 0x91] * (n // 2), [0] * n)
    hb.cols["flag"][2001] = 0x11                                        # q1000 loses its read two to the others: 2000 is a singleton
    q, off = hb.cols["qual"], hb.cols["qual_off"]
    q[int(off[2000]) + 7] = 94
    q[int(off[2001]) + 1] = 200
    q[int(off[2500]) + 3] = 255
    path = str(tmp_path / "bad.bam")
    bamio.write_bam(path, hb, NAMES, LENS, with_index=False, names=names)
    for kw, index in ((dict(), 2000), (dict(two_files=True, batch_records=500), 2000), (dict(batch_records=2001, **ALL), 2000),
                      (dict(require_flags=1, exclude_flags=0x40, **ALL), 2001), (dict(max_records=2001, two_files=True, other=True), 2000)):
        assert model(path, **kw) == fm.error_message(index)
        with pytest.raises(host.NgsqError) as e:
            convert(gpu_lib, path, str(tmp_path), **kw)
        assert e.value.code == ffi.ERR_INVALID_ARGUMENT and e.value.message == fm.error_message(index)
        assert all(os.path.getsize(os.path.join(tmp_path, f)) == 0 for f in os.listdir(tmp_path) if f.startswith("c_"))
    check(gpu_lib, path, str(tmp_path), max_records=2000, **ALL)              # the records in front of it are fine
    _, rep = check(gpu_lib, path, str(tmp_path), require_flags=0x80, **ALL)   # records that are not kept are not checked: only the read twos are
    assert rep["singletons"] == 1499 and rep["pairs"] == 0


def test_a_failed_write_ends_the_call_with_its_message(gpu_lib, tmp_path):
    """/dev/full refuses every write: the message names the output."""
    import faulthandler
    faulthandler.dump_traceback_later(120, exit=True)
    try:
        path, _ = hand_names(tmp_path / "n.bam")
        for k, what in enumerate(("read one file", "read two file", "other reads file", "singletons file")):
            p = [str(tmp_path / f"w{j}.fastq") for j in range(4)]
            p[k] = "/dev/full"
            with pytest.raises(host.NgsqError) as e:
                host.bam_to_fastq_collated(path, p[0], p[1], p[2], p[3], piece_records=2, lib=gpu_lib)
            assert e.value.message == f"could not write record to {what}: No space left on device (os error 28)"
    finally:
        faulthandler.cancel_dump_traceback_later()


def test_bad_arguments_are_refused_before_anything_is_written(gpu_lib, tmp_path):
    path = hand_order(tmp_path / "o.bam")
    p = [str(tmp_path / f"a{j}.fastq") for j in range(4)]
    for kw, args in ((dict(exclude_flags=65536), p[:1]), (dict(require_flags=1 << 20), p[:1]), (dict(default_quality=94), p[:1]), (dict(bgzf_mask=2), p[:1]),
                     (dict(bgzf_mask=8), p[:3]), (dict(bgzf_mask=4), [p[0], p[1], None, p[3]]), (dict(bgzf_mask=16), p), (dict(name_suffix=2), p[:1]),
                     (dict(hash_bits=64), p[:1]), (dict(), [p[0], None, p[2]])):
        with pytest.raises(host.NgsqError) as e:
            host.bam_to_fastq_collated(path, *args, lib=gpu_lib, **kw)
        assert e.value.code == ffi.ERR_INVALID_ARGUMENT, kw
        assert all(os.path.getsize(x) == 0 for x in p if os.path.exists(x))


# ---- 7. compressed outputs and the command line ---------------------------------------------------------------------------------
def test_compressed_outputs_and_the_command_line(gpu_lib, ngs, tmp_path, pairs_file):
    (path, _), want = pairs_file
    got, rep = check(gpu_lib, path, str(tmp_path), bgzf_mask=15, piece_records=100, **ALL)      # (gunzips, looks for the EOF block)
    assert got == list(want[:4]) and rep["blocks"] >= 4 and all(c > 28 for c in rep["compressed_bytes"])
    half, rep_half = check(gpu_lib, path, str(tmp_path), bgzf_mask=10, effort="high", **ALL)
    assert half == got and rep_half["compressed_bytes"][0] == 0 and rep_half["compressed_bytes"][2] == 0
    # the command line: plain output is the library's, byte for byte; --gzip host and --gzip device gunzip to the same bytes
    p = [str(tmp_path / x) for x in ("c1.fastq", "c2.fq", "c3.fastq", "c4.fq")]
    r = run(ngs, "fastq", "--collate", path, p[0], p[1], "--other", p[2], "--singletons", p[3])
    assert r.returncode == 0, r.stderr
    assert [open(x, "rb").read() for x in p] == got
    c = want[4]
    assert f"{c['pairs']} pairs, {c['singletons']} singletons ({c['ambiguous']} ambiguous, 0 dropped), 0 other reads dropped" in r.stderr
    for where in ("host", "device"):
        z = [str(tmp_path / x) for x in (f"{where}1.fastq.gz", f"{where}2.fq.gz", f"{where}3.fastq", f"{where}4.fastq.gz")]
        r = run(ngs, "-v", "fastq", "--collate", "--gzip", where, path, z[0], z[1], "--other", z[2], "--singletons", z[3], "--collate-memory", "1G")
        assert r.returncode == 0, r.stderr
        assert "[ngs] fastq --collate: " in r.stderr
        raw = [open(x, "rb").read() for x in z]
        assert [gzip.decompress(raw[0]), gzip.decompress(raw[1]), raw[2], gzip.decompress(raw[3])] == got
        assert (raw[0].endswith(EOF) and raw[1].endswith(EOF) and raw[3].endswith(EOF)) == (where == "device")
    # one file, the suffix, -n, a budget too small, and nothing said with -q
    one = str(tmp_path / "i.fastq")
    r = run(ngs, "-q", "fastq", "--collate", "--name-suffix", "-n", "700", path, one)
    w = model(path, name_suffix=True, max_records=700)
    assert r.returncode == 0 and r.stderr == "" and open(one, "rb").read() == w[0]
    r = run(ngs, "fastq", "--collate", path, one)
    assert r.returncode == 0 and f"({c['ambiguous']} ambiguous, {c['singletons']} dropped), {c['reads_other']} other reads dropped" in r.stderr
    r = run(ngs, "fastq", "--collate", "--collate-memory", "1K", path, one)
    assert r.returncode == 1 and "Error: fastq --collate holds the kept records in device memory: " in r.stderr and "1024 allowed" in r.stderr
    assert os.path.getsize(one) == 0
    r = run(ngs, "-q", "fastq", "--collate", "-n", "0", "--gzip", "device", path, str(tmp_path / "z.fastq.gz"), "--singletons", str(tmp_path / "zs.fq.gz"))
    assert r.returncode == 0 and open(tmp_path / "z.fastq.gz", "rb").read() == EOF and open(tmp_path / "zs.fq.gz", "rb").read() == EOF


# ---- 8. round trip with the project's own tools ------------------------------------------------------------------------------
def test_round_trip_through_generate_and_convert(gpu_lib, ngs, tmp_path):
    """`ngs generate`'s pairs as SAM text with the /1 and /2 taken off the names and the records shuffled, converted to BAM:
    --collate --name-suffix gives every read back, the two files pair line by line, and the pairs come in the model's order."""
    rng = np.random.default_rng(48)
    fa = str(tmp_path / "ref.fasta")
    open(fa, "wb").write(gm.fasta_text([(b"a", gm.random_letters(rng, 60_000)), (b"b", gm.random_letters(rng, 30_000))], 80))
    g1, g2 = str(tmp_path / "g_1.fastq"), str(tmp_path / "g_2.fastq")
    host.generate([(fa, 100, 300.0, 30.0, 101, 1)], g1, g2, 7, 2000, lib=gpu_lib)
    r1, r2 = gm.parse_fastq(open(g1, "rb").read()), gm.parse_fastq(open(g2, "rb").read())
    assert len(r1) == len(r2) == 2000 and all(a[0].endswith(b"/1") and b[0] == a[0][:-2] + b"/2" for a, b in zip(r1, r2))
    comp = bytes.maketrans(b"ACGTN", b"TGCAN")
    lines = []
    for k, (a, b) in enumerate(zip(r1, r2)):
        for flag, (name, seq, qual) in ((77, a), (141, b)):
            if k % 2:
                flag, seq, qual = flag | 16, seq.translate(comp)[::-1], qual[::-1]
            lines.append(b"\t".join([name[:-2], b"%d" % flag, b"*", b"0", b"0", b"*", b"*", b"0", b"0", seq, qual]) + b"\n")
    lines = [lines[k] for k in rng.permutation(len(lines))]
    sam, bam = str(tmp_path / "u.sam"), str(tmp_path / "u.bam")
    open(sam, "wb").write(b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(lines))
    assert host.sam_to_bam(sam, bam, lib=gpu_lib)["records"] == 4000
    o1, o2 = str(tmp_path / "back_1.fastq"), str(tmp_path / "back_2.fastq")
    r = run(ngs, "fastq", "--collate", "--name-suffix", bam, o1, o2)
    assert r.returncode == 0, r.stderr
    assert "2000 pairs, 0 singletons" in r.stderr
    b1, b2 = open(o1, "rb").read(), open(o2, "rb").read()
    want = model(bam, two_files=True, name_suffix=True)
    assert (b1, b2) == want[:2]
    p1, p2 = gm.parse_fastq(b1), gm.parse_fastq(b2)
    assert all(a[0][:-2] == b[0][:-2] for a, b in zip(p1, p2))            # line by line
    assert sorted(p1) == sorted(r1) and sorted(p2) == sorted(r2)          # generate's reads, every one
    # plain `ngs fastq` on this file: the same reads, and two files that do not pair
    host.bam_to_fastq(bam, o1, o2, name_suffix=True, lib=gpu_lib)
    q1, q2 = gm.parse_fastq(open(o1, "rb").read()), gm.parse_fastq(open(o2, "rb").read())
    assert sorted(q1) == sorted(r1) and any(a[0][:-2] != b[0][:-2] for a, b in zip(q1, q2))


# ---- 9. a slice of the randomised sweep ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 6, 12, 18])
def test_fuzz_slice(gpu_lib, base):
    collate_sweep(gpu_lib, 6, base, verbose=False)
