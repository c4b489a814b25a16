"""`ngs markdup` on the GPU (include/ngsq_markdup.h): the decompressed output and every metric equal the
test-side model (tests/markdup_model.py) -- on the hand-worked files with and without --remove, with 0 to 2 records, around the
64 lanes of a wave, on reads whose QUAL sits on every edge of the score pass's loads, on CIGARs whose clip runs cross the lanes,
at the bounds of the packed end and beyond them, on runs of 5000 equal keys, at the run limit of the mate search and one beyond
it, with the name hash cut to one and three bits, over batches and ingest chunks that cut records, over pieces that cut records,
at the budget and one byte short of it, with a write that fails, at both encoder efforts, through the command line, in a chain
with `ngs index`, `ngs qc` and `ngs depth`, and on a slice of the randomised sweep of tools/fuzz_markdup.py."""
import ctypes as C
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from ngs_amd import build, ffi, host
from ngs_amd.genome_shape import grch38_no_alt
from tests import markdup_model as mm
from tests.test_markdup import (HAND_CLIPS_FLAGS, HAND_PAIRS_FLAGS, HAND_PAIRS_JSON, HAND_PAIRS_METRICS, HAND_PAIRS_REMOVED, flags_in, hand_clips, hand_pairs,
                                pair, q)
from tools.fuzz_markdup import EOF, check, convert, markdup_sweep, model, rec, write_bam

pytestmark = pytest.mark.gpu

GENOME = "GRCh38_no_alt_AnalysisSet"
H28 = ((1 << 28) - 1, "H")


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def run(ngs, *args):
    return subprocess.run([ngs, *args], capture_output=True, text=True, timeout=300)


def both(lib, path, d, **kw):
    """Marked and removed, each held to the model; the marked run's (bytes, report)."""
    check(lib, path, d, remove=True, **kw)
    return check(lib, path, d, **kw)


# ---- 1. hand files ----------------------------------------------------------------------------------------------------------
def test_hand_files(gpu_lib, tmp_path):
    d = str(tmp_path)
    p = write_bam(d + "/p.bam", hand_pairs())
    got, rep = check(gpu_lib, p, d)
    assert flags_in(got) == HAND_PAIRS_FLAGS and {k: rep[k] for k in HAND_PAIRS_METRICS} == HAND_PAIRS_METRICS      # (the literals of the CPU test)
    got, _ = check(gpu_lib, p, d, remove=True)
    assert flags_in(got) == HAND_PAIRS_REMOVED
    got, _ = both(gpu_lib, write_bam(d + "/c.bam", hand_clips()), d)
    assert flags_in(got) == HAND_CLIPS_FLAGS
    a, b = pair(b"a", 100, 300, 30, 30), pair(b"b", 100, 300, 30, 30)
    got, _ = both(gpu_lib, write_bam(d + "/t.bam", [a[1], b[1], b[0], a[0]]), d)
    assert flags_in(got) == [0x91, 0x491, 0x441, 0x41]
    fr = pair(b"a", 100, 300, 30, 30) + pair(b"b", 1, 399, 40, 40, f1=0x51, f2=0x81) + pair(b"c", 300, 100, 20, 20, f1=0x51, f2=0x81)
    got, _ = both(gpu_lib, write_bam(d + "/f.bam", fr), d)
    assert flags_in(got) == [0x41, 0x91, 0x51, 0x81, 0x451, 0x481]
    zero = [rec(b"z1", 0, 0, 50, "", q(30, 10)), rec(b"z2", 0x10, 0, 50, "", q(30, 10)), rec(b"z3", 0, 0, 50, "10M", q(20, 10)), rec(b"z4", 0x10, 0, 41, "10M", q(40, 10))]
    got, _ = both(gpu_lib, write_bam(d + "/z.bam", zero), d)
    assert flags_in(got) == [0x0, 0x410, 0x400, 0x10]
    cut = pair(b"a", 100, 300, 20, 20) + pair(b"b", 100, 300, 40, 40, f1=0x41, f2=0x91)
    got, rep = check(gpu_lib, write_bam(d + "/n.bam", cut), d, max_records=3)
    assert flags_in(got) == [0x41, 0x91, 0x441] and (rep["records"], rep["pairs"], rep["fragments"]) == (3, 1, 1)


# ---- 2. few records, and the lanes of a wave ------------------------------------------------------------------------------------
def test_few_records(gpu_lib, tmp_path):
    d = str(tmp_path)
    got, rep = both(gpu_lib, write_bam(d + "/e.bam", []), d)
    assert flags_in(got) == [] and rep["records"] == 0 and rep["pieces"] == 0 and rep["duplication"] == 0.0
    for recs in ([rec(b"a", 0, 0, 100, "10M", q(30, 10))], [rec(b"a", 0x4, -1, -1, "", q(30, 10))], pair(b"a", 100, 300, 30, 30),
                 [rec(b"a", 0, 0, 100, "10M", q(30, 10)), rec(b"b", 0, 0, 100, "10M", q(31, 10))]):
        both(gpu_lib, write_bam(d + "/k.bam", recs), d)
    _, rep = check(gpu_lib, d + "/k.bam", d, remove=True)
    assert rep["duplicate_fragments"] == 1 and rep["records"] == 2


@pytest.mark.parametrize("n", [63, 64, 65])
def test_records_around_a_wave(gpu_lib, tmp_path, n):
    """n fragments of two ends with rising scores (the last of each end survives), then n records that are n // 2 pairs of one
    key whose mates lie n // 2 apart."""
    d = str(tmp_path)
    frags = [rec(b"f%d" % k, 0, 0, 100 + 50 * (k % 2), "20M", q(15 + k % 60, 20)) for k in range(n)]
    _, rep = both(gpu_lib, write_bam(d + "/w.bam", frags), d)
    assert rep["duplicate_fragments"] == n - 2
    h = n // 2
    pairs = [rec(b"p%d" % k, 0x41, 0, 100, "20M", q(20 + k % 7, 20)) for k in range(h)] + [rec(b"p%d" % k, 0x91, 0, 300, "20M", q(20, 20)) for k in range(h)]
    pairs += [rec(b"odd", 0x41, 0, 100, "20M", q(40, 20))] * (n % 2)
    _, rep = both(gpu_lib, write_bam(d + "/x.bam", pairs), d)
    assert rep["pairs"] == h and rep["duplicate_pairs"] == h - 1 and rep["duplicate_fragments"] == n % 2


# ---- 3. the score pass's loads and tails -----------------------------------------------------------------------------------------
def test_scores_on_every_edge_of_the_loads(gpu_lib, tmp_path):
    """Reads of 1 to 1025 bases.  Every read has a rival on its own end, earlier in the file, whose QUAL differs in one byte at a
    random place by one score, so that a byte missed or counted twice anywhere turns the pair of them round.  Then the uniform
    QUALs: all 14 (nothing counts), all 15, all 93, and QUAL missing, each against the rival one byte away."""
    rng = np.random.default_rng(281)
    recs, site = [], 0

    def duel(ql_low, ql_high):
        nonlocal site
        site += 1
        l = len(ql_high) if ql_high is not None else len(ql_low)
        for name, ql in ((b"lo", ql_low), (b"hi", ql_high)):
            recs.append(rec(name + b"%d" % site, 0, 0, 1000 + 2 * site, f"{l}M", ql, l_seq=l, seq=bytes(rng.integers(0, 256, (l + 1) // 2).astype(np.uint8))))

    for l in (1, 63, 64, 65, 255, 256, 257, 1025):
        for _ in range(4):
            hi = rng.integers(0, 94, l).astype(np.uint8)
            at = int(rng.integers(0, l))
            hi[at] = max(int(hi[at]), 16)
            lo = hi.copy()
            lo[at] -= 1
            duel(bytes(lo), bytes(hi))
        for v in (15, 93):
            lo = bytearray([v]) * l
            lo[int(rng.integers(0, l))] -= 1
            duel(bytes(lo), bytes([v]) * l)
        hi = bytearray([14]) * l
        hi[int(rng.integers(0, l))] = 15
        duel(bytes([14]) * l, bytes(hi))                               # 0 against 15
        duel(None, bytes(hi))                                          # QUAL missing against 15
        duel(None, bytes([14]) * l)                                    # 0 against 0: the earlier record stays
    path = write_bam(str(tmp_path / "s.bam"), recs)
    got, rep = both(gpu_lib, path, str(tmp_path))
    flags = flags_in(got)
    assert rep["duplicate_fragments"] == len(recs) // 2
    # the last duel of every length is the tie: its first record stays; in every other duel the second stays
    per_len = len(recs) // 8
    for k in range(0, len(recs), 2):
        tie = (k % per_len) == per_len - 2
        assert (flags[k], flags[k + 1]) == ((0, 0x400) if tie else (0x400, 0)), k


# ---- 4. CIGARs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ops", [1, 2, 64, 65, 130])
def test_clip_runs_across_the_lanes(gpu_lib, tmp_path, n_ops):
    """A forward read whose leading run, and a reverse read whose trailing run, is n_ops - 1 clips of rising lengths, against a
    plain read on the same end; a reverse read whose span is spread over n_ops operations; a clip sum of 70 000."""
    clips = [(k + 1, "H") for k in range(n_ops - 2)] + ([(4, "S")] if n_ops > 1 else [])
    run_len = sum(n for n, _ in clips)
    l = 30 + (4 if n_ops > 1 else 0)
    recs = [rec(b"plain", 0, 0, 20000, "30M", q(30, 30)), rec(b"clipped", 0, 0, 20000 + run_len, clips + [(30, "M")], q(20, l)),
            rec(b"rplain", 0x10, 0, 40000, "30M", q(30, 30)), rec(b"rclipped", 0x10, 0, 40000 - run_len, [(30, "M")] + clips[::-1], q(20, l))]
    mid = [((k % 3) + 1, "MDI"[k % 3]) for k in range(n_ops)]
    span = sum(n for n, op in mid if op in "MD")
    query = sum(n for n, op in mid if op in "MI")
    recs += [rec(b"spread", 0x10, 0, 60000, mid, q(20, query)), rec(b"whole", 0x10, 0, 60000, f"{span}M", q(30, span))]
    recs += [rec(b"far", 0, 0, 170000, "70000H10M", q(20, 10)), rec(b"near", 0, 0, 100000, "10M", q(30, 10)),
             rec(b"rfar", 0x10, 0, 100000, "10M1000S69000H", q(14, 1010)), rec(b"rnear", 0x10, 0, 170000, "10M", q(30, 10))]
    got, rep = both(gpu_lib, write_bam(str(tmp_path / "c.bam"), recs), str(tmp_path))
    assert flags_in(got) == [0x0, 0x400, 0x10, 0x410, 0x410, 0x10, 0x400, 0x0, 0x410, 0x10] and rep["duplicate_fragments"] == 5


def test_the_bounds_of_the_packed_end(gpu_lib, tmp_path):
    d = str(tmp_path)
    low = [H28] * 4 + [(9, "H"), (10, "M")]                             # a leading run of 2^30 + 5
    high = [(10, "M")] + [H28] * 3 + [((1 << 28) - 12, "H")]            # a trailing run of 2^30 - 15
    ok = [rec(b"a", 0, 0, 5, low, q(30, 10)), rec(b"b", 0x10, 0, 5, high, q(30, 10)), rec(b"c", 0x10, 0, 5, high, q(20, 10))]
    got, _ = both(gpu_lib, write_bam(d + "/ok.bam", ok), d)                   # u = -2^30 and u = 2^30 - 1: the bounds themselves
    assert flags_in(got) == [0x0, 0x10, 0x410]
    for bad, index in (([ok[0], rec(b"x", 0x4, 0, 4, low, q(30, 10)), rec(b"y", 0x100, 0, 4, low, q(30, 10)), rec(b"z", 0, 0, 4, low, q(30, 10)), rec(b"w", 0, 0, 3, low, q(30, 10))], 3),
                       ([ok[1]] * 70 + [rec(b"z", 0x10, 0, 6, high, q(30, 10))] + [rec(b"w", 0x10, 0, 7, [H28] * 5, q(30, 10))] * 3, 70)):
        path = write_bam(d + "/bad.bam", bad)
        assert model(path) == mm.error_message(index)
        for kw in (dict(), dict(batch_records=2), dict(remove=True)):
            with pytest.raises(host.NgsqError) as e:
                convert(gpu_lib, path, d, **kw)
            assert e.value.code == ffi.ERR_LIMIT and e.value.message == mm.error_message(index)
            assert os.path.getsize(os.path.join(d, "m_out.bam")) == 0
        check(gpu_lib, path, d, max_records=index)                            # the records in front of it are fine


# ---- 5. long runs of keys, and the run limit of the mate search --------------------------------------------------------------------
def test_5000_identical_pairs_and_5000_identical_fragments(gpu_lib, tmp_path):
    d = str(tmp_path)
    recs = []
    for k in range(5000):
        recs += [rec(b"p%d" % k, 0x41, 0, 100, "20M", q(20 + (k * 7) % 13, 20)), rec(b"p%d" % k, 0x91, 1, 300, "20M", q(20, 20))]
    _, rep = check(gpu_lib, write_bam(d + "/p.bam", recs), d)
    assert (rep["pairs"], rep["duplicate_pairs"], rep["duplicate_fragments"]) == (5000, 4999, 0)
    frags = [rec(b"f%d" % k, 0x10, 2, 100, "20M", q(20 + (k * 7) % 13, 20)) for k in range(5000)]
    _, rep = check(gpu_lib, write_bam(d + "/f.bam", frags), d, remove=True)
    assert (rep["fragments"], rep["duplicate_fragments"]) == (5000, 4999)


def test_run_limit(gpu_lib, tmp_path):
    """1024 pair candidates of one name are accepted (fragments, all ambiguous); records of that name that are no pair candidates
    do not count; 1025 are refused before the search."""
    d = str(tmp_path)
    same = [rec(b"same", (0x41, 0x91)[k % 2], 0, 100 + k, "10M", q(30, 10)) for k in range(1024)]
    extra = [rec(b"same", 0x0, 0, 5000 + k, "10M", q(30, 10)) for k in range(50)]
    _, rep = check(gpu_lib, write_bam(d + "/ok.bam", same + extra), d)
    assert (rep["pairs"], rep["fragments"], rep["ambiguous"]) == (0, 1074, 1024)
    over = write_bam(d + "/over.bam", same + [rec(b"same", 0x41, 0, 9000, "10M", q(30, 10))])
    with pytest.raises(host.NgsqError) as e:
        convert(gpu_lib, over, d)
    assert e.value.code == ffi.ERR_LIMIT and e.value.message == "markdup: more than 1024 reads share a name or a name hash"
    assert os.path.getsize(os.path.join(d, "m_out.bam")) == 0


# ---- 6. a file of every kind of template: collisions, batches, pieces, the budget, the efforts ------------------------------------
@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    """A sweep case's records (tools/fuzz_markdup.markdup_case, seed 1000) in blocks of 60000 and of 7000 bytes, so that ingest
    chunks cut records, with the model's outputs."""
    from tools.fuzz_markdup import markdup_case
    from tests import bai_model as bm
    d = str(tmp_path_factory.mktemp("mixed"))
    case = markdup_case(1000, d)
    _blocks, stream, _ = bm.read_blocks(case["path"])
    cut = os.path.join(d, "cut.bam")
    from tests import bamio
    with open(cut, "wb") as f:
        for at in range(0, len(stream), 7000):
            f.write(bamio.bgzf_block(stream[at:at + 7000], 1))
        f.write(EOF)
    want = {r: model(case["path"], remove=r) for r in (False, True)}
    m = want[False][1]
    assert m["duplicate_pairs"] > 5 and m["duplicate_fragments"] > 5 and m["ambiguous"] > 0 and m["cleared"] > 0
    return (case["path"], cut), want, case["n"]


def same_as(want, raw, rep):
    assert raw.endswith(EOF)
    assert gzip.decompress(raw) == want[0]
    assert all(rep[k] == v for k, v in want[1].items()), {k: (rep[k], v) for k, v in want[1].items() if rep[k] != v}


@pytest.mark.parametrize("bits", [1, 3])
def test_unlike_names_in_one_run(gpu_lib, tmp_path, mixed, bits):
    (path, _), want, _ = mixed
    raw, rep = convert(gpu_lib, path, str(tmp_path), hash_bits=bits)
    same_as(want[False], raw, rep)
    assert rep["name_collisions"] > 0
    raw0, rep0 = convert(gpu_lib, path, str(tmp_path))
    assert gzip.decompress(raw0) == gzip.decompress(raw) and rep0["name_collisions"] == 0


@pytest.mark.parametrize("batch", [1, 7, 64, 997, 0])
def test_batch_edges(gpu_lib, tmp_path, mixed, batch):
    (path, cut), want, n = mixed
    remove = batch in (7, 997)
    raw, rep = convert(gpu_lib, cut, str(tmp_path), batch_records=batch, remove=remove)
    same_as(want[remove], raw, rep)
    assert rep["batches"] >= (-(-n // batch) if batch else 1)
    if batch in (997, 0):
        raw, rep = convert(gpu_lib, path, str(tmp_path), batch_records=batch)
        same_as(want[False], raw, rep)


@pytest.mark.parametrize("piece", [100, 333, 4096])
def test_pieces_that_cut_records(gpu_lib, tmp_path, mixed, piece):
    (path, _), want, _ = mixed
    for remove in (False, True):
        raw, rep = convert(gpu_lib, path, str(tmp_path), piece_bytes=piece, remove=remove)
        same_as(want[remove], raw, rep)
        assert rep["bam_bytes"] == len(want[remove][0]) and rep["pieces"] >= (len(want[remove][0]) - 400) // piece      # (the header is no piece's)


def test_budget(gpu_lib, tmp_path, mixed):
    (path, _), want, n = mixed
    _, rep = convert(gpu_lib, path, str(tmp_path))
    need = rep["resident_bytes"]
    assert need > n * gpu_lib.ngsq_markdup_bytes_per_record()
    raw, rep = convert(gpu_lib, path, str(tmp_path), memory_budget=need)
    same_as(want[False], raw, rep)
    with pytest.raises(host.NgsqError) as e:
        convert(gpu_lib, path, str(tmp_path), memory_budget=need - 1)
    assert e.value.code == ffi.ERR_LIMIT
    assert e.value.message == f"markdup holds the records in device memory: {need} bytes needed, {need - 1} allowed"
    assert os.path.getsize(os.path.join(tmp_path, "m_out.bam")) == 0


def test_gzip_effort_high(gpu_lib, tmp_path, mixed):
    (path, _), want, _ = mixed
    normal, rep_n = convert(gpu_lib, path, str(tmp_path))
    high, rep_h = convert(gpu_lib, path, str(tmp_path), effort="high")
    same_as(want[False], high, rep_h)
    assert gzip.decompress(normal) == gzip.decompress(high) and rep_h["blocks"] == rep_n["blocks"]


def test_a_failed_write_ends_the_call_with_its_message(gpu_lib, mixed):
    """/dev/full refuses every write."""
    import faulthandler
    faulthandler.dump_traceback_later(120, exit=True)
    try:
        (path, _), _, _ = mixed
        for kw in (dict(), dict(piece_bytes=1000, remove=True)):
            with pytest.raises(host.NgsqError) as e:
                host.bam_mark_duplicates(path, "/dev/full", lib=gpu_lib, **kw)
            assert e.value.message == "writing BAM record: No space left on device (os error 28)"
    finally:
        faulthandler.cancel_dump_traceback_later()


def test_bad_arguments_are_refused_before_anything_is_written(gpu_lib, tmp_path, mixed):
    (path, _), _, _ = mixed
    out = str(tmp_path / "o.bam")
    for kw in (dict(hash_bits=64), dict(remove=2)):
        with pytest.raises(host.NgsqError) as e:
            host.bam_mark_duplicates(path, out, lib=gpu_lib, **kw)
        assert e.value.code == ffi.ERR_INVALID_ARGUMENT and os.path.getsize(out) == 0


# ---- 7. the command line -----------------------------------------------------------------------------------------------------------
def test_the_command_line_against_the_library(gpu_lib, ngs, tmp_path, mixed):
    (path, _), want, n = mixed
    d = str(tmp_path)
    lib_raw, _ = convert(gpu_lib, path, d)
    out, met = d + "/cli.bam", d + "/cli.json"
    r = run(ngs, "-v", "markdup", path, out, "--metrics", met, "-t", "4")
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == lib_raw                                  # the library's file, byte for byte
    assert open(met).read() == mm.metrics_json(want[False][1]) and "[ngs] markdup: " in r.stderr
    m = want[False][1]
    assert f"{m['duplicate_records']} duplicate records of {n}: {m['duplicate_pairs']} duplicate pairs of {m['pairs']}" in r.stderr
    r = run(ngs, "markdup", path, out)
    assert r.returncode == 1 and "Error: refusing to overwrite existing output file: " in r.stderr and open(out, "rb").read() == lib_raw
    rem = d + "/rem.bam"
    r = run(ngs, "-q", "markdup", "--remove", "--gzip-effort", "high", "--memory", "1G", path, rem)
    assert r.returncode == 0 and r.stderr == "" and gzip.decompress(open(rem, "rb").read()) == want[True][0]
    cut = d + "/n.bam"
    r = run(ngs, "-q", "markdup", "-n", "700", path, cut)
    assert r.returncode == 0 and gzip.decompress(open(cut, "rb").read()) == model(path, max_records=700)[0]
    # the hand file's document as a literal
    hand = write_bam(d + "/hand.bam", hand_pairs())
    r = run(ngs, "-q", "markdup", hand, d + "/hand_out.bam", "--metrics", d + "/hand.json")
    assert r.returncode == 0 and open(d + "/hand.json").read() == HAND_PAIRS_JSON
    # every error removes the output: a budget too small, an end that cannot be packed
    r = run(ngs, "markdup", "--memory", "1K", path, d + "/small.bam")
    assert r.returncode == 1 and "Error: markdup holds the records in device memory: " in r.stderr and "1024 allowed" in r.stderr
    bad = write_bam(d + "/bad.bam", [rec(b"z", 0, 0, 4, [H28] * 4 + [(9, "H"), (10, "M")], q(30, 10))])
    r = run(ngs, "markdup", bad, d + "/bad_out.bam", "--metrics", d + "/bad.json")
    assert r.returncode == 1 and "Error: " + mm.error_message(0) in r.stderr
    assert not any(os.path.exists(d + x) for x in ("/small.bam", "/bad_out.bam", "/bad.json"))


# ---- 8. in a chain with the project's own tools -----------------------------------------------------------------------------------
def test_chain_with_index_qc_and_depth(gpu_lib, ngs, tmp_path):
    """The synthetic writer's sorted file over the GRCh38 header: marked, indexed and counted, the General facet's duplicate
    count is the model's; the depth of the marked file under the default exclude flags is the depth of the --remove file."""
    d = str(tmp_path)
    names, lens, _ = grch38_no_alt()
    src = d + "/s.bam"
    cfg = host.synth_config(20000, read_len=150, genome=lens, file_style=ffi.SYNTH_FILE_REALISTIC, lib=gpu_lib)
    arr = (C.c_char_p * len(names))(*[x.encode() for x in names])
    assert gpu_lib.ngsq_synth_write_bam_named(C.byref(cfg), arr, src.encode(), 20000, 1, 0) == 0, gpu_lib.ngsq_bam_last_error()
    want = model(src)
    marked_path, removed = d + "/marked.bam", d + "/removed.bam"
    r = run(ngs, "-q", "markdup", src, marked_path)
    assert r.returncode == 0, r.stderr
    assert gzip.decompress(open(marked_path, "rb").read()) == want[0]
    assert run(ngs, "-q", "markdup", "--remove", src, removed).returncode == 0
    assert run(ngs, "-q", "index", marked_path).returncode == 0
    r = run(ngs, "-q", "qc", marked_path, GENOME, "-o", d + "/qc")
    assert r.returncode == 0, r.stderr[-2000:]
    doc = json.load(open(d + "/qc/marked.bam.results.json"))
    assert doc["general"]["records"]["duplicate"] == want[1]["duplicate_records"]
    depths = [subprocess.run([ngs, "-q", "depth", p], capture_output=True, timeout=300) for p in (marked_path, removed)]
    assert depths[0].returncode == 0 and depths[1].returncode == 0, depths[0].stderr
    assert depths[0].stdout == depths[1].stdout and len(depths[0].stdout) > 1000


# ---- 9. a slice of the randomised sweep ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 6, 12, 18])
def test_fuzz_slice(gpu_lib, base):
    markdup_sweep(gpu_lib, 6, base, verbose=False)
