"""The device DEFLATE encoder at high effort (include/ngsq_bgzf.h: ngsq_bgzf_set_effort): candidates
inside a position's own tile, several candidates along a hash chain, the lazy step of the parse, and the choice per block that
keeps a block from ever being larger than at normal effort.  Every output is checked the three ways of
tests/test_bgzf_deflate_gpu.py (the model's walk, gzip.decompress, the device inflater with its CRC check); what the match
search found is read from the tokens (tests/deflate_tokens.py)."""
import ctypes as C
import gzip
import os
import subprocess
import zlib

import numpy as np
import pytest

from ngs_amd import build, ffi, host
from tests import bam_sort_model as bsm
from tests import bam_text_model as tm
from tests import bgzf_model as bm
from tests import deflate_tokens as dt
from tests import generate_model as gm
from tests import sort_model as som
from tests import sort_rounds_model as srm
from tests.test_bam_sort_gpu import bam_of
from tests.test_bgzf_deflate_gpu import check, de_bruijn, deflate, mixed, random_bytes, text
from tests.test_sam_sort_gpu import shuffled
from tests.test_sam_to_bam import random_sam
from tests.test_sort_rounds_gpu import constants

pytestmark = pytest.mark.gpu

B = bm.BLOCK_INPUT
NORMAL, HIGH = ffi.BGZF_EFFORT_NORMAL, ffi.BGZF_EFFORT_HIGH


def context(lib, effort=None):
    c = host.QcContext([1000], [1], lib=lib)
    if effort is not None:
        assert lib.ngsq_bgzf_set_effort(c._ctx, effort) == 0
    return c


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    c = context(gpu_lib)
    yield c
    c.close()


@pytest.fixture(scope="module")
def high(gpu_lib):
    c = context(gpu_lib, HIGH)
    yield c
    c.close()


@pytest.fixture(scope="module")
def high2(gpu_lib):
    c = context(gpu_lib, HIGH)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def tokens_of(comp: bytes, blocks, k: int = 0):
    data, toks = dt.member_tokens(comp, blocks[k])
    return data, toks


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi(gpu_lib, ctx):
    lib = gpu_lib
    rng = np.random.default_rng(1)
    data = mixed(rng, 3)
    a, b = context(lib), context(lib)
    try:
        assert lib.ngsq_bgzf_effort(a._ctx) == NORMAL and lib.ngsq_bgzf_effort(None) == NORMAL     # a context that was never told
        default = deflate(lib, a, data)[0]
        assert default == deflate(lib, ctx, data)[0]
        assert lib.ngsq_bgzf_set_effort(a._ctx, NORMAL) == 0 and deflate(lib, a, data)[0] == default
        assert lib.ngsq_bgzf_set_effort(a._ctx, HIGH) == 0 and lib.ngsq_bgzf_effort(a._ctx) == HIGH
        hi = check(lib, a, data)[0]
        assert hi != default and len(hi) <= len(default)
        assert lib.ngsq_bgzf_set_effort(a._ctx, NORMAL) == 0 and lib.ngsq_bgzf_effort(a._ctx) == NORMAL
        assert deflate(lib, a, data)[0] == default                                             # high, then back: the default bytes again
        for bad in (2, 3, 0xFFFFFFFF):
            assert lib.ngsq_bgzf_set_effort(a._ctx, bad) == ffi.ERR_INVALID_ARGUMENT
            assert b"effort" in lib.ngsq_last_error(a._ctx) and lib.ngsq_bgzf_effort(a._ctx) == NORMAL
        assert lib.ngsq_bgzf_set_effort(None, HIGH) == ffi.ERR_INVALID_ARGUMENT
        # two contexts of different efforts, used alternately
        assert lib.ngsq_bgzf_set_effort(b._ctx, HIGH) == 0
        for _ in range(2):
            assert deflate(lib, a, data)[0] == default and deflate(lib, b, data)[0] == hi
        assert lib.ngsq_bgzf_effort(a._ctx) == NORMAL and lib.ngsq_bgzf_effort(b._ctx) == HIGH
        # unknown flags are refused as before, at either effort
        n = C.c_uint64(0)
        out = np.empty(1 << 20, np.uint8)
        assert lib.ngsq_bgzf_deflate_device(b._ctx, data, len(data), out.ctypes.data, len(out), C.byref(n), 2, None) == ffi.ERR_INVALID_ARGUMENT
        assert host.bgzf_deflate(data, lib=lib)[0] == default and host.bgzf_deflate(data, lib=lib, effort="high")[0] == hi
        with pytest.raises(ValueError):
            host.bgzf_deflate(data, lib=lib, effort="best")
    finally:
        a.close()
        b.close()


# ---- 2. lengths ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 65279, 65280, 65281])
def test_lengths(gpu_lib, high, n):
    rng = np.random.default_rng(n)
    comp, blocks, _ = check(gpu_lib, high, text(rng, n))
    if n == 0:
        assert comp == bm.EOF_BLOCK
    if n >= 4095:
        assert all(b.btype == 2 for b in blocks[:-1]) and len(comp) < n
    check(gpu_lib, high, random_bytes(rng, n))


# ---- 3. reach inside the tile -------------------------------------------------------------------------------------------------------
def pair(rng, d: int, second: int, total: int = 2048):
    """R (100 bytes over 256 values) and R again, d bytes on, at `second`, in a filler of sixteen values.  Below d = 100 the two
    overlap: what repeats at distance d is then R's first d bytes, over the same 100 positions."""
    R = random_bytes(rng, 100)
    period = (R + random_bytes(rng, max(d - 100, 0), 16))[:d]
    period = period[:-1] + bytes([period[-1] or 1])                             # the bytes in front of the two copies differ:
    first = second - d                                                          # the match begins in the second copy
    assert first >= 1 and second + 100 < total
    body = period + (period * 2)[:100]
    data = random_bytes(rng, first - 1, 16) + b"\x00" + body + random_bytes(rng, total - first - len(body), 16)
    assert len(data) == total and data[second:second + 100] == data[first:first + 100] and data[second - 1] != data[first - 1]
    return data


def reaches(toks, second: int, d: int) -> bool:
    return any(m.distance == d and m.length >= 96 and second <= m.start < second + 100 for m in dt.matches(toks))


PLACES = {"one tile": lambda d: 522 + d, "pair across an edge": lambda d: 1024 + 7, "copy across an edge": lambda d: 1024 - 50,
          "lane 0": lambda d: 1152, "lane 63": lambda d: 1215}


@pytest.mark.parametrize("d", [64, 65, 127, 200, 511, 512, 513])
def test_reach_inside_the_tile(gpu_lib, ctx, high, d):
    for k, (place, at) in enumerate(PLACES.items()):
        second = at(d)
        one_tile = (second - d) // 512 == (second + 99) // 512
        if place == "one tile" and not one_tile:
            continue                                                            # (d + 100 > 512: no tile holds both)
        data = pair(np.random.default_rng(1000 * d + k), d, second)
        comp, blocks, _ = check(gpu_lib, high, data)
        assert blocks[0].btype == 2
        got, toks = tokens_of(comp, blocks)
        assert got == data and reaches(toks, second, d), (d, place, dt.matches(toks)[-8:])
        if one_tile:
            # normal effort looks at earlier tiles only: the behaviour that is pinned, and what tells the two efforts apart
            comp_n, blocks_n, _ = check(gpu_lib, ctx, data)
            assert not reaches(tokens_of(comp_n, blocks_n)[1], second, d), (d, place)
            assert len(comp) < len(comp_n)


# ---- 4. the chain and the distance limit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distance", [32768, 32769, 40000])
def test_chain_and_the_distance_limit(gpu_lib, high, distance):
    """R at 0, a decoy that shares R's first four bytes and nothing more at 30000, R again at `distance`: the table's candidate
    is the decoy, the long match lies one link further, legal at 32768 and at no greater distance."""
    rng = np.random.default_rng(distance)
    R = random_bytes(rng, 100)
    decoy = R[:4] + bytes([R[4] ^ 0xFF]) + random_bytes(rng, 40)
    data = R + random_bytes(rng, 30000 - 100, 16) + decoy + random_bytes(rng, distance - 30000 - len(decoy), 16) + R + random_bytes(rng, 200, 16)
    assert data[distance:distance + 100] == R and data[30000:30004] == R[:4]
    comp, blocks, rep = check(gpu_lib, high, data)                                # (a distance too far back: zlib, gzip and the inflater refuse)
    assert blocks[0].btype == 2
    got, toks = tokens_of(comp, blocks)
    assert got == data
    ms = dt.matches(toks)
    assert all(m.distance <= 32768 for m in ms)
    long = [m for m in ms if distance <= m.start < distance + 100 and m.length >= 96]
    if distance == 32768:
        assert long and long[0].distance == 32768, ms[-8:]
    else:
        assert not long
    print(f"distance {distance}: {len(comp)} bytes, {rep.matches} matches")


# ---- 5. the lazy step ------------------------------------------------------------------------------------------------------------------
def lazy_instance(rng, letters: bytes) -> bytes:
    """`abcd`, junk, `bcdefghijklmnopq`, junk, `abcdefghijklmnopq` (the letters are seventeen byte values): the last string
    begins 140 bytes behind `abcd` and 77 behind `bcde...`, both further than a wave."""
    assert len(letters) == 17
    return letters[:4] + random_bytes(rng, 60) + letters[1:] + random_bytes(rng, 60) + letters


LAZY_AT, LAZY_LEN = 140, 157


def lazy_input(rng, special: str):
    """(data, the positions of every `abcdefghijklmnopq`).  Zeros (so that the block is dynamic), then instances between
    stretches of 256-valued random bytes (so that literals are dear and a match of four pays).  special: where the fourth
    instance's `a` lies -- "plain", "tile" (on the last byte of a 4 KiB parse tile), or "end0" to "end3" (the string ends that
    many bytes before the end of the block)."""
    values = rng.permutation(256).astype(np.uint8)
    parts, at = [b"\x00" * 1200], []
    size = lambda: sum(len(x) for x in parts)
    n_inst = 4 if special.startswith("end") else 7
    for k in range(n_inst):
        gap = 300
        if special == "tile" and k == 3:
            gap = 4095 - LAZY_AT - size()
            assert gap >= 0
        parts.append(random_bytes(rng, gap))
        at.append(size() + LAZY_AT)
        parts.append(lazy_instance(rng, values[17 * k:17 * k + 17].tobytes()))
    if special.startswith("end"):
        parts.append(random_bytes(rng, int(special[3:])))
    data = b"".join(parts)
    if special == "tile":
        assert at[3] == 4095
    if special.startswith("end"):
        assert at[3] + 17 + int(special[3:]) == len(data)
    return data, at


@pytest.mark.parametrize("special", ["plain", "tile", "end0", "end1", "end2", "end3"])
def test_lazy_step(gpu_lib, high, special):
    data, at = lazy_input(np.random.default_rng(len(special) * 7 + ord(special[-1])), special)
    comp, blocks, _ = check(gpu_lib, high, data)
    assert blocks[0].btype == 2 and len(blocks) == 1
    got, toks = tokens_of(comp, blocks)
    assert got == data
    starts, p = {}, 0
    for t in toks:
        starts[p] = t
        p += t.length if isinstance(t, dt.Match) else 1
    for a in at:
        lit, m = starts.get(a), starts.get(a + 1)
        assert lit == data[a] and not isinstance(lit, dt.Match), (special, a, lit)          # the literal `a` ...
        assert isinstance(m, dt.Match) and m.length >= 16 and m.distance == 77, (special, a, m)  # ... and one match of `bcdefghijklmnopq`


# ---- 6. blocks are independent ---------------------------------------------------------------------------------------------------------
def test_no_match_across_blocks(gpu_lib, high):
    rng = np.random.default_rng(3)
    R = random_bytes(rng, 100)
    data = random_bytes(rng, B - 100, 16) + R + R + random_bytes(rng, 3000, 16)
    comp, blocks, _ = check(gpu_lib, high, data)
    second = comp[blocks[1].offset:blocks[1].offset + blocks[1].size]
    assert zlib.decompress(second[18:-8], -15) == data[B:]                        # alone, with no history
    assert all(m.distance <= m.start for m in dt.matches(dt.member_tokens(comp, blocks[1])[1]))


# ---- 7. code shapes ------------------------------------------------------------------------------------------------------------------
def test_code_shapes(gpu_lib, high):
    rng = np.random.default_rng(4)
    seq = bytes(97 + x for x in de_bruijn(16, 4)[:20000])                         # every window of four is met once: no match anywhere
    _, blocks, rep = check(gpu_lib, high, seq)
    assert blocks[0].btype == 2 and rep.matches == 0 and rep.tokens == len(seq)
    _, _, rep = check(gpu_lib, high, b"\x00" * (1 + 3 * 258))                     # only matches behind the first literal
    assert (rep.tokens, rep.matches) == (4, 3)
    _, blocks, rep = check(gpu_lib, high, random_bytes(rng, B))
    assert blocks[0].btype == 0 and blocks[0].size == B + 31 and rep.stored_blocks == 1
    check(gpu_lib, high, b"aaaaa")
    check(gpu_lib, high, b"J" * B)


# ---- 8. the grid, determinism -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(gpu_lib, high):
    data = mixed(np.random.default_rng(6), 257)
    return data, check(gpu_lib, high, data)[0]


@pytest.mark.parametrize("n_blocks", [3, 65])
def test_the_bytes_do_not_depend_on_the_grid(gpu_lib, high, many, n_blocks):
    data, comp_all = many
    comp, blocks, _ = check(gpu_lib, high, data[:n_blocks * B])
    assert len(blocks) == n_blocks
    assert comp[:-28] == comp_all[:len(comp) - 28]


def test_deterministic(gpu_lib, high, high2):
    data = mixed(np.random.default_rng(8), 5)
    first = deflate(gpu_lib, high, data)[0]
    for c in (high2, high, high2):
        assert deflate(gpu_lib, c, data)[0] == first


# ---- 9. never larger than normal ------------------------------------------------------------------------------------------------------
def test_never_larger_than_normal(gpu_lib, ctx, high, tmp_path):
    """Per input and, as the encoder sizes both parses of every block and emits the smaller, per member.  The sizes beside
    zlib's at the same block size are printed."""
    sam = random_sam(61, 3000, tmp_path)
    rng = np.random.default_rng(62)
    fa = str(tmp_path / "f.fa")
    open(fa, "wb").write(gm.fasta_text([(b"chr1", gm.random_letters(rng, 100_000))], 60))
    p1, p2 = str(tmp_path / "f_1.fastq"), str(tmp_path / "f_2.fastq")
    host.generate([(fa, 1000, 200.0, 30.0, 150, 1)], p1, p2, 11, 200, lib=gpu_lib)
    inputs = [("BAM stream", tm.bam_stream(sam)), ("SAM text", sam), ("generator FASTQ", open(p1, "rb").read()),
              ("word text", text(rng, 3 * B + 1000)), ("mixed corpus", mixed(rng, 5))]
    for name, data in inputs:
        comp_n, blocks_n, _ = check(gpu_lib, ctx, data)
        comp_h, blocks_h, rep = check(gpu_lib, high, data)
        z = [bm.zlib_size(data, level) for level in (1, 6, 9)]
        n, h = len(comp_n) - 28, len(comp_h) - 28
        print(f"{name} {len(data)} bytes: normal {n}, high {h} (high/normal {h / n:.4f}), zlib -1 {z[0]} (high/zlib {h / z[0]:.3f}), "
              f"-6 {z[1]} ({h / z[1]:.3f}), -9 {z[2]} ({h / z[2]:.3f}); {rep.tokens} tokens, {rep.matches} matches at high")
        assert h <= n, name
        assert len(blocks_h) == len(blocks_n) and all(a.size <= b.size for a, b in zip(blocks_h, blocks_n)), name
        if name == "BAM stream":
            assert h < n


# ---- 10. the writers, through the command line -----------------------------------------------------------------------------------------
def run(ngs, *args):
    r = subprocess.run([ngs, *args], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stderr.decode()


DEVICE_HIGH = ["--gzip", "device", "--gzip-effort", "high"]


def test_sam_to_bam_through_the_command_line(gpu_lib, ngs, tmp_path):
    sam = random_sam(63, 2000, tmp_path)
    src, out, normal, back = (str(tmp_path / x) for x in ("in.sam", "high.bam", "normal.bam", "back.sam"))
    open(src, "wb").write(sam)
    assert " compressed at effort high; " in run(ngs, "convert", "-v", *DEVICE_HIGH, src, out)
    assert " compressed at effort normal; " in run(ngs, "convert", "-v", "--gzip", "device", src, normal)
    raw = open(out, "rb").read()
    assert gzip.decompress(raw) == tm.bam_stream(sam) and bm.walk(raw)[0] == tm.bam_stream(sam)
    assert len(raw) < os.path.getsize(normal)
    lib_normal = str(tmp_path / "lib.bam")
    host.sam_to_bam(src, lib_normal, lib=gpu_lib)
    assert open(normal, "rb").read() == open(lib_normal, "rb").read()            # `normal` and no flag: the same bytes
    host.sam_to_bam(src, lib_normal, lib=gpu_lib, effort="high")
    assert open(lib_normal, "rb").read() == raw                                  # the library call is the command
    run(ngs, "convert", out, back)
    assert open(back, "rb").read() == sam


def indexed_by_ngs_index(ngs, out: str) -> bytes:
    """The index `ngs index` writes for the BAM at `out`, whose own index is kept where it is."""
    os.rename(out + ".bai", out + ".kept")
    try:
        run(ngs, "index", out)
        return open(out + ".bai", "rb").read()
    finally:
        os.replace(out + ".kept", out + ".bai")


def test_sorted_bam_with_index_through_the_command_line(gpu_lib, ngs, tmp_path):
    sam = shuffled(random_sam(64, 1500, tmp_path), 5)
    bam = bam_of(shuffled(random_sam(65, 1500, tmp_path), 6), 7000)
    src_sam, src_bam = str(tmp_path / "in.sam"), str(tmp_path / "in.bam")
    open(src_sam, "wb").write(sam)
    open(src_bam, "wb").write(bam)
    sorted_high = ["convert", "-v", *DEVICE_HIGH, "--sort", "coordinate", "--write-index"]
    for src, want, name in ((src_sam, som.bam_stream(sam), "s"), (src_bam, bsm.bam_stream(bam), "b")):
        out, normal = str(tmp_path / (name + ".bam")), str(tmp_path / (name + ".normal.bam"))
        assert " compressed at effort high; " in run(ngs, *sorted_high, src, out)
        run(ngs, "convert", "--gzip", "device", "--sort", "coordinate", "--write-index", src, normal)
        raw = open(out, "rb").read()
        assert gzip.decompress(raw) == want and bm.walk(raw)[0] == want
        assert len(raw) < os.path.getsize(normal)
        bai = open(out + ".bai", "rb").read()
        assert bai == indexed_by_ngs_index(ngs, out)                              # the block offsets moved with the block sizes
        assert bai != open(normal + ".bai", "rb").read()
    # the shuffled BAM again in rounds: the bytes of the in-memory output, BAM and BAI
    per, _ = constants(gpu_lib)
    plan = srm.plan_of(bam, 64 << 10, per)
    assert len(plan) >= 3
    rounds = str(tmp_path / "rounds.bam")
    err = run(ngs, *sorted_high, "--sort-memory", "64K", src_bam, rounds)
    assert f"[ngs] convert: {len(plan)} rounds over " in err and " compressed at effort high; " in err
    assert open(rounds, "rb").read() == open(str(tmp_path / "b.bam"), "rb").read()
    assert open(rounds + ".bai", "rb").read() == open(str(tmp_path / "b.bam.bai"), "rb").read()


def test_generate_through_the_command_line(gpu_lib, ngs, tmp_path):
    rng = np.random.default_rng(66)
    fa = str(tmp_path / "g.fa")
    open(fa, "wb").write(gm.fasta_text([(b"chr1", gm.random_letters(rng, 50_000))], 60))
    provider = f"{fa}:100:200:30:150:1"
    z = [str(tmp_path / x) for x in ("h_1.fastq.gz", "h_2.fastq.gz")]
    zn = [str(tmp_path / x) for x in ("n_1.fastq.gz", "n_2.fastq.gz")]
    plain = [str(tmp_path / x) for x in ("p_1.fastq", "p_2.fastq")]
    err = run(ngs, "generate", "-v", "-n", "1500", "--seed", "17", *DEVICE_HIGH, *z, provider)
    assert "BGZF on the device at effort high: " in err
    run(ngs, "generate", "-n", "1500", "--seed", "17", "--gzip", "device", *zn, provider)
    run(ngs, "generate", "-n", "1500", "--seed", "17", *plain, provider)
    for zh, znorm, p in zip(z, zn, plain):
        raw, want = open(zh, "rb").read(), open(p, "rb").read()
        assert len(want) > 3 * B and gzip.decompress(raw) == want and bm.walk(raw)[0] == want
        assert len(raw) <= os.path.getsize(znorm)
    lib1, lib2 = str(tmp_path / "l_1.fastq.gz"), str(tmp_path / "l_2.fastq.gz")
    host.generate([(fa, 100, 200.0, 30.0, 150, 1)], lib1, lib2, 17, 1500, lib=gpu_lib, bgzf=True, effort="high")
    assert open(lib1, "rb").read() == open(z[0], "rb").read() and open(lib2, "rb").read() == open(z[1], "rb").read()
