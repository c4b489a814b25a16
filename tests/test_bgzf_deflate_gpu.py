"""The device DEFLATE encoder (include/ngsq_bgzf.h).  Every output is checked three ways: the model
(tests/bgzf_model.py: framing, zlib's inflate of every payload, CRC32, ISIZE, the data), gzip.decompress of the whole buffer, and
the library's own device inflater with its CRC check, which has to give the input back."""
import ctypes as C
import gzip
import zlib

import numpy as np
import pytest

from ngs_amd import ffi, host
from tests import bgzf_model as bm
from tests import generate_model as gm

pytestmark = pytest.mark.gpu

B = bm.BLOCK_INPUT


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    c = host.QcContext([1000], [1], lib=gpu_lib)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx2(gpu_lib):
    c = host.QcContext([1000], [1], lib=gpu_lib)
    yield c
    c.close()


def deflate(lib, ctx, data: bytes, eof: bool = True):
    flags = ffi.BGZF_EOF if eof else 0
    cap = lib.ngsq_bgzf_deflate_bound(len(data), flags)
    out = np.empty(max(cap, 1), np.uint8)
    n = C.c_uint64(0)
    rep = ffi.BgzfDeflateReport()
    rc = lib.ngsq_bgzf_deflate_device(ctx._ctx, data, len(data), out.ctypes.data, cap, C.byref(n), flags, C.byref(rep))
    assert rc == 0, (lib.ngsq_last_error(ctx._ctx) or b"").decode()
    assert n.value <= cap
    return bytes(out[:n.value]), rep


def inflate(lib, ctx, comp: bytes, n: int) -> bytes:
    out = np.empty(max(n, 1), np.uint8)
    got = C.c_uint64(0)
    rc = lib.ngsq_bgzf_inflate_device(ctx._ctx, comp, len(comp), out.ctypes.data, n, C.byref(got), 1)
    assert rc == 0, (lib.ngsq_last_error(ctx._ctx) or b"").decode()
    return bytes(out[:got.value])


def check(lib, ctx, data: bytes):
    """Compress, check three ways; (stream, blocks without the EOF block, report)."""
    comp, rep = deflate(lib, ctx, data)
    got, blocks = bm.walk(comp)
    assert got == data
    assert gzip.decompress(comp) == data
    assert inflate(lib, ctx, comp, len(data)) == data
    assert blocks[-1].eof and not any(b.eof for b in blocks[:-1])
    blocks = blocks[:-1]
    assert [b.isize for b in blocks] == [min(B, len(data) - i) for i in range(0, len(data), B)]
    assert rep.blocks == len(blocks) and rep.in_bytes == len(data) and rep.out_bytes == len(comp)
    assert rep.stored_blocks == sum(b.btype == 0 for b in blocks)
    for b in blocks:
        assert b.btype in (0, 2) and b.size <= b.isize + 31
    return comp, blocks, rep


def text(rng, n: int) -> bytes:
    words = [b"read", b"chr1", b"ACGT", b"TTGACCA", b"\t", b"\n", b"IIIIHHHGG#", b"0123", b"flag", b" the "]
    out = b"".join(words[k] for k in rng.integers(0, len(words), n // 3 + 8))
    return out[:n]


def random_bytes(rng, n: int, values: int = 256) -> bytes:
    return rng.integers(0, values, n, dtype=np.uint8).tobytes()


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 257, 258, 259, 4095, 4096, 4097, 65279, 65280, 65281, 2 * 65280 + 1])
def test_lengths(gpu_lib, ctx, n):
    rng = np.random.default_rng(n)
    comp, blocks, _ = check(gpu_lib, ctx, text(rng, n))
    if n == 0:
        assert comp == bm.EOF_BLOCK
    if n >= 4095:
        assert all(b.btype == 2 for b in blocks[:-1]) and len(comp) < n
    check(gpu_lib, ctx, random_bytes(rng, n))


@pytest.mark.parametrize("n", [3, 4, 258, 259, 260, 261, 516, 517, 65280])
def test_runs_of_one_value(gpu_lib, ctx, n):
    comp, blocks, rep = check(gpu_lib, ctx, b"J" * n)
    if n == 65280:
        # one literal and 253 matches of 258 and one of 5, or a few more where tokens are cut: at most 28 bits each, beside a
        # header of 74 + 316 * 7 bits
        assert len(comp) - 28 < 1024


def test_runs_across_the_tile_edge_and_up_to_the_block_end(gpu_lib, ctx):
    rng = np.random.default_rng(2)
    check(gpu_lib, ctx, random_bytes(rng, 4090, 16) + b"J" * 300 + random_bytes(rng, 1000, 16))
    check(gpu_lib, ctx, random_bytes(rng, B - 300, 16) + b"J" * 300 + random_bytes(rng, 500, 16))  # ends with block 0; J is no byte of block 1
    check(gpu_lib, ctx, random_bytes(rng, B - 300, 16) + b"J" * 600)                                # goes on in block 1
    check(gpu_lib, ctx, b"J" * (1 + 3 * 258) + b"ab")


@pytest.mark.parametrize("distance", [32768, 32769, 40000])
def test_the_distance_limit(gpu_lib, ctx, distance):
    """R, a filler of sixteen values (so that the block is dynamic and R's 256 values are dear), R again: a match is legal at
    32768 and at no greater distance; a reader answers one with 'invalid distance too far back' or an invalid code."""
    rng = np.random.default_rng(distance)
    R = random_bytes(rng, 100)
    data = R + random_bytes(rng, distance - 100, 16) + R + random_bytes(rng, 200, 16)
    comp, blocks, rep = check(gpu_lib, ctx, data)
    assert blocks[0].btype == 2
    print(f"distance {distance}: {len(comp)} bytes, {rep.matches} matches")


def test_no_match_across_blocks(gpu_lib, ctx):
    rng = np.random.default_rng(3)
    R = random_bytes(rng, 100)
    data = random_bytes(rng, B - 100, 16) + R + R + random_bytes(rng, 3000, 16)
    comp, blocks, _ = check(gpu_lib, ctx, data)
    second = comp[blocks[1].offset:blocks[1].offset + blocks[1].size]
    assert zlib.decompress(second[18:-8], -15) == data[B:]  # alone, with no history


def de_bruijn(k: int, n: int):
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return seq


def test_code_shapes(gpu_lib, ctx):
    rng = np.random.default_rng(4)
    check(gpu_lib, ctx, b"aaaaa")                                     # one value: two literal/length codes with the end of block
    check(gpu_lib, ctx, random_bytes(rng, 1000, 2))
    # all 256 values equally often, twice: the second half is matches, so the block is dynamic with 256 literals of 8 bits
    perm = np.tile(np.arange(256, dtype=np.uint8), 64)
    rng.shuffle(perm)
    _, blocks, _ = check(gpu_lib, ctx, perm.tobytes() * 2)
    assert blocks[0].btype == 2
    # Fibonacci counts over 22 values, 46367 bytes: the unlimited Huffman tree is 21 deep, the codes have to be limited to 15
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    v = np.repeat(np.arange(22, dtype=np.uint8) + 65, fib)
    assert len(v) == 46367
    rng.shuffle(v)
    _, blocks, _ = check(gpu_lib, ctx, v.tobytes())
    assert blocks[0].btype == 2
    # no match anywhere: every window of four is met once (a de Bruijn sequence over 16 values)
    seq = bytes(97 + x for x in de_bruijn(16, 4)[:20000])
    _, blocks, rep = check(gpu_lib, ctx, seq)
    assert blocks[0].btype == 2 and rep.matches == 0 and rep.tokens == len(seq)
    # only matches behind the first literal
    _, _, rep = check(gpu_lib, ctx, b"\x00" * (1 + 3 * 258))
    assert (rep.tokens, rep.matches) == (4, 3)


def test_stored_fallback(gpu_lib, ctx):
    rng = np.random.default_rng(5)
    _, blocks, rep = check(gpu_lib, ctx, random_bytes(rng, B) + text(rng, B))
    assert blocks[0].btype == 0 and blocks[0].size <= 65311 and blocks[0].size == B + 31
    assert blocks[1].btype == 2 and rep.stored_blocks == 1


def mixed(rng, n_blocks: int) -> bytes:
    parts = []
    for k in range(n_blocks):
        kind = int(rng.integers(0, 4))
        n = B if k < n_blocks - 1 else int(rng.integers(1, B + 1))
        if kind == 0:
            parts.append(text(rng, n))
        elif kind == 1:
            parts.append(random_bytes(rng, n))
        elif kind == 2:
            parts.append(random_bytes(rng, n, 4))
        else:
            parts.append((b"J" * 150 + b"\n+\n" + random_bytes(rng, 150, 4)) * (n // 303 + 1))
            parts[-1] = parts[-1][:n]
    return b"".join(parts)


@pytest.fixture(scope="module")
def many(gpu_lib, ctx):
    data = mixed(np.random.default_rng(6), 257)
    return data, check(gpu_lib, ctx, data)[0]


@pytest.mark.parametrize("n_blocks", [3, 64, 65, 257])
def test_many_blocks_and_every_grid(gpu_lib, ctx, many, n_blocks):
    """The blocks are independent and the bytes do not depend on the grid: the first n blocks alone are a prefix of all 257."""
    data, comp_all = many
    comp, blocks, _ = check(gpu_lib, ctx, data[:n_blocks * B])
    assert len(blocks) == n_blocks
    assert comp[:-28] == comp_all[:len(comp) - 28]


def test_out_cap_too_small(gpu_lib, ctx):
    rng = np.random.default_rng(7)
    data = text(rng, 100_000)
    comp, _ = deflate(gpu_lib, ctx, data)
    for cap in (0, 27, len(comp) - 1):
        out = np.full(len(comp) + 64, 0xA5, np.uint8)
        n = C.c_uint64(0)
        rc = gpu_lib.ngsq_bgzf_deflate_device(ctx._ctx, data, len(data), out.ctypes.data, cap, C.byref(n), ffi.BGZF_EOF, None)
        assert rc == ffi.ERR_LIMIT and n.value == len(comp)
        assert (out[cap:] == 0xA5).all()
    out = np.full(len(comp) + 64, 0xA5, np.uint8)
    n = C.c_uint64(0)
    assert gpu_lib.ngsq_bgzf_deflate_device(ctx._ctx, data, len(data), out.ctypes.data, len(comp), C.byref(n), ffi.BGZF_EOF, None) == 0
    assert bytes(out[:len(comp)]) == comp and (out[len(comp):] == 0xA5).all()
    # no EOF flag: the same blocks without the last 28 bytes; nothing at all for no input
    assert deflate(gpu_lib, ctx, data, eof=False)[0] == comp[:-28]
    assert deflate(gpu_lib, ctx, b"", eof=False)[0] == b""


def test_deterministic(gpu_lib, ctx, ctx2):
    rng = np.random.default_rng(8)
    a, b = mixed(rng, 5), mixed(rng, 3)
    first = deflate(gpu_lib, ctx, a)[0]
    assert deflate(gpu_lib, ctx, a)[0] == first
    other = deflate(gpu_lib, ctx2, b)[0]          # another context, another stream, between two calls of the first
    assert deflate(gpu_lib, ctx, a)[0] == first
    assert deflate(gpu_lib, ctx2, a)[0] == first and deflate(gpu_lib, ctx, b)[0] == other
    assert host.bgzf_deflate(a, lib=gpu_lib)[0] == first


def test_floor_on_generator_text(gpu_lib, ctx, tmp_path):
    """200 pairs of k_gen_write's FASTQ text: the device output has to beat zlib's Huffman-only coding of the same blocks.  Margin
    zero: 43 % of the text is a run of J, so matches and dynamic codes together beat codes alone widely; an encoder that stores
    everything or writes literals only does not pass.  The ratios to zlib's levels 1 and 6 are printed."""
    rng = np.random.default_rng(9)
    fa = str(tmp_path / "f.fa")
    open(fa, "wb").write(gm.fasta_text([(b"chr1", gm.random_letters(rng, 100_000))], 60))
    p1, p2 = str(tmp_path / "f_1.fastq"), str(tmp_path / "f_2.fastq")
    host.generate([(fa, 1000, 200.0, 30.0, 150, 1)], p1, p2, 11, 200, lib=gpu_lib)
    data = open(p1, "rb").read()
    assert data.count(b"\n") == 800
    comp, blocks, rep = check(gpu_lib, ctx, data)
    mine = len(comp) - 28
    huff = bm.zlib_size(data, 6, zlib.Z_HUFFMAN_ONLY)
    l1, l6 = bm.zlib_size(data, 1), bm.zlib_size(data, 6)
    print(f"generator text {len(data)} bytes: device {mine}, Huffman only {huff}, zlib -1 {l1} (device/zlib {mine / l1:.3f}), "
          f"zlib -6 {l6} ({mine / l6:.3f}); {rep.tokens} tokens, {rep.matches} matches")
    assert mine < huff
