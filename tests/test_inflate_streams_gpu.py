"""The device inflate (`k_bgzf_inflate`) on DEFLATE streams zlib's writer never produces: the case lists of tests/deflate_writer.py
(distances up to 32 768 and at the edges of the decoder's 2 KiB ring, every length code both ways, code shapes from 1-bit to
15-bit with second-level tables of every size, headers of every form, block structure inside a member, fixed blocks, a random
sweep) against expand(symbols), CRC check on; and malformed streams, which must be refused with their block's number.
tests/test_deflate_writer.py has put every one of these streams through zlib's inflate on the CPU."""
import re

import pytest

from tests.deflate_writer import SWEEP_SEEDS, DeflateWriter, malformed_cases, sweep_cases, valid_cases
from tests.test_device_ingest_gpu import bgzf_block, ctx, device_inflate  # noqa: F401  (ctx: the module-scoped context fixture)

pytestmark = pytest.mark.gpu


def stored_member(data: bytes) -> bytes:
    return bgzf_block(data, raw=DeflateWriter().stored(data, 1).getvalue())


def members_of(cases):
    """One buffer of BGZF members, one per case; a case that wants its payload at a given offset mod 4 gets a stored member of
    suitable size in front.  Returns (buffer, [(case name, first output byte, expected bytes)])."""
    buf, want, out_at = bytearray(), [], 0
    for c in cases:
        if c.in_mis is not None:
            pad = bytes((7 * i + 1) & 255 for i in range(4 + (c.in_mis - len(buf) - 31 - 18) % 4))   # (a stored member is 31 + n bytes)
            buf += stored_member(pad)
            want.append((c.name + " (pad)", out_at, pad))
            out_at += len(pad)
            assert (len(buf) + 18) % 4 == c.in_mis
        buf += bgzf_block(c.expect, raw=c.raw)
        want.append((c.name, out_at, c.expect))
        out_at += len(c.expect)
    return bytes(buf), want


def check_members(lib, ctx, cases):
    """Decode the cases' members in one call, CRC check on, and compare member by member; a failure names the case (an error of
    the decoder by its block number; after a CRC mismatch the buffer is decoded again without the check to say which byte)."""
    buf, want = members_of(cases)
    refused = None
    try:
        got = device_inflate(lib, ctx, buf)
    except RuntimeError as e:
        block = re.search(r"block (\d+): ", str(e))
        refused = f"{want[int(block.group(1))][0] if block else '?'}: {e}"
        if "CRC mismatch" not in str(e):
            pytest.fail(refused)
        got = device_inflate(lib, ctx, buf, check_crc=False)
    assert len(got) == sum(len(e) for _, _, e in want)
    for name, at, expect in want:
        piece = got[at:at + len(expect)]
        if piece != expect:
            first = next(i for i, (x, y) in enumerate(zip(piece, expect)) if x != y)
            pytest.fail(f"{name}: byte {first} of {len(expect)} is {piece[first]}, expected {expect[first]}")
    assert refused is None, refused


@pytest.mark.parametrize("group", "abcdef")
def test_valid_streams(gpu_lib, ctx, group):
    """(a) distances, (b) lengths, (c) code shapes, (d) windows and batches, (e) block structure, (f) fixed blocks: one buffer
    per group, every member of it one case."""
    cases = [c for c in valid_cases() if c.group == group]
    assert cases
    check_members(gpu_lib, ctx, cases)


@pytest.mark.parametrize("seed", SWEEP_SEEDS)
def test_random_sweep(gpu_lib, ctx, seed):
    """(h) about 40 members of 1..4 deflate blocks of random type, random complete code sets, random header style."""
    check_members(gpu_lib, ctx, sweep_cases(seed))


def test_malformed_streams(gpu_lib, ctx):
    """(g) each malformed member in a buffer of its own, as block 1: a valid member in front, more than 64 KiB of valid
    (stored) members behind it, so that no read of the decoder leaves the buffers whatever it makes of the stream.  The error
    names the block; where only one status is right its wording is checked too.  After each case the context still decodes.
    (`distance_3001_at_position_3000` announces ISIZE 3 003, all others at most 1 024: the decoder refuses output beyond
    ISIZE before it looks at a batch's distances.)"""
    front = next(c for c in valid_cases() if c.name == "len258_both_ways")
    good, want = members_of([front, next(c for c in valid_cases() if c.name == "half_own_at100")])
    behind = b"".join(stored_member(bytes((i * k + 3) & 255 for i in range(34_000))) for k in (5, 11))
    assert len(behind) > 65536
    for m in malformed_cases():
        bad = bytearray(bgzf_block(bytes(m.isize), raw=m.raw))
        bad[len(bad) - 8:len(bad) - 8 + len(m.tail)] = m.tail
        buf = bgzf_block(front.expect, raw=front.raw) + bytes(bad) + behind
        try:
            device_inflate(gpu_lib, ctx, buf)
        except RuntimeError as e:
            print(f"{m.name}: {e}")
            assert "block 1: " + (m.text or "") in str(e) and "block 1: ok" not in str(e), f"{m.name}: {e}"
        else:
            pytest.fail(f"{m.name}: accepted")
        got = device_inflate(gpu_lib, ctx, good)
        assert got == b"".join(e for _, _, e in want), f"after {m.name}"
