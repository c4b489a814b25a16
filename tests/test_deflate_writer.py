"""tests/deflate_writer.py against zlib's inflate, on the CPU: every stream tests/test_inflate_streams_gpu.py feeds the device
decoder is accepted here first (consumed exactly, output == expand(symbols)), every malformed one refused; and the case lists
hold what their names say (the code shapes, the header forms, the second-level table sizes)."""
import random
import zlib

import pytest

from tests import deflate_writer as dw
from tests.deflate_writer import (DIST_EXTRA, LEN_EXTRA, SWEEP_SEEDS, DeflateWriter, complete_lengths, expand, header_runs, kraft,
                                  malformed_cases, sub_need, sub_tables, sweep_cases, valid_cases)

MAX_PAYLOAD = 65536 - 26   # what a BGZF member holds beside its header and trailer
SUB_BOUND = 308            # zlib's `enough 286 10 15` = 1332, less the 1024 first-level entries


def accepted(case):
    d = zlib.decompressobj(-15)
    out = d.decompress(case.raw)
    assert d.eof and not d.unused_data and not d.unconsumed_tail, case.name
    assert out == case.expect, case.name
    assert len(case.raw) <= MAX_PAYLOAD and len(case.expect) <= 65536, case.name
    for b in case.blocks:   # the bound the decoder's second-level storage rests on
        if kraft(b["ll"]) == 32768:
            assert sub_need(b["ll"]) <= SUB_BOUND, case.name


def by_name(name):
    return next(c for c in valid_cases() if c.name == name)


def test_writer_basics():
    # RFC 1951 3.2.2's example: lengths (3, 3, 3, 3, 3, 2, 4, 4) -> codes 010 011 100 101 110 00 1110 1111
    codes = dw.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4])
    msb_first = [format(c, "0%db" % l)[::-1] for c, l in codes]
    assert msb_first == ["010", "011", "100", "101", "110", "00", "1110", "1111"]
    # zlib's own fixed-block output, bit for bit
    co = zlib.compressobj(9, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
    ref = co.compress(b"deflate\xf0\x90") + co.flush()      # (nothing repeats: literals, 8- and 9-bit ones)
    assert DeflateWriter().fixed([("lit", b) for b in b"deflate\xf0\x90"], 1).getvalue() == ref
    assert zlib.decompress(DeflateWriter().fixed([("lit", 97), ("lit", 98), ("lit", 99), ("match", 9, 3)], 1).getvalue(), -15) == b"abc" * 4
    assert expand([("lit", 1), ("lit", 2), ("match", 5, 2), ("raw", 257, 0, 0, 0)]) == bytes([1, 2, 1, 2, 1, 2, 1, 1, 1, 1])
    with pytest.raises(ValueError):
        expand([("lit", 1), ("match", 3, 2)])
    assert dw.length_symbol(258) == (285, 0) and dw.length_symbol(258, 284) == (284, 31) and dw.dist_symbol(32768) == (29, 8191)
    assert dw.rle_header([0] * 138 + [7] * 8 + [0] * 3 + [2, 2]) == [(18, 127), (7, 0), (16, 3), (7, 0), (17, 0), (2, 0), (2, 0)]


def test_complete_lengths_and_sub_need():
    rng = random.Random(1)
    for n, max_len in ((286, 15), (286, 9), (30, 15), (30, 5), (19, 7), (2, 1), (16, 15), (257, 11)):
        for _ in range(20):
            lens = complete_lengths(rng, n, max_len)
            assert len(lens) == n and kraft(lens) == 32768 and max(lens) == max_len and min(lens) >= 1
    lens = complete_lengths(rng, 286, 15, used=40, longest_first=[256, 7])
    assert kraft(lens) == 32768 and lens[256] == lens[7] == 15 and 40 <= sum(1 for l in lens if l) <= 42
    assert max(complete_lengths(rng, 30, 15, used=[0, 1, 2])) == 2   # three codes cannot reach further
    # sub_need by hand: sixteen 14-bit codes fill one 10-bit prefix, two 11-bit codes another
    lens = [1, 2, 3, 4, 5, 6, 7, 8, 9] + [11] * 2 + [14] * 16
    assert kraft(lens) == 32768 and sub_need(lens) == 2 + 16 and sorted(sub_tables(lens).values()) == [11, 14]
    assert sub_need(dw.GEN_LL) == 0 and sub_need(dw.FIXED_LITLEN) == 0
    for _ in range(300):
        assert sub_need(complete_lengths(rng, 286, 15, used=rng.randrange(16, 287))) <= SUB_BOUND


def test_valid_cases_are_accepted_by_zlib():
    cases = valid_cases()
    assert {c.group for c in cases} == set("abcdef")
    for c in cases:
        accepted(c)


def test_valid_cases_hold_what_they_say():
    for L in (10, 11, 15):
        assert max(by_name(f"litlen_longest_{L}").blocks[0]["ll"]) == L
    assert {l - 10 for l in sub_tables(by_name("sub_tables_1_to_5_bits").blocks[0]["ll"]).values()} == {1, 2, 3, 4, 5}
    ll = by_name("sub_need_largest_eob_15_bits").blocks[0]["ll"]
    assert sub_need(ll) == 288 and ll[256] == 15 and kraft(ll) == 32768
    for L in (8, 9, 15):
        dl = by_name(f"dist_longest_{L}").blocks[0]["dl"]
        assert max(dl) == L and len(dl) == 30 and min(dl) >= 1
    assert by_name("one_distance_code_0").blocks[0]["dl"] == (1,)
    assert by_name("one_distance_code_29").blocks[1]["dl"] == (0,) * 29 + (1,)
    b = by_name("plain_header_over_2048_bits_cl_7_bits").blocks[0]
    assert b["header_bits"] > 2048 and b["hclen"] == 19 and len(b["ll"]) == 286 and len(b["dl"]) == 30
    b = by_name("no_distance_code_hlit_257_hdist_1").blocks[0]
    assert len(b["ll"]) == 257 and b["dl"] == (0,)
    assert by_name("hclen_5").blocks[0]["hclen"] == 5
    b = by_name("rle_across_the_boundary").blocks[0]
    assert any(sym == 16 and at < 286 < at + n for at, sym, n in header_runs(b["items"]))
    b = by_name("rle_repeats_3_6_10_11_138").blocks[0]
    assert {(16, 3), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138)} <= {(sym, n) for _, sym, n in header_runs(b["items"])}
    # the widest symbol the decoder's windows step over: 15 + 5 + 8 + 13 bits
    for ls, ds in ((281, 28), (282, 29)):
        assert dw.WIDE_LL[ls] + LEN_EXTRA[ls - 257] + dw.WIDE_DL[ds] + DIST_EXTRA[ds] == 41
    assert dw.WIDE_LL[65] == 1 and len(by_name("widest_symbol_at_bit_0_to_128").blocks) == 130
    assert all(l > 8 for l in dw.LONG_DL[8:16]) and kraft(dw.LONG_DL) == 32768
    assert len(by_name("stored_len_largest_in_a_member").raw) == MAX_PAYLOAD
    assert len(by_name("last_match_ends_at_65536").expect) == 65536
    assert by_name("eob_only_dynamic_block_final").expect == b""
    assert sorted(c.in_mis for c in valid_cases() if c.in_mis is not None) == [0, 1, 2, 3]


def test_malformed_cases_are_refused_by_zlib():
    for m in malformed_cases():
        with pytest.raises(zlib.error):
            zlib.decompress(m.raw, -15)
        assert m.isize <= 1024 or m.name == "distance_3001_at_position_3000", m.name
        assert len(m.tail) <= 4
    # the cut stream is a whole, valid one with the byte that was cut off
    m = next(m for m in malformed_cases() if m.name == "huffman_block_cut_mid_symbol")
    assert len(zlib.decompress(m.raw + m.tail, -15)) == m.isize


@pytest.mark.parametrize("seed", SWEEP_SEEDS)
def test_sweep_is_accepted_by_zlib(seed):
    cases = sweep_cases(seed)
    assert 36 <= len(cases) <= 44 and sum(len(c.expect) > 4096 for c in cases) == 2
    for c in cases:
        assert 1 <= len(c.expect) <= 65536
        accepted(c)
