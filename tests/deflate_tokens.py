"""A raw DEFLATE stream (RFC 1951) taken apart into its tokens, in plain Python: what the tests of the encoder's match search
look at.  tokens(raw) -> (data, tokens); a token is an int (a literal's byte) or a Match (length, distance, the position of its
first byte in the inflated data).  Stored, fixed and dynamic blocks are read; every error of the stream is a ValueError."""
from __future__ import annotations

from typing import List, NamedTuple, Tuple, Union


class Match(NamedTuple):
    length: int
    distance: int
    start: int


Token = Union[int, Match]

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class _Bits:
    def __init__(self, raw: bytes):
        self.raw, self.at = raw, 0  # at: in bits

    def take(self, n: int) -> int:
        v = 0
        for k in range(n):
            byte = self.at >> 3
            if byte >= len(self.raw):
                raise ValueError("the stream ends inside a block")
            v |= ((self.raw[byte] >> (self.at & 7)) & 1) << k
            self.at += 1
        return v


def _decoder(lengths: List[int]):
    """Canonical Huffman codes of the lengths (RFC 1951 3.2.2) as {(length, code): symbol}."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for s, l in enumerate(lengths):
        if l:
            table[(l, nxt[l])] = s
            nxt[l] += 1
    return table


def _symbol(bits: _Bits, table) -> int:
    code = 0
    for l in range(1, 16):
        code = code << 1 | bits.take(1)  # Huffman codes come most significant bit first
        s = table.get((l, code))
        if s is not None:
            return s
    raise ValueError("a code of no symbol")


def tokens(raw: bytes) -> Tuple[bytes, List[Token]]:
    bits, out, toks = _Bits(raw), bytearray(), []
    while True:
        final, btype = bits.take(1), bits.take(2)
        if btype == 0:
            bits.at = (bits.at + 7) & ~7
            n, nn = bits.take(16), bits.take(16)
            if n ^ nn != 0xFFFF:
                raise ValueError("stored block: LEN and NLEN disagree")
            at = bits.at >> 3
            if at + n > len(raw):
                raise ValueError("the stream ends inside a stored block")
            out += raw[at:at + n]
            toks.extend(raw[at:at + n])
            bits.at += 8 * n
        elif btype == 3:
            raise ValueError("block type 3")
        else:
            if btype == 1:
                ll = _decoder([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
                dd = _decoder([5] * 30)
            else:
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                cl = [0] * 19
                for k in range(hclen):
                    cl[CL_ORDER[k]] = bits.take(3)
                cld, lengths = _decoder(cl), []
                while len(lengths) < hlit + hdist:
                    s = _symbol(bits, cld)
                    if s < 16:
                        lengths.append(s)
                    elif s == 16:
                        if not lengths:
                            raise ValueError("a repeat with nothing before it")
                        lengths += [lengths[-1]] * (3 + bits.take(2))
                    elif s == 17:
                        lengths += [0] * (3 + bits.take(3))
                    else:
                        lengths += [0] * (11 + bits.take(7))
                if len(lengths) != hlit + hdist:
                    raise ValueError("a repeat runs past the code lengths")
                ll, dd = _decoder(lengths[:hlit]), _decoder(lengths[hlit:])
            while True:
                s = _symbol(bits, ll)
                if s < 256:
                    out.append(s)
                    toks.append(s)
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise ValueError("length symbol %d" % s)
                    length = LEN_BASE[s - 257] + bits.take(LEN_EXTRA[s - 257])
                    d = _symbol(bits, dd)
                    if d > 29:
                        raise ValueError("distance symbol %d" % d)
                    distance = DIST_BASE[d] + bits.take(DIST_EXTRA[d])
                    if distance > len(out):
                        raise ValueError("invalid distance too far back")
                    toks.append(Match(length, distance, len(out)))
                    for _ in range(length):
                        out.append(out[-distance])
        if final:
            return bytes(out), toks


def matches(toks: List[Token]) -> List[Match]:
    return [t for t in toks if isinstance(t, Match)]


def member_tokens(stream: bytes, block) -> Tuple[bytes, List[Token]]:
    """The tokens of one BGZF member (a tests.bgzf_model.Block of `stream`)."""
    return tokens(stream[block.offset + 18:block.offset + block.size - 8])
