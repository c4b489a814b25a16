"""A plain-Python DEFLATE (RFC 1951) *writer* under the test's control -- not a compressor.

zlib's `deflate` reaches only part of the format (no distance above 32 506, 258 always as code 285, at least two distance
codes, ...).  This module writes whatever RFC 1951 allows, and what it forbids, symbol by symbol:

  symbols   ("lit", byte)
            ("match", length, distance[, length_code])     the length code may be chosen: 258 as 285, or as 284 plus 31
            ("raw", litlen_symbol, extra, dist_symbol or None, extra)    for malformed streams
  blocks    DeflateWriter.stored / .fixed / .dynamic; the dynamic header "plain" (every length sent as itself, HCLEN 19,
            the code-length code chosen by the caller), "rle" (16, 17 and 18 used greedily, running across the
            literal/length - distance boundary), or an explicit list of code-length symbols
  helpers   expand(symbols), complete_lengths(rng, n_symbols, max_len, ...), sub_need(litlen_lens)

and, at the end, the CASE LISTS of tests/test_inflate_streams_gpu.py: valid_cases(), malformed_cases(), sweep_cases(seed).
tests/test_deflate_writer.py runs every one of them through zlib's inflate on the CPU, so the GPU test only ever feeds the
device decoder streams the reference has accepted (or, the malformed ones, refused).  `rng` is a `random.Random`.
"""
from __future__ import annotations

import functools
import random
from collections import namedtuple

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_EXTRA = {16: 2, 17: 3, 18: 7}
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
# a code-length code that has every symbol: 13 / 16 + 6 / 32 = 1
DEFAULT_CL = [4, 5, 5, 5, 4, 4, 4, 4, 4, 4, 4, 4, 4, 5, 5, 5, 4, 4, 4]


class BitWriter:
    """Bits go out LSB first (RFC 1951 3.1.1); Huffman codes are packed starting with their most significant bit."""

    def __init__(self):
        self.acc = 0
        self.n = 0
        self.out = bytearray()

    @property
    def nbits(self) -> int:
        return len(self.out) * 8 + self.n

    def bits(self, value: int, n: int) -> None:
        assert 0 <= value < (1 << n), (value, n)
        self.acc |= value << self.n
        self.n += n
        if self.n >= 64:
            k = self.n // 8
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def align(self) -> None:
        self.bits(0, -self.nbits % 8)

    def raw_bytes(self, data: bytes) -> None:
        assert self.n % 8 == 0
        self.out += self.acc.to_bytes(self.n // 8, "little")
        self.acc = self.n = 0
        self.out += data

    def getvalue(self) -> bytes:
        return bytes(self.out) + self.acc.to_bytes((self.n + 7) // 8, "little")


def canonical_codes(lens):
    """RFC 1951 3.2.2: per symbol (code as it goes into the stream: bit-reversed, length), None without a code.
    An over-subscribed set still gets codes (cut to their length): malformed streams need a writer too."""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lens:
        if l == 0:
            out.append(None)
            continue
        c = nxt[l] & ((1 << l) - 1)
        nxt[l] += 1
        out.append((int(format(c, "0%db" % l)[::-1], 2), l))
    return out


def kraft(lens) -> int:
    """Sum of 2^-l over the codes, in units of 2^-15: 32768 for a complete set."""
    return sum(1 << (15 - l) for l in lens if l)


def length_symbol(length: int, prefer: int | None = None):
    """(symbol, extra bits' value) of a match length; `prefer` picks the code where two can say it (258: 285, or 284 + 31)."""
    if prefer is None:
        prefer = 285 if length == 258 else max(s for s in range(257, 285) if LEN_BASE[s - 257] <= length)
    base, ex = LEN_BASE[prefer - 257], LEN_EXTRA[prefer - 257]
    assert base <= length < base + (1 << ex), (length, prefer)
    return prefer, length - base


def dist_symbol(distance: int):
    s = max(s for s in range(30) if DIST_BASE[s] <= distance)
    assert distance < DIST_BASE[s] + (1 << DIST_EXTRA[s])
    return s, distance - DIST_BASE[s]


def symbol_length(sym) -> int:
    """Output bytes of a VALID symbol."""
    if sym[0] == "lit":
        return 1
    if sym[0] == "match":
        return sym[1]
    _, ls, lex, ds, dex = sym
    if ls < 256:
        return 1
    if not (257 <= ls <= 285 and ds is not None and 0 <= ds < 30):
        raise ValueError(f"no output for {sym}")
    return LEN_BASE[ls - 257] + lex


def expand(symbols) -> bytes:
    """The bytes the symbols stand for, by the obvious byte-by-byte copy."""
    out = bytearray()
    for sym in symbols:
        if sym[0] == "lit":
            out.append(sym[1])
            continue
        if sym[0] == "match":
            length, distance = sym[1], sym[2]
        else:
            _, ls, lex, ds, dex = sym
            if ls < 256:
                out.append(ls)
                continue
            length = symbol_length(sym)
            distance = DIST_BASE[ds] + dex
        if not 1 <= distance <= len(out):
            raise ValueError(f"distance {distance} at position {len(out)}")
        for _ in range(length):
            out.append(out[-distance])
    return bytes(out)


def rle_header(seq):
    """Code-length symbols for the lengths `seq`, 16 / 17 / 18 used greedily (the caller passes the literal/length and distance
    lengths as ONE sequence: a run goes across the boundary, as RFC 1951 3.2.7 allows)."""
    items, i, n = [], 0, len(seq)
    while i < n:
        v, run = seq[i], 1
        while i + run < n and seq[i + run] == v:
            run += 1
        if v == 0 and run >= 3:
            r = min(run, 138)
            items.append((18, r - 11) if r >= 11 else (17, r - 3))
            i += r
            continue
        items.append((v, 0))
        i += 1
        run -= 1
        while v and run >= 3:
            r = min(run, 6)
            items.append((16, r - 3))
            i += r
            run -= r
    return items


def header_runs(items):
    """(first index, code-length symbol, count) of every item of a dynamic header: which lengths a repeat covers."""
    out, i = [], 0
    for sym, extra in items:
        n = 1 if sym < 16 else (3 if sym < 18 else 11) + extra
        out.append((i, sym, n))
        i += n
    return out


class DeflateWriter:
    """One raw DEFLATE stream, block by block.  `symbols` collects what the blocks stand for (stored bytes as literals), so
    expand(w.symbols) is the stream's output; `blocks` notes what each dynamic block was made of: its two sets of lengths, the
    header's code-length symbols, HCLEN and the header's size in bits."""

    def __init__(self):
        self.w = BitWriter()
        self.symbols = []
        self.blocks = []

    def getvalue(self) -> bytes:
        return self.w.getvalue()

    def stored(self, data: bytes, last, len_: int | None = None, nlen: int | None = None):
        w = self.w
        w.bits(int(last), 1)
        w.bits(0, 2)
        w.align()
        n = len(data) if len_ is None else len_
        w.bits(n, 16)
        w.bits((n ^ 0xFFFF) if nlen is None else nlen, 16)
        w.raw_bytes(bytes(data))
        self.symbols += [("lit", b) for b in data]
        return self

    def _symbols(self, lcodes, dcodes, symbols, eob: bool):
        w = self.w

        def code(table, s):
            assert table[s] is not None, f"symbol {s} has no code"
            w.bits(*table[s])

        for sym in symbols:
            if sym[0] == "lit":
                code(lcodes, sym[1])
                continue
            if sym[0] == "match":
                ls, lex = length_symbol(sym[1], sym[3] if len(sym) > 3 else None)
                ds, dex = dist_symbol(sym[2])
            else:
                _, ls, lex, ds, dex = sym
            code(lcodes, ls)
            if 257 <= ls <= 285:
                w.bits(lex, LEN_EXTRA[ls - 257])
            if ls >= 257 and ds is not None:
                code(dcodes, ds)
                w.bits(dex, DIST_EXTRA[ds] if ds < 30 else 0)
        if eob:
            code(lcodes, 256)
        self.symbols += list(symbols)

    def fixed(self, symbols, last, eob: bool = True):
        self.w.bits(int(last), 1)
        self.w.bits(1, 2)
        self._symbols(canonical_codes(FIXED_LITLEN), canonical_codes(FIXED_DIST), symbols, eob)
        return self

    def dynamic(self, litlen_lens, dist_lens, symbols, last, header="rle", cl_lens=None, hclen: int | None = None, eob: bool = True):
        w = self.w
        seq = list(litlen_lens) + list(dist_lens)
        if header == "plain":
            items = [(v, 0) for v in seq]
            hclen = 19 if hclen is None else hclen
        elif header == "rle":
            items = rle_header(seq)
        else:
            items = [(x, 0) if isinstance(x, int) else tuple(x) for x in header]
        cl_lens = list(DEFAULT_CL if cl_lens is None else cl_lens)
        if hclen is None:
            hclen = max([4] + [k + 1 for k, s in enumerate(CL_ORDER) if cl_lens[s]])
        bit0 = w.nbits
        w.bits(int(last), 1)
        w.bits(2, 2)
        w.bits(len(litlen_lens) - 257, 5)
        w.bits(len(dist_lens) - 1, 5)
        w.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            w.bits(cl_lens[s], 3)
        sent = [cl_lens[s] if s in CL_ORDER[:hclen] else 0 for s in range(19)]
        ccodes = canonical_codes(sent)
        for sym, extra in items:
            assert ccodes[sym] is not None, f"code-length symbol {sym} has no code"
            w.bits(*ccodes[sym])
            if sym >= 16:
                w.bits(extra, CL_EXTRA[sym])
        self.blocks.append(dict(ll=tuple(litlen_lens), dl=tuple(dist_lens), items=tuple(items), hclen=hclen, header_bits=w.nbits - bit0))
        self._symbols(canonical_codes(litlen_lens), canonical_codes(dist_lens), symbols, eob)
        return self


def complete_lengths(rng, n_symbols: int, max_len: int, used=None, longest_first=()):
    """Code lengths of a COMPLETE prefix code (Kraft sum exactly 1) whose longest code has `max_len` bits (less, if fewer than
    max_len + 1 symbols get a code), drawn at random: a chain 1, 2, ..., max_len, max_len whose leaves are split at random.
    used: how many of the n_symbols get a code, or which (default all); longest_first: symbols that take the longest codes."""
    if used is None:
        idx = list(range(n_symbols))
    elif isinstance(used, int):
        idx = sorted(set(rng.sample(range(n_symbols), used)) | set(longest_first))
    else:
        idx = sorted(set(used) | set(longest_first))
    k = len(idx)
    assert k >= 2, "a complete code has at least two codes"
    max_len = min(max_len, k - 1)
    assert k <= 1 << max_len, (k, max_len)
    cnt = [0] * (max_len + 2)
    for l in range(1, max_len):
        cnt[l] = 1
    cnt[max_len] = 2
    leaves = max_len + 1
    while leaves < k:
        r = rng.randrange(sum(cnt[1:max_len]))
        l = 1
        while r >= cnt[l]:
            r -= cnt[l]
            l += 1
        cnt[l] -= 1
        cnt[l + 1] += 2
        leaves += 1
    pool = [l for l in range(max_len, 0, -1) for _ in range(cnt[l])]   # longest first
    first = list(longest_first)
    rest = [s for s in idx if s not in set(longest_first)]
    tail = pool[len(first):]
    rng.shuffle(tail)
    lens = [0] * n_symbols
    for s, l in zip(first + rest, pool[:len(first)] + tail):
        lens[s] = l
    assert kraft(lens) == 32768
    return lens


def sub_tables(litlen_lens, first_level: int = 10):
    """{first_level-bit prefix (the code's first bits, MSB first): longest code behind it} for the codes longer than first_level."""
    out = {}
    for c in canonical_codes(litlen_lens):
        if c is not None and c[1] > first_level:
            rev, l = c
            msb_first = int(format(rev, "0%db" % l)[::-1], 2)
            p = msb_first >> (l - first_level)
            out[p] = max(out.get(p, 0), l)
    return out


def sub_need(litlen_lens, first_level: int = 10) -> int:
    """Second-level table entries a decoder with a 10-bit first level needs for this set: the sum of 2^(longest - 10) over
    the 10-bit prefixes that own codes longer than 10 bits."""
    return sum(1 << (l - first_level) for l in sub_tables(litlen_lens, first_level).values())


# ---------------------------------------------------------------------------------------------------------------------------
# Symbol lists with a running output position
# ---------------------------------------------------------------------------------------------------------------------------
GEN_LL = [8] * 226 + [9] * 60      # every literal/length symbol has a code: 226 / 256 + 60 / 512 = 1
GEN_DL = [4] * 2 + [5] * 28        # every distance symbol: 2 / 16 + 28 / 32 = 1
# distances at which the decoder changes path: lane width, the 2 KiB LDS ring, the last distance code, what zlib never writes
DIST_EDGES = [1, 63, 64, 65, 2047, 2048, 2049, 24577, 32506, 32507, 32767, 32768]


class Syms:
    """A symbol list that knows how many bytes it stands for; restricted to the symbols that have a code in (ll, dl)."""

    def __init__(self, rng, start: int = 0, ll=GEN_LL, dl=GEN_DL):
        self.rng, self.pos, self.s = rng, start, []
        self.lits = [b for b in range(min(256, len(ll))) if ll[b]]
        self.lsyms = [s for s in range(257, min(286, len(ll))) if ll[s]]
        self.dsyms = [s for s in range(min(30, len(dl))) if dl[s]]

    def lit(self, b=None):
        self.s.append(("lit", self.rng.choice(self.lits) if b is None else b))
        self.pos += 1
        return self

    def nlits(self, n):
        for _ in range(n):
            self.lit()
        return self

    def match(self, length, distance, lsym=None):
        assert 1 <= distance <= self.pos and 3 <= length <= 258, (length, distance, self.pos)
        self.s.append(("match", length, distance) if lsym is None else ("match", length, distance, lsym))
        self.pos += length
        return self

    def random_match(self, room, edges=(), far=300):
        """A match of at most `room` bytes from the codes at hand; False if there is none."""
        rng = self.rng
        ls = [s for s in self.lsyms if LEN_BASE[s - 257] <= room]
        ds = [s for s in self.dsyms if DIST_BASE[s] <= self.pos]
        if not ls or not ds:
            return False
        lsym = rng.choice(ls)
        length = min(room, LEN_BASE[lsym - 257] + rng.randrange(1 << LEN_EXTRA[lsym - 257]))
        length = max(length, LEN_BASE[lsym - 257])
        cand = [d for d in edges if d <= self.pos and dist_symbol(d)[0] in ds]
        if cand and rng.random() < 0.5:
            distance = rng.choice(cand)
        else:
            near = [s for s in ds if DIST_BASE[s] <= far] or ds
            dsym = rng.choice(near)
            distance = min(self.pos, DIST_BASE[dsym] + rng.randrange(1 << DIST_EXTRA[dsym]))
        self.match(length, distance, lsym)
        return True

    def fill(self, upto, p_lit=0.3, edges=(), far=300):
        """Random literals and matches until the output stands at exactly `upto`."""
        rng = self.rng
        while self.pos < upto:
            room = upto - self.pos
            if self.lits and (self.pos < 40 or room < 3 or rng.random() < p_lit):
                self.lit()
            elif not self.random_match(room, edges, far):
                assert self.lits, "neither a literal nor a match fits"
                self.lit()
        return self


Case = namedtuple("Case", "group name raw expect blocks in_mis", defaults=(None,))
Malformed = namedtuple("Malformed", "name raw isize text tail", defaults=(None, b""))


def _case(group, name, dw, in_mis=None):
    return Case(group, name, dw.getvalue(), expand(dw.symbols), tuple(dw.blocks), in_mis)


# ---------------------------------------------------------------------------------------------------------------------------
# (a) distances
# ---------------------------------------------------------------------------------------------------------------------------
def _group_a():
    rng = random.Random(101)
    out = []

    def one(name, build):
        s = Syms(rng)
        build(s)
        out.append(_case("a", name, DeflateWriter().dynamic(GEN_LL, GEN_DL, s.s, 1, header="rle")))

    for d in DIST_EDGES:
        # early: the match at the first position that allows it (distance == position, its source is byte 0: the bound of the
        # decoder's distance check).  late: 2 KiB + 512 and more of output further on -- the ring has wrapped, and pieces have left
        for when, p in (("early", d), ("late", d + 2560 + 37)):
            one(f"dist{d}_{when}", lambda s, d=d, p=p: s.fill(p).match(100, d).nlits(5).match(258, d).nlits(3))
    # a source that starts exactly at base - RING of the 64-byte emit chunk (base = 2560; RING = 2048), and one byte either
    # side; the match starting at the chunk's first byte and inside it
    for off in (0, 17):
        for delta in (-1, 0, 1):
            one(f"ring_edge_off{off}_{delta:+d}", lambda s, off=off, delta=delta: s.fill(2560 + off).match(100, 2048 + off + delta).nlits(2))
    for d in (5, 2100):
        one(f"straddle2_d{d}", lambda s, d=d: s.fill(2560 + 50).match(30, d).nlits(2))
        one(f"straddle3_d{d}", lambda s, d=d: s.fill(2560 + 50).match(100, d).nlits(2))
    for d in (1, 2, 3, 4, 5, 6, 63):   # pointer jumping: up to six rounds inside a 64-byte chunk
        one(f"jump_d{d}_len258", lambda s, d=d: s.fill(70).match(258, d).nlits(1))
        one(f"jump_d{d}_at_chunk_start", lambda s, d=d: s.fill(128).match(258, d).nlits(1))
    for at in (2560 + 10, 2560 + 50, 100):   # first half from the ring, second half from the match's own output
        one(f"half_own_at{at}", lambda s, at=at: s.fill(at).match(40, 20).nlits(1))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# (b) lengths
# ---------------------------------------------------------------------------------------------------------------------------
def _group_b():
    rng = random.Random(102)
    out = []
    for kind in ("fixed", "dynamic"):
        for ones in (0, 1):
            s = Syms(rng).nlits(70)
            for sym in range(257, 286):
                ex = LEN_EXTRA[sym - 257]
                s.match(LEN_BASE[sym - 257] + (((1 << ex) - 1) if ones else 0), rng.randrange(1, 70), sym)   # (284 + 31 = 258)
                s.lit()
            dw = DeflateWriter()
            dw.fixed(s.s, 1) if kind == "fixed" else dw.dynamic(GEN_LL, GEN_DL, s.s, 1)
            out.append(_case("b", f"every_length_code_{kind}_extra_{'ones' if ones else 'zero'}", dw))
    s = Syms(rng).nlits(10).match(258, 7, 285).match(258, 7, 284).lit().match(258, 300, 284).match(258, 300, 285)
    out.append(_case("b", "len258_both_ways", DeflateWriter().dynamic(GEN_LL, GEN_DL, s.s, 1)))
    s = Syms(rng).fill(65536 - 258, p_lit=0.1).match(258, 1000, 284)
    out.append(_case("b", "last_match_ends_at_65536", DeflateWriter().dynamic(GEN_LL, GEN_DL, s.s, 1)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# (c) code shapes
# ---------------------------------------------------------------------------------------------------------------------------
def sub_1to5_lengths(rng):
    """286 codes whose canonical order puts the 11-, 12-, 13-, 14- and 15-bit codes behind one 10-bit prefix each: second-level
    tables of 1, 2, 3, 4 and 5 index bits in one block.  (256 + 760 + 2 + 1 + 5) / 1024 = 1."""
    pool = [7] * 32 + [8] * 190 + [9] + [10] + [11] * 2 + [12] * 4 + [13] * 8 + [14] * 16 + [15] * 32
    rng.shuffle(pool)
    return pool


def sub_max_lengths(rng):
    """The largest second-level need a simple construction reaches: nine short codes, one prefix that holds 11, 12, 13, 14, 15, 15,
    and eight prefixes full of 15-bit codes: 9 x 32 = 288 entries for 271 codes.  End-of-block on a 15-bit code."""
    pool = [1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14] + [15] * 257   # (and one more 15 for the end of block)
    syms = rng.sample([s for s in range(286) if s != 256], 270)
    lens = [0] * 286
    for s, l in zip(syms, pool):
        lens[s] = l
    lens[256] = 15
    assert kraft(lens) == 32768
    return lens


def repeats_lengths():
    """Literal/length lengths whose greedy run-length header holds repeats of 138 and 11 (symbol 18), 10 and 3 (17), 6 and 3 (16)."""
    ll = [0] * 138 + [8] + [0] * 11 + [8] + [0] * 10 + [8] + [0] * 3 + [8] * 7 + [7] * 4 + [6] * 30 + [7] * 38 + [8] * 42
    assert len(ll) == 286 and kraft(ll) == 32768
    return ll


WIDE_LL = [0] * 283   # 'A' on one bit, end of block on 14, the length codes 281 and 282 (five extra bits) on 15
for _s, _l in zip([65] + list(range(66, 78)) + [256, 281, 282], list(range(1, 15)) + [15, 15]):
    WIDE_LL[_s] = _l
WIDE_DL = [1, 2, 3, 4, 5, 6, 7] + [0] * 21 + [8, 8]   # codes 28 and 29 (13 extra bits) on 8 bits: 15 + 5 + 8 + 13 = 41 bits
# distance codes 8..15 (distances 17..256) longer than the decoder's 8-bit distance table: every such match is resolved serially
LONG_DL = list(range(1, 15)) + [15, 15] + [0] * 14


def _group_c():
    rng = random.Random(103)
    out = []

    def filled(name, ll, dl, upto=3000, header="rle", far=300, **kw):
        s = Syms(rng, ll=ll, dl=dl).fill(upto, far=far)
        out.append(_case("c", name, DeflateWriter().dynamic(ll, dl, s.s, 1, header=header, **kw)))

    for L in (10, 11, 15):
        filled(f"litlen_longest_{L}", complete_lengths(rng, 286, L), GEN_DL)
    filled("sub_tables_1_to_5_bits", sub_1to5_lengths(rng), GEN_DL)
    filled("sub_need_largest_eob_15_bits", sub_max_lengths(rng), GEN_DL)
    # end of block on a 1-bit code, literals on 8; no distance code at all (HDIST 1 with length 0)
    dw = DeflateWriter()
    ll = [8] * 128 + [0] * 128 + [1]
    for k, n in enumerate((1, 70, 0, 200)):
        dw.dynamic(ll, [0], Syms(rng, ll=ll, dl=[0]).nlits(n).s, k == 3)
    out.append(_case("c", "eob_1_bit_no_distance_code", dw))
    filled("no_distance_code_hlit_257_hdist_1", [8] * 255 + [9, 9], [0], upto=700)
    for L in (8, 9, 15):   # all 30 codes in use; the small distances take the longest codes
        filled(f"dist_longest_{L}", GEN_LL, complete_lengths(rng, 30, L, longest_first=[4, 9, 0, 13, 16, 2, 19, 7]), upto=3500, far=4000)
    filled("one_distance_code_0", GEN_LL, [1], upto=600)
    dw = DeflateWriter()
    s = Syms(rng).fill(25000, p_lit=0.1)
    dw.dynamic(GEN_LL, GEN_DL, s.s, 0)
    dl = [0] * 29 + [1]
    s = Syms(rng, start=s.pos, dl=dl).match(258, 24577, 284).lit().match(9, 24580).fill(33100, far=40000).match(77, 32768).match(258, 32768)
    dw.dynamic(GEN_LL, dl, s.s, 1)
    out.append(_case("c", "one_distance_code_29", dw))
    # HLIT 286, HDIST 30, HCLEN 19 together, 7-bit code-length codes, and a header of more than 2 048 bits: the lengths 8 and 9
    # (286 of the 316) on 7-bit codes
    cl = [0] * 19
    for sym, l in ((0, 1), (1, 2), (2, 3), (3, 4), (5, 5), (4, 6), (8, 7), (9, 7)):
        cl[sym] = l
    filled("plain_header_over_2048_bits_cl_7_bits", GEN_LL, [4] * 2 + [5] * 28, header="plain", cl_lens=cl)
    assert 286 * 7 + 2 * 6 + 28 * 5 > 2048
    # HCLEN 5, the fewest a block with an end-of-block code can have (HCLEN 4 sends 16, 17, 18 and 0 only: no length but 0)
    cl = [0] * 19
    cl[16], cl[0], cl[8] = 2, 2, 1
    filled("hclen_5", [8] * 255 + [0, 8], [0], upto=500, cl_lens=cl)
    # a repeat (16) that copies a literal/length length into the distance lengths
    filled("rle_across_the_boundary", [8] * 150 + [9] * 102 + [10] * 28 + [5] * 6, [5] * 28 + [4] * 2)
    filled("rle_repeats_3_6_10_11_138", repeats_lengths(), [5] * 28 + [4] * 2)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# (d) windows and batches
# ---------------------------------------------------------------------------------------------------------------------------
def _group_d():
    rng = random.Random(104)
    out = []
    # the widest symbol the window phase steps over (15 + 5 + 8 + 13 bits) at every bit offset of a 128-bit window: a block
    # starts a window, k one-bit literals shift the match; k = 128: more one-bit symbols than a batch takes, then the match
    dw = DeflateWriter()
    s = Syms(rng).fill(24700, p_lit=0.1)
    dw.dynamic(GEN_LL, GEN_DL, s.s, 0)
    pos = s.pos
    for k in range(129):
        s = Syms(rng, start=pos, ll=WIDE_LL, dl=WIDE_DL)
        for _ in range(k):
            s.lit(65)
        if k & 1:
            s.match(162, 24576, 281)    # 131 + 31 on code 281, 16385 + 8191 on code 28: all extra bits one
        else:
            s.match(163, 24577, 282)    # all extra bits zero, code 29
        s.lit(66 + k % 12)
        dw.dynamic(WIDE_LL, WIDE_DL, s.s, k == 128)
        pos = s.pos
    out.append(_case("d", "widest_symbol_at_bit_0_to_128", dw))
    # exactly 63, 64 and 65 symbols between two chain stops (matches whose distance code is longer than the table)
    dw = DeflateWriter()
    s = Syms(rng, dl=LONG_DL).nlits(400)
    for n in (63, 64, 65, 64, 63):
        s.match(10, 200).nlits(n)
    s.match(10, 256)
    dw.dynamic(GEN_LL, LONG_DL, s.s, 1)
    out.append(_case("d", "63_64_65_symbols_between_stops", dw))
    # the same counted from a block start, the queue emptied by a stored block in front
    dw = DeflateWriter()
    pos = 0
    for k, n in enumerate((63, 64, 65)):
        dw.stored(bytes(rng.randrange(256) for _ in range(300)), 0)
        s = Syms(rng, start=pos + 300, dl=LONG_DL).nlits(n).match(20, 129 + k).nlits(n)
        dw.dynamic(GEN_LL, LONG_DL, s.s, k == 2)
        pos = s.pos
    out.append(_case("d", "63_64_65_symbols_from_a_block_start", dw))
    # long-distance-code matches back to back: every symbol takes the serial path
    s = Syms(rng, dl=LONG_DL).nlits(400)
    for _ in range(200):
        s.match(rng.randrange(3, 20), rng.randrange(17, 257))
    out.append(_case("d", "long_distance_codes_back_to_back", DeflateWriter().dynamic(GEN_LL, LONG_DL, s.s, 1)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# (e) block structure inside one member
# ---------------------------------------------------------------------------------------------------------------------------
EOB_ONLY = [0] * 256 + [1]


def _group_e():
    rng = random.Random(105)
    out = []

    def rbytes(n):
        return bytes(rng.randrange(256) for _ in range(n))

    dw = DeflateWriter()
    for k in range(300):
        dw.fixed([("lit", rng.randrange(256))], k == 299)
    out.append(_case("e", "300_fixed_blocks_of_one_literal", dw))
    dw = DeflateWriter()
    for k in range(300):
        ll = [0] * 257
        b = rng.randrange(256)
        ll[b] = ll[256] = 1
        dw.dynamic(ll, [0], [("lit", b)], k == 299, header="rle" if k & 1 else "plain")
    out.append(_case("e", "300_dynamic_blocks_of_one_literal", dw))
    dw = DeflateWriter()
    s = Syms(rng).nlits(30)
    dw.fixed(s.s, 0).fixed([], 0).dynamic(EOB_ONLY, [0], [], 0)
    s = Syms(rng, start=30).nlits(40).match(20, 65)
    dw.fixed(s.s, 0).dynamic(EOB_ONLY, [0], [], 0).fixed([], 0).stored(b"", 0)
    s = Syms(rng, start=s.pos).match(30, 90).fill(400)
    dw.dynamic(GEN_LL, GEN_DL, s.s, 0).dynamic(GEN_LL, GEN_DL, [], 1)
    out.append(_case("e", "empty_blocks_between_others", dw))
    out.append(_case("e", "eob_only_dynamic_block_final", DeflateWriter().dynamic(EOB_ONLY, [0], [], 1)))
    out.append(_case("e", "eob_only_dynamic_block_then_empty_stored", DeflateWriter().dynamic(EOB_ONLY, [0], [], 0).stored(b"", 1)))
    # a stored block's header at each of the eight bit phases, behind 1..63 queued bytes: a fixed block of q literals, j of them
    # 9-bit ones, ends 3 + 8 q + j + 7 bits behind a byte boundary
    for shift in range(8):
        dw = DeflateWriter()
        for q in range(1, 64):
            j = min(q, (q + shift) % 8)
            dw.fixed([("lit", rng.randrange(144, 256) if i < j else rng.randrange(144)) for i in range(q)], 0)
            dw.stored(rbytes(1 + (q * 7 + shift) % 40), q == 63)
        out.append(_case("e", f"stored_header_phases_shift{shift}", dw))
    dw = DeflateWriter()
    dw.stored(b"", 0).fixed([("lit", 1), ("lit", 2), ("lit", 3)], 0)
    for n in (1, 511, 512, 513):
        dw.stored(rbytes(n), 0)
    dw.stored(b"", 1)
    out.append(_case("e", "stored_len_0_1_511_512_513", dw))
    out.append(_case("e", "stored_len_largest_in_a_member", DeflateWriter().stored(rbytes(65536 - 26 - 5), 1)))
    dw = DeflateWriter().stored(rbytes(3000), 0)
    s = Syms(rng, start=3000).match(50, 5).match(100, 2900).match(258, 3150).lit().match(70, 2048).match(3, 3000)
    out.append(_case("e", "stored_then_matches_into_it", dw.fixed(s.s, 1)))
    for m in range(4):   # the payload at every in_off mod 4 (the test pads in front)
        s = Syms(rng).fill(1500)
        out.append(_case("e", f"payload_at_offset_{m}_mod_4", DeflateWriter().dynamic(GEN_LL, GEN_DL, s.s, 1), in_mis=m))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# (f) fixed blocks
# ---------------------------------------------------------------------------------------------------------------------------
def _group_f():
    rng = random.Random(106)
    out = []
    s = Syms(rng)
    for b in range(144, 256):
        s.lit(b)
    s.match(258, 1, 284).match(258, 1, 285).lit(7).match(3, 1).match(200, 112)
    out.append(_case("f", "nine_bit_literals_distance_code_0_and_284_plus_31", DeflateWriter().fixed(s.s, 1)))
    s = Syms(rng).fill(24577, p_lit=0.1).match(258, 24577, 284).fill(32768, far=40000).match(258, 32768, 284).match(3, 32507).match(4, 24577)
    out.append(_case("f", "distance_code_29", DeflateWriter().fixed(s.s, 1)))
    return out


@functools.lru_cache(maxsize=None)
def valid_cases():
    """Every hand-made valid stream: Case(group, name, raw DEFLATE, expected output, in_mis)."""
    cases = _group_a() + _group_b() + _group_c() + _group_d() + _group_e() + _group_f()
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


# ---------------------------------------------------------------------------------------------------------------------------
# (g) malformed streams
# ---------------------------------------------------------------------------------------------------------------------------
TEXT_INPUT_OVERRUN = "compressed data ends inside a symbol"   # inflate_status_text(INF_INPUT_OVERRUN)


@functools.lru_cache(maxsize=None)
def malformed_cases():
    """Malformed(name, raw, isize, text, tail): `raw` is the member's DEFLATE data, `isize` what its trailer announces, `text`
    the decoder's wording where one status is the only right one, `tail` bytes to put into the CRC field (a cut stream's continuation)."""
    rng = random.Random(107)
    out = []
    lits = [("lit", b) for b in b"malformed"]

    def dyn(name, *a, isize=9, **kw):
        out.append(Malformed(name, DeflateWriter().dynamic(*a, **kw).getvalue(), isize))

    dyn("oversubscribed_litlen", [8] * 257 + [9] * 29, GEN_DL, lits, 1, header="plain")
    dyn("oversubscribed_distance", GEN_LL, [1, 1, 1], lits, 1)
    dyn("oversubscribed_code_length_code", GEN_LL, GEN_DL, lits, 1, cl_lens=[3] * 19)
    # incomplete sets of more than one code: zlib refuses them; a decoder that builds its tables from them can still read these
    # symbols, and then it is the member's CRC (of ISIZE zero bytes) that refuses the member -- either is an error of block 1
    dyn("incomplete_litlen", GEN_LL[:285] + [0], GEN_DL, lits, 1)
    dyn("incomplete_distance", GEN_LL, [2, 2, 2], lits, 1)
    dyn("incomplete_code_length_code", GEN_LL, GEN_DL, lits, 1, cl_lens=DEFAULT_CL[:15] + [0] + DEFAULT_CL[16:])
    dyn("no_end_of_block_code", [8] * 256 + [0] + [9] * 0, GEN_DL, lits, 1, eob=False)
    dyn("symbol_16_first", GEN_LL, GEN_DL, lits, 1, header=[(16, 0)] + rle_header(GEN_LL[3:] + GEN_DL))
    dyn("repeat_past_hlit_plus_hdist", GEN_LL, GEN_DL, lits, 1, header=rle_header(GEN_LL + GEN_DL[:-3]) + [(16, 3)])
    dyn("hlit_287", GEN_LL + [0], GEN_DL, lits, 1)
    dyn("hlit_288", GEN_LL + [0, 0], GEN_DL, lits, 1)
    dyn("hdist_31", GEN_LL, GEN_DL + [0], lits, 1)
    dyn("hdist_32", GEN_LL, GEN_DL + [0, 0], lits, 1)
    # HCLEN 4 sends code lengths for 16, 17, 18 and 0 only: every length is 0, so there is no end-of-block code
    cl = [0] * 19
    cl[18], cl[0] = 1, 1
    dyn("hclen_4", [0] * 257, [0], [], 1, cl_lens=cl, hclen=4, eob=False, isize=0)
    w = BitWriter()
    w.bits(1, 1)
    w.bits(3, 2)
    w.bits(0, 29)
    out.append(Malformed("block_type_3", w.getvalue(), 9, "invalid DEFLATE block type"))
    out.append(Malformed("nlen_mismatch", DeflateWriter().stored(b"malformed", 1, nlen=9).getvalue(), 9, "stored block length check failed"))
    for sym in (286, 287):
        out.append(Malformed(f"fixed_litlen_symbol_{sym}", DeflateWriter().fixed(lits + [("raw", sym, 0, 0, 0)], 1).getvalue(), 12))
    for sym in (30, 31):
        out.append(Malformed(f"fixed_distance_code_{sym}", DeflateWriter().fixed(lits + [("raw", 257, 0, sym, 0)], 1).getvalue(), 12))
    out.append(Malformed("distance_1_at_position_0", DeflateWriter().fixed([("raw", 257, 0, 0, 0)], 1).getvalue(), 3,
                         "match distance reaches before the block"))
    # (this one cannot keep ISIZE at or below 1 024: the decoder refuses output beyond ISIZE before it looks at a distance)
    body = [("lit", rng.randrange(256)) for _ in range(3000)]
    d = dist_symbol(3001)
    out.append(Malformed("distance_3001_at_position_3000", DeflateWriter().dynamic(GEN_LL, GEN_DL, body + [("raw", 257, 0, d[0], d[1])], 1).getvalue(),
                         3003, "match distance reaches before the block"))
    # a stored LEN beyond the member's input (and within ISIZE, so that nothing else refuses it first)
    out.append(Malformed("stored_len_exceeds_input", DeflateWriter().stored(b"only ten b", 1, len_=1000).getvalue(), 1000, TEXT_INPUT_OVERRUN))
    # a Huffman block cut inside its last symbol by BSIZE: the member's payload ends one byte early, inside the 15-bit
    # end-of-block code; the byte cut off stands where the trailer's CRC begins, so the decoder reads the whole stream, finds
    # ISIZE bytes -- and has consumed more than the member holds
    ll = complete_lengths(rng, 286, 15, longest_first=[256, 0x41])
    s = Syms(rng, ll=ll).fill(500)
    s.lit(0x41)
    raw = DeflateWriter().dynamic(ll, GEN_DL, s.s, 1).getvalue()
    out.append(Malformed("huffman_block_cut_mid_symbol", raw[:-1], s.pos, TEXT_INPUT_OVERRUN, raw[-1:]))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------------
# (h) random sweep
# ---------------------------------------------------------------------------------------------------------------------------
SWEEP_SEEDS = tuple(range(24))


def _random_sets(rng):
    """A random complete literal/length set (longest code 7..15 bits) with the end of block, some literals and some length codes
    in it, and a random complete distance set."""
    max_len = rng.randrange(7, 16)
    n_used = rng.randrange(max_len + 1, min(286, 1 << max_len) + 1)
    need = {256, rng.randrange(256), rng.randrange(257, 265), rng.randrange(257, 286)}
    used = set(rng.sample(range(286), max(0, n_used - len(need)))) | need
    ll = complete_lengths(rng, 286, max_len, used=sorted(used))
    while ll[-1] == 0 and len(ll) > 257 and rng.random() < 0.7:   # (HLIT varies)
        ll.pop()
    dused = set(rng.sample(range(30), rng.randrange(2, 31))) | {rng.randrange(4)}
    d_max = min(rng.randrange(1, 16), len(dused) - 1)
    while len(dused) > (1 << d_max):
        d_max += 1
    dl = complete_lengths(rng, 30, d_max, used=sorted(dused))
    while dl[-1] == 0 and len(dl) > 1 and rng.random() < 0.7:
        dl.pop()
    return ll, dl


def _plain_cl(rng, seq):
    """A complete code-length code (longest 3..7 bits) for a header that sends every length as itself."""
    need = sorted(set(seq))
    used = set(need)
    while len(used) < 4:
        used.add(rng.randrange(19))
    max_len = rng.randrange(3, 8)
    while len(used) > (1 << max_len):
        max_len += 1
    return complete_lengths(rng, 19, max_len, used=sorted(used))


@functools.lru_cache(maxsize=None)
def sweep_cases(seed: int):
    """About 40 members of 1..4 deflate blocks of random type; two of them grow to 65 536 bytes."""
    rng = random.Random(9000 + seed)
    out = []
    n_members = rng.randrange(36, 45)
    big = set(rng.sample(range(n_members), 2))
    for m in range(n_members):
        target = rng.randrange(40_000, 65_537) if m in big else rng.randrange(1, 4097)
        if rng.random() < 0.1:
            target = 65536 if m in big else 4096
        n_blocks = rng.randrange(1, 5)
        cuts = sorted(rng.randrange(0, target + 1) for _ in range(n_blocks - 1)) + [target]
        dw, pos, kinds = DeflateWriter(), 0, []
        for k, upto in enumerate(cuts):
            last = k == n_blocks - 1
            kind = rng.choice(("stored", "fixed", "dynamic", "dynamic"))
            if kind == "stored" and upto - pos > (2000 if m in big else 65535):
                kind = "fixed"
            kinds.append(kind[0])
            if kind == "stored":
                dw.stored(bytes(rng.randrange(256) for _ in range(upto - pos)), last)
                pos = upto
                continue
            ll, dl = (FIXED_LITLEN[:286], FIXED_DIST[:30]) if kind == "fixed" else _random_sets(rng)
            s = Syms(rng, start=pos, ll=ll, dl=dl)
            s.fill(upto, p_lit=0.05 if m in big else rng.choice((0.1, 0.5, 0.9)), edges=DIST_EDGES, far=rng.choice((300, 3000, 40000)))
            if kind == "fixed":
                dw.fixed(s.s, last)
            elif rng.random() < 0.5:
                dw.dynamic(ll, dl, s.s, last, header="plain", cl_lens=_plain_cl(rng, ll + dl))
            else:
                dw.dynamic(ll, dl, s.s, last, header="rle")
            pos = s.pos
        out.append(_case("h", f"seed{seed}_member{m}_{''.join(kinds)}", dw))
    return tuple(out)
