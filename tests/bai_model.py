"""A restatement of `ngs index` for BAM in plain Python: the BAI a coordinate-sorted BAM file gets.

It reads the file itself (zlib; its own BGZF block table and record walk), gives every record its chunk -- from the
virtual position behind the record in front of it (or behind the header) to the virtual position behind its own last
byte, the start of the next block when that byte ends a block, empty or not -- and writes the index with the rules of
section 12.1: reg2bin over the reference span (at least 1), a record's chunk merged into the last chunk of its bin only
when that chunk ends where it starts, bins ascending, the metadata pseudo-bin 37450 last, the 16 kb linear index with the
first record's chunk start per window and gaps carrying the value in front of them, n_no_coor at the end.  A placed record
the index cannot hold (include/ngsq_index.h: a sequence id outside the header, an end beyond 2^29, a window at or beyond
ceil(LN / 16384) + 64) is refused, behind any order violation of the file.

Nothing here calls the library: the GPU tests hold the device-built index against this."""
from __future__ import annotations

import bisect
import struct
import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

META_BIN = 37450


class Unsorted(ValueError):
    """A record breaks the coordinate order; .index is its index in the file."""

    def __init__(self, index: int):
        super().__init__(f"record {index} is out of coordinate order")
        self.index = index


MAX_POS = 1 << 29      # the binning scheme's coordinate range (SAM specification 5.3)
LIN_SLACK = 64         # 16 kb windows kept beyond @SQ LN: 1 Mbp


class Limit(ValueError):
    """A placed record the BAI cannot hold; .index is the first such record's index in the file."""

    def __init__(self, index: int):
        super().__init__(f"record {index} (0-based) cannot be held by a BAI: its sequence id is out of range, or it reaches "
                         "beyond position 2^29 or more than 1 Mbp beyond its @SQ LN")
        self.index = index


def lin_cap(ln: int) -> int:
    """The 16 kb windows kept for a sequence of length ln."""
    return min((ln + 16383) // 16384 + LIN_SLACK, MAX_POS >> 14)


def beyond_limit(r: "Rec", n_ref: int, ref_lens: Optional[Sequence[int]]) -> bool:
    """The limit rule for a placed record (ref_lens None: the lengths are not known, only the first two rules apply)."""
    end = r.pos + max(r.span, 1)
    if r.ref >= n_ref or end > MAX_POS:
        return True
    return ref_lens is not None and (end - 1) >> 14 >= lin_cap(ref_lens[r.ref])


def reg2bin(beg: int, end: int) -> int:
    """SAM specification 5.3 (end exclusive)."""
    end -= 1
    for shift, off in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return off + (beg >> shift)
    return 0


@dataclass
class Block:
    coff: int   # file offset of the gzip member
    out: int    # offset of its data in the inflated stream
    isize: int  # bytes of data (0: an empty member, e.g. the EOF marker)


@dataclass
class Rec:
    ref: int
    pos: int
    flag: int
    span: int   # reference length of the CIGAR: M D N = X
    v0: int = 0  # chunk start
    v1: int = 0  # chunk end


def read_blocks(path: str) -> Tuple[List[Block], bytes, int]:
    """The BGZF members of the file (SAM specification 4.1), the inflated stream, and the file size."""
    raw = open(path, "rb").read()
    blocks, data, p = [], [], 0
    out = 0
    while p < len(raw):
        if raw[p:p + 4] != b"\x1f\x8b\x08\x04":
            raise ValueError(f"not a BGZF member at {p}")
        xlen = struct.unpack_from("<H", raw, p + 10)[0]
        bsize, q = None, p + 12
        while q < p + 12 + xlen:
            si, slen = raw[q:q + 2], struct.unpack_from("<H", raw, q + 2)[0]
            if si == b"BC" and slen == 2:
                bsize = struct.unpack_from("<H", raw, q + 4)[0] + 1
            q += 4 + slen
        isize = struct.unpack_from("<I", raw, p + bsize - 4)[0]
        d = zlib.decompress(raw[p + 12 + xlen:p + bsize - 8], -15)
        assert len(d) == isize
        blocks.append(Block(p, out, isize))
        data.append(d)
        out += isize
        p += bsize
    return blocks, b"".join(data), len(raw)


def pos_after(blocks: Sequence[Block], e: int, file_size: int, outs: Optional[Sequence[int]] = None) -> int:
    """The virtual position behind stream byte e - 1: inside its block, or -- its block's last byte -- the start of the
    member behind that block (empty or not; the file size when there is none)."""
    outs = outs if outs is not None else [b.out for b in blocks]
    k = bisect.bisect_right(outs, e - 1) - 1   # the last member whose data starts at or before e - 1
    b = blocks[k]                                                    # (an empty member there is followed by one with data)
    if e == b.out + b.isize:
        return (blocks[k + 1].coff if k + 1 < len(blocks) else file_size) << 16
    return b.coff << 16 | (e - b.out)


def _cigar_span(ops) -> int:
    return sum(c >> 4 for c in ops if (c & 15) in (0, 2, 3, 7, 8))


def _cg_tag(aux: bytes) -> Optional[List[int]]:
    """The CG:B,I array of the auxiliary data (SAM specification 4.2.2), or None."""
    p = 0
    sizes = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}
    while p + 3 <= len(aux):
        tag, ty = aux[p:p + 2], aux[p + 2:p + 3]
        p += 3
        if ty in sizes:
            p += sizes[ty]
        elif ty in (b"Z", b"H"):
            p = aux.index(b"\0", p) + 1
        elif ty == b"B":
            sub, cnt = aux[p:p + 1], struct.unpack_from("<I", aux, p + 1)[0]
            if tag == b"CG" and sub == b"I":
                return list(struct.unpack_from(f"<{cnt}I", aux, p + 5))
            p += 5 + cnt * sizes[sub]
        else:
            return None
    return None


def read_records(path: str) -> Tuple[List[Rec], int, List[str]]:
    """Every record of a BAM file with its chunk; the number of @SQ sequences; the header text."""
    recs, lens, text = read_file(path)
    return recs, len(lens), text


def read_file(path: str) -> Tuple[List[Rec], List[int], List[str]]:
    """Every record of a BAM file with its chunk; the lengths of the binary reference list; the header text."""
    blocks, s, size = read_blocks(path)
    assert s[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", s, 4)[0]
    text = s[8:8 + l_text].decode()
    n_ref = struct.unpack_from("<i", s, 8 + l_text)[0]
    p = 12 + l_text
    lens = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", s, p)[0]
        lens.append(struct.unpack_from("<i", s, p + 4 + l_name)[0])
        p += 8 + l_name
    recs: List[Rec] = []
    outs = [b.out for b in blocks]
    prev_end = pos_after(blocks, p, size, outs)
    while p < len(s):
        bs, ref, pos, l_rn, _mq, _bin, n_op, flag, l_seq = struct.unpack_from("<iiiBBHHHi", s, p)
        body = p + 4
        cig_at = body + 32 + l_rn
        ops = list(struct.unpack_from(f"<{n_op}I", s, cig_at))
        if n_op == 2 and l_seq and ops[0] == (l_seq << 4 | 4) and (ops[1] & 15) == 3:
            aux_at = cig_at + 4 * n_op + (l_seq + 1) // 2 + l_seq
            cg = _cg_tag(s[aux_at:body + bs])
            if cg is not None and len(cg) >= 2:
                ops = cg
        end = body + bs
        v1 = pos_after(blocks, end, size, outs)
        recs.append(Rec(ref, pos, flag, _cigar_span(ops), prev_end, v1))
        prev_end = v1
        p = end
    return recs, lens, text.splitlines()


def build(recs: Sequence[Rec], n_ref: int, meta: bool = True, ref_lens: Optional[Sequence[int]] = None) -> bytes:
    """The BAI bytes of records given in file order with their chunks.  Raises Unsorted for the first record out of order,
    and for a file in order Limit for the first record the index cannot hold (ref_lens: the @SQ lengths)."""
    limit = None
    last, seen_unplaced = None, False
    for i, r in enumerate(recs):
        if not (r.ref >= 0 and r.pos >= 0):
            seen_unplaced = True
            continue
        if seen_unplaced or (last is not None and (r.ref, r.pos) < last):
            raise Unsorted(i)
        last = (r.ref, r.pos)
        if limit is None and beyond_limit(r, n_ref, ref_lens):
            limit = i
    if limit is not None:
        raise Limit(limit)
    bins: List[Dict[int, List[List[int]]]] = [dict() for _ in range(n_ref)]
    lin: List[Dict[int, int]] = [dict() for _ in range(n_ref)]
    stats = [None] * n_ref  # [ref_beg, ref_end, n_mapped, n_unmapped]
    n_no_coor = 0
    last = None  # (ref, pos) of the previous record, None when it was unplaced
    seen_unplaced = False
    for i, r in enumerate(recs):
        placed = r.ref >= 0 and r.pos >= 0
        if not placed:
            n_no_coor += 1
            seen_unplaced = True
            continue
        if seen_unplaced or (last is not None and (r.ref, r.pos) < last):
            raise Unsorted(i)
        last = (r.ref, r.pos)
        end = r.pos + max(r.span, 1)
        chunks = bins[r.ref].setdefault(reg2bin(r.pos, end), [])
        if chunks and chunks[-1][1] == r.v0:
            chunks[-1][1] = r.v1
        else:
            chunks.append([r.v0, r.v1])
        for w in range(r.pos >> 14, ((end - 1) >> 14) + 1):
            lin[r.ref].setdefault(w, r.v0)
        st = stats[r.ref]
        if st is None:
            st = stats[r.ref] = [r.v0, r.v1, 0, 0]
        st[1] = r.v1
        st[3 if r.flag & 4 else 2] += 1
    out = bytearray(b"BAI\1" + struct.pack("<i", n_ref))
    for ref in range(n_ref):
        has_meta = meta and stats[ref] is not None
        out += struct.pack("<i", len(bins[ref]) + has_meta)
        for b in sorted(bins[ref]):
            out += struct.pack("<Ii", b, len(bins[ref][b]))
            for c0, c1 in bins[ref][b]:
                out += struct.pack("<QQ", c0, c1)
        if has_meta:
            out += struct.pack("<Ii", META_BIN, 2) + struct.pack("<QQQQ", *stats[ref])
        n_intv = max(lin[ref]) + 1 if lin[ref] else 0
        out += struct.pack("<i", n_intv)
        carry = 0
        for w in range(n_intv):
            carry = lin[ref].get(w, carry)
            out += struct.pack("<Q", carry)
    out += struct.pack("<Q", n_no_coor)
    return bytes(out)


def expected_bai(path: str, meta: bool = True) -> bytes:
    recs, lens, _ = read_file(path)
    return build(recs, len(lens), meta, lens)


def parse(bai: bytes):
    """[(bins {bin: [(beg, end), ...]}, linear [..]) per sequence], n_no_coor (None: absent)."""
    assert bai[:4] == b"BAI\1"
    n_ref = struct.unpack_from("<i", bai, 4)[0]
    p, refs = 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", bai, p)[0]
        p += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, p)
            p += 8
            bins[b] = [struct.unpack_from("<QQ", bai, p + 16 * k) for k in range(n_chunk)]
            p += 16 * n_chunk
        n_intv = struct.unpack_from("<i", bai, p)[0]
        p += 4
        refs.append((bins, list(struct.unpack_from(f"<{n_intv}Q", bai, p))))
        p += 8 * n_intv
    n_no_coor = struct.unpack_from("<Q", bai, p)[0] if p + 8 <= len(bai) else None
    return refs, n_no_coor


def strip_meta(bai: bytes) -> bytes:
    """The same index without the pseudo-bin 37450 (what the project's other writers leave out)."""
    refs, n_no_coor = parse(bai)
    out = bytearray(b"BAI\1" + struct.pack("<i", len(refs)))
    for bins, lin in refs:
        kept = {b: c for b, c in bins.items() if b != META_BIN}
        out += struct.pack("<i", len(kept))
        for b in sorted(kept):
            out += struct.pack("<Ii", b, len(kept[b]))
            for c in kept[b]:
                out += struct.pack("<QQ", *c)
        out += struct.pack("<i", len(lin)) + struct.pack(f"<{len(lin)}Q", *lin)
    if n_no_coor is not None:
        out += struct.pack("<Q", n_no_coor)
    return bytes(out)
