"""A restatement of `ngs convert <BAM> <SAM>` in plain Python: the SAM text of a BAM file.

It reads the file itself (tests/bai_model.read_blocks: zlib and its own BGZF walk), takes the header text as the file holds
it (trailing NULs dropped, a final newline added when missing, nothing for an empty text) and writes one line per record
with the rules of section 13.1: QNAME without its NUL, FLAG / MAPQ / TLEN in decimal, 1-based POS and PNEXT (0 for -1), RNAME
and RNEXT from the binary reference list (`*` for -1, `=` for a mate on the record's own sequence), the CIGAR (a long CIGAR's
operations from its CG:B,I tag, which then is no tag of the line), SEQ by nibble, QUAL + 33 (`*` when there are no bases or
the first byte is 0xFF), the tags in file order with every integer type as `i` and floats as Rust's Display prints an f32
(section 13.2: numpy's shortest unique positional form, which the GPU tests hold the device's to).

A record without SAM text raises SamError with the library's message (section 13.3).  Nothing here calls the library."""
from __future__ import annotations

import struct
from typing import List, Optional, Tuple

import numpy as np

from tests import bai_model as bm

SEQ_CODES = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"
B_WIDTH = {b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}
INT_FMT = {b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I"}

# the library's SamError codes (ngs_amd/csrc/sam_kernels.h) and texts (sam.cpp): the smallest code of a record is reported
E_REF, E_CIGAR_OP, E_QUAL, E_TAG_TYPE, E_STR_NUL, E_B_SUB, E_OVERRUN = 1, 2, 3, 4, 5, 6, 7
ERROR_TEXT = {
    E_REF: "reference sequence id out of range",
    E_CIGAR_OP: "invalid CIGAR operation",
    E_QUAL: "quality score above 93",
    E_TAG_TYPE: "invalid tag value type",
    E_STR_NUL: "Z or H tag value without its NUL",
    E_B_SUB: "invalid B array subtype",
    E_OVERRUN: "tag value runs past the end of the record",
}


class SamError(ValueError):
    """A record without SAM text: .index its 0-based index in the file, .code its SamError code."""

    def __init__(self, index: int, code: int):
        self.index, self.code = index, code
        super().__init__(self.message)

    @property
    def message(self) -> str:
        return f"writing SAM record: record {self.index}: {ERROR_TEXT[self.code]}"


def fmt_f32(x) -> str:
    """An f32 as Rust's Display prints it: shortest digits that read back, closest, positional; NaN, inf, -inf, -0."""
    f = np.float32(x)
    if np.isnan(f):
        return "NaN"
    if np.isinf(f):
        return "inf" if f > 0 else "-inf"
    return np.format_float_positional(f, unique=True, trim="-")


def records_written(n_records: int, num_records: Optional[int]) -> int:
    """`-n` (RecordCounter::time_to_break, tested behind the write): min(records, max(N, 1)); every record without -n."""
    return n_records if num_records is None else min(n_records, max(num_records, 1))


def header_text(text: str) -> bytes:
    t = text.encode("latin-1") if isinstance(text, str) else text
    t = t.rstrip(b"\0")
    return t + b"\n" if t and not t.endswith(b"\n") else t


def _find_cg(s: bytes, p: int, end: int) -> int:
    """The offset of the first CG:B,I tag in s[p:end] if the tags in front of it are whole and it holds >= 2 values, else -1
    (the ingest's rule for a long CIGAR, SAM specification 4.2.2)."""
    p0 = p
    while end - p >= 4:
        tag, ty, at = s[p:p + 2], s[p + 2:p + 3], p
        p += 3
        if ty in (b"A", b"c", b"C"):
            n = 1
        elif ty in (b"s", b"S"):
            n = 2
        elif ty in (b"i", b"I", b"f"):
            n = 4
        elif ty in (b"Z", b"H"):
            z = s.find(b"\0", p, end)
            if z < 0:
                return -1
            p, n = z, 1
        elif ty == b"B":
            if end - p < 5:
                return -1
            sub, cnt = s[p:p + 1], struct.unpack_from("<I", s, p + 1)[0]
            if sub not in B_WIDTH:
                return -1
            n = 5 + cnt * B_WIDTH[sub]
            if tag == b"CG" and sub == b"I":
                return at - p0 if end - p >= n and cnt >= 2 else -1
        else:
            return -1
        if end - p < n:
            return -1
        p += n
    return -1


def record_line(s: bytes, p: int, names: List[bytes]) -> Tuple[bytes, int, int]:
    """The line of the record whose block_size is at s[p]; the offset behind it; its smallest error code (0: none)."""
    bs, ref, pos, l_rn, mapq, _bin, n_op, flag, l_seq, nref, npos, tlen = struct.unpack_from("<IiiBBHHHIiii", s, p)
    body = p + 4
    end = body + bs
    errs = []

    def rname(r):
        if r == -1:
            return b"*"
        if r < -1 or r >= len(names):
            errs.append(E_REF)
            return b"*"
        return names[r]

    cig_at = body + 32 + l_rn
    ops = list(struct.unpack_from(f"<{n_op}I", s, cig_at))
    seq_at = cig_at + 4 * n_op
    qual_at = seq_at + (l_seq + 1) // 2
    aux = qual_at + l_seq
    cg = -1
    if n_op == 2 and l_seq and ops[0] == (l_seq << 4 | 4) and (ops[1] & 15) == 3:
        cg = _find_cg(s, aux, end)
        if cg >= 0:
            cnt = struct.unpack_from("<I", s, aux + cg + 4)[0]
            ops = list(struct.unpack_from(f"<{cnt}I", s, aux + cg + 8))
    f = [s[body + 32:body + 32 + l_rn - 1] if l_rn else b"", b"%d" % flag, rname(ref), b"%d" % (pos + 1), b"%d" % mapq]
    if not ops:
        f.append(b"*")
    else:
        if any((c & 15) > 8 for c in ops):
            errs.append(E_CIGAR_OP)
        f.append(b"".join(b"%d%s" % (c >> 4, (CIGAR_OPS + "???????")[c & 15].encode()) for c in ops))
    f.append(b"=" if nref == ref and ref >= 0 else rname(nref))
    f += [b"%d" % (npos + 1), b"%d" % tlen]
    if not l_seq:
        f += [b"*", b"*"]
    else:
        packed = np.frombuffer(s, np.uint8, (l_seq + 1) // 2, seq_at)
        nib = np.empty(2 * len(packed), np.uint8)
        nib[0::2], nib[1::2] = packed >> 4, packed & 15
        f.append(np.frombuffer(SEQ_CODES.encode(), np.uint8)[nib[:l_seq]].tobytes())
        q = np.frombuffer(s, np.uint8, l_seq, qual_at)
        if q[0] == 0xFF:
            f.append(b"*")
        else:
            if (q > 93).any():
                errs.append(E_QUAL)
            f.append((q.astype(np.uint16) + 33).astype(np.uint8).tobytes())
    # the tags
    t = aux
    while t < end:
        if end - t < 3:
            errs.append(E_OVERRUN)
            break
        tag, ty, v = s[t:t + 2], s[t + 2:t + 3], t + 3
        skip = t - aux == cg
        left = end - v
        text = None
        if ty in (b"A", b"c", b"C", b"s", b"S", b"i", b"I", b"f"):
            w = 1 if ty in (b"A", b"c", b"C") else 2 if ty in (b"s", b"S") else 4
            if left < w:
                errs.append(E_OVERRUN)
                break
            if ty == b"A":
                text = b"A:" + s[v:v + 1]
            elif ty == b"f":
                text = b"f:" + fmt_f32(np.frombuffer(s, np.float32, 1, v)[0]).encode()
            else:
                text = b"i:%d" % struct.unpack_from(INT_FMT[ty], s, v)[0]
            nxt = v + w
        elif ty in (b"Z", b"H"):
            z = s.find(b"\0", v, end)
            if z < 0:
                errs.append(E_STR_NUL)
                break
            text = ty + b":" + s[v:z]
            nxt = z + 1
        elif ty == b"B":
            if left < 5:
                errs.append(E_OVERRUN)
                break
            sub = s[v:v + 1]
            if sub not in B_WIDTH:
                errs.append(E_B_SUB)
                break
            cnt = struct.unpack_from("<I", s, v + 1)[0]
            if cnt * B_WIDTH[sub] > left - 5:
                errs.append(E_OVERRUN)
                break
            if sub == b"f":
                vals = [fmt_f32(x).encode() for x in np.frombuffer(s, np.float32, cnt, v + 5)]
            else:
                vals = [b"%d" % x for x in struct.unpack_from("<%d%s" % (cnt, INT_FMT[sub][1]), s, v + 5)]
            text = b"B:" + sub + b"".join(b"," + x for x in vals)
            nxt = v + 5 + cnt * B_WIDTH[sub]
        else:
            errs.append(E_TAG_TYPE)
            break
        if not skip:
            f.append(tag + b":" + text)
        t = nxt
    return b"\t".join(f) + b"\n", end, min(errs) if errs else 0


def read_bam(path: str) -> Tuple[bytes, List[bytes], bytes, int]:
    """The header text, the @SQ names of the binary list, the inflated stream and the offset of the first record."""
    _blocks, s, _size = bm.read_blocks(path)
    assert s[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", s, 4)[0]
    text = s[8:8 + l_text]
    n_ref = struct.unpack_from("<i", s, 8 + l_text)[0]
    p = 12 + l_text
    names = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", s, p)[0]
        names.append(s[p + 4:p + 4 + l_name].rstrip(b"\0"))
        p += 8 + l_name
    return text, names, s, p


def expected_sam(path: str, max_records: int = 0) -> bytes:
    """The bytes `ngs convert <path> x.sam` writes (max_records: the library's, 0 = all).  Raises SamError."""
    text, names, s, p = read_bam(path)
    out = [header_text(text)]
    k = 0
    while p < len(s) and (not max_records or k < max_records):
        line, p, err = record_line(s, p, names)
        if err:
            raise SamError(k, err)
        out.append(line)
        k += 1
    return b"".join(out)


def count_records(path: str) -> int:
    _text, _names, s, p = read_bam(path)
    k = 0
    while p < len(s):
        p += 4 + struct.unpack_from("<I", s, p)[0]
        k += 1
    return k
