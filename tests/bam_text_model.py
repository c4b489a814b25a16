"""A restatement of `ngs convert --gzip device <SAM> <BAM>` in plain Python: SAM text in, the decompressed
BAM stream out.

The header is the leading lines that start with `@`; their text goes into the stream unchanged and the reference list comes
from SN and LN of the @SQ lines.  Every other line becomes one record by the rules of section 18.1: POS - 1, the bin of
tests/bamio.py, SEQ letters (either case) as nibbles, QUAL - 33 (0xFF for `*`), CIGAR operations as `len << 4 | op` (more than
65535 of them: the placeholder and a CG:B,I tag behind the line's own tags), the tags in line order with `i` in the smallest
type that holds the value and `f` as Rust's f32::from_str reads it (exact arithmetic on fractions.Fraction here).

A line without a record raises TextError with the library's message; a refused header raises HeaderError.  Within a line the
fault furthest left is reported: the faults are ordered by field, the tags are walked in order and the walk ends at the first
faulty one, and inside one field or one tag the smallest code is taken.  Nothing here calls the library."""
from __future__ import annotations

import re
import struct
from fractions import Fraction
from typing import Dict, List, Optional, Tuple

from tests import bamio

SEQ_CODES = b"=ACMGRSVTWYHKDBN"
CIGAR_OPS = b"MIDNSHP=X"
FLOAT_TEXT_MAX = 48

(E_FIELDS, E_QNAME_EMPTY, E_QNAME_LONG, E_FLAG, E_RNAME, E_POS, E_MAPQ, E_CIGAR_DIGITS, E_CIGAR_OP, E_CIGAR_LEN, E_RNEXT, E_PNEXT,
 E_TLEN, E_SEQ, E_QUAL_NO_SEQ, E_QUAL_LEN, E_QUAL_CHAR, E_TAG_FORM, E_TAG_TYPE, E_B_SUB, E_NUMBER, E_HEX, E_FLOAT_LONG,
 E_TOO_LARGE) = range(1, 25)
ERROR_TEXT = {
    E_FIELDS: "fewer than 11 fields",
    E_QNAME_EMPTY: "empty read name",
    E_QNAME_LONG: "read name longer than 254 bytes",
    E_FLAG: "invalid FLAG",
    E_RNAME: "reference sequence name not in the header",
    E_POS: "invalid POS",
    E_MAPQ: "invalid MAPQ",
    E_CIGAR_DIGITS: "CIGAR operation without a length",
    E_CIGAR_OP: "invalid CIGAR operation",
    E_CIGAR_LEN: "CIGAR operation length of 2^28 or more",
    E_RNEXT: "mate reference sequence name not in the header",
    E_PNEXT: "invalid PNEXT",
    E_TLEN: "invalid TLEN",
    E_SEQ: "invalid SEQ base",
    E_QUAL_NO_SEQ: "QUAL without SEQ",
    E_QUAL_LEN: "QUAL length differs from SEQ length",
    E_QUAL_CHAR: "QUAL byte outside 33..126",
    E_TAG_FORM: "tag not of the form TG:T:V",
    E_TAG_TYPE: "invalid tag value type",
    E_B_SUB: "invalid B array subtype",
    E_NUMBER: "malformed number",
    E_HEX: "invalid H value",
    E_FLOAT_LONG: "float text longer than 48 characters",
    E_TOO_LARGE: "record larger than 2^31 bytes",
}


class TextError(ValueError):
    """A line without a BAM record: .index its 0-based record index in the file, .code its kind."""

    def __init__(self, index: int, code: int):
        self.index, self.code = index, code
        super().__init__(self.message)

    @property
    def message(self) -> str:
        return f"reading SAM record: record {self.index}: {ERROR_TEXT[self.code]}"


class HeaderError(ValueError):
    """A refused header; str() is the library's message."""

    def __init__(self, what: str):
        super().__init__("opening SAM input file: " + what)


# ---- f32 ----------------------------------------------------------------------------------------------------------------
_FLOAT = re.compile(rb"([+-]?)(?:([0-9]*)(?:\.([0-9]*))?)(?:[eE]([+-]?[0-9]+))?\Z")


def parse_f32(text: bytes) -> Optional[int]:
    """The bits of the f32 that Rust's f32::from_str reads from `text`, None if it is no float: a decimal with optional
    fraction and exponent, or inf / infinity / nan in any case, each with an optional sign; rounded to nearest, ties to even."""
    m = re.match(rb"([+-]?)(.*)\Z", text, re.S)
    sign = 0x80000000 if m.group(1) == b"-" else 0
    word = m.group(2).lower()
    if word in (b"inf", b"infinity"):
        return sign | 0x7F800000
    if word == b"nan":
        return sign | 0x7FC00000
    m = _FLOAT.match(text)
    if not m or not ((m.group(2) or b"") + (m.group(3) or b"")):
        return None
    digits = (m.group(2) or b"") + (m.group(3) or b"")
    d, q = int(digits), int(m.group(4) or 0) - len(m.group(3) or b"")
    if d == 0:
        return sign
    if len(str(d)) + q > 40:       # at least 10^40, past the largest float: no power of ten that large is built
        return sign | 0x7F800000
    if len(str(d)) + q < -46:      # under 10^-46, less than half the smallest denormal
        return sign
    v = Fraction(d) * Fraction(10) ** q
    # floor(log2 v), then v in units of the last place of its binade (the denormals share the lowest one's)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1
    E = max(e, -126)
    units = v / Fraction(2) ** (E - 23)
    n = units.numerator // units.denominator
    rest = units - n
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n & 1):
        n += 1
    if n == 1 << 24:
        n, E = 1 << 23, E + 1
    if E > 127:
        return sign | 0x7F800000
    return sign | (n if n < 1 << 23 else (E + 127) << 23 | (n - (1 << 23)))


# ---- the header -----------------------------------------------------------------------------------------------------------
def split_header(text: bytes) -> Tuple[bytes, bytes]:
    """(header text, the rest): the leading lines that start with `@`."""
    p = 0
    while p < len(text) and text[p:p + 1] == b"@":
        e = text.find(b"\n", p)
        p = len(text) if e < 0 else e + 1
    return text[:p], text[p:]


def references(header: bytes) -> List[Tuple[bytes, int]]:
    out, seen = [], set()
    for line in header.split(b"\n"):
        if not line.startswith(b"@SQ\t"):
            continue
        sn = ln = None
        for f in line.split(b"\t")[1:]:
            if f.startswith(b"SN:") and sn is None:
                sn = f[3:]
            if f.startswith(b"LN:") and ln is None:
                ln = f[3:]
        k = len(out) + 1
        if not sn:
            raise HeaderError(f"@SQ line {k} has no SN")
        name = sn.decode("latin-1")
        if ln is None:
            raise HeaderError(f"@SQ line {k} ({name}) has no LN")
        if not re.fullmatch(rb"[0-9]+", ln) or not 1 <= int(ln) <= 2 ** 31 - 1:
            raise HeaderError(f"@SQ line {k} ({name}): LN {ln.decode('latin-1')} is outside 1..2147483647")
        if sn in seen:
            raise HeaderError(f"@SQ line {k}: the sequence name {name} stands in more than one @SQ line")
        seen.add(sn)
        out.append((sn, int(ln)))
    return out


def header_stream(header: bytes, refs: List[Tuple[bytes, int]]) -> bytes:
    s = b"BAM\1" + struct.pack("<i", len(header)) + header + struct.pack("<i", len(refs))
    for n, l in refs:
        s += struct.pack("<i", len(n) + 1) + n + b"\0" + struct.pack("<i", l)
    return s


# ---- one line ---------------------------------------------------------------------------------------------------------------
def _dec(b: bytes, neg: bool = False) -> Optional[int]:
    return int(b) if re.fullmatch(rb"-?[0-9]+" if neg else rb"[0-9]+", b) else None


_B_RANGE = {b"c": (-128, 127), b"C": (0, 255), b"s": (-32768, 32767), b"S": (0, 65535), b"i": (-2 ** 31, 2 ** 31 - 1), b"I": (0, 2 ** 32 - 1)}
_B_FMT = {b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I"}


def _int_tag(v: int) -> bytes:
    """The smallest type that holds v (htslib's rule): C S I for v >= 0, c s i below."""
    if v >= 0:
        return b"C" + struct.pack("<B", v) if v < 256 else b"S" + struct.pack("<H", v) if v < 65536 else b"I" + struct.pack("<I", v)
    return b"c" + struct.pack("<b", v) if v >= -128 else b"s" + struct.pack("<h", v) if v >= -32768 else b"i" + struct.pack("<i", v)


def _tag(t: bytes) -> Tuple[bytes, int]:
    """(bytes, 0) of the tag TG:T:V, or (b"", code)."""
    if len(t) < 5 or t[2:3] != b":" or t[4:5] != b":":
        return b"", E_TAG_FORM
    tag, ty, v = t[:2], t[3:4], t[5:]
    if ty == b"A":
        return (tag + b"A" + v, 0) if len(v) == 1 else (b"", E_TAG_FORM)
    if ty == b"i":
        x = _dec(v, True)
        return (tag + _int_tag(x), 0) if x is not None and -2 ** 31 <= x <= 2 ** 32 - 1 else (b"", E_NUMBER)
    if ty == b"f":
        if len(v) > FLOAT_TEXT_MAX:
            return b"", E_FLOAT_LONG
        u = parse_f32(v)
        return (tag + b"f" + struct.pack("<I", u), 0) if u is not None else (b"", E_NUMBER)
    if ty == b"Z":
        return tag + b"Z" + v + b"\0", 0
    if ty == b"H":
        return (tag + b"H" + v + b"\0", 0) if len(v) % 2 == 0 and re.fullmatch(rb"[0-9A-Fa-f]*", v) else (b"", E_HEX)
    if ty == b"B":
        if not v:
            return b"", E_TAG_FORM
        sub = v[:1]
        if sub not in b"cCsSiIf":
            return b"", E_B_SUB
        if len(v) > 1 and v[1:2] != b",":
            return b"", E_NUMBER
        items = v[2:].split(b",") if len(v) > 1 else []
        errs, out = [], b""
        for it in items:
            if sub == b"f":
                u = None if len(it) > FLOAT_TEXT_MAX else parse_f32(it)
                if u is None:
                    errs.append(E_FLOAT_LONG if len(it) > FLOAT_TEXT_MAX else E_NUMBER)
                else:
                    out += struct.pack("<I", u)
            else:
                lo, hi = _B_RANGE[sub]
                x = _dec(it, lo < 0)
                if x is None or not lo <= x <= hi:
                    errs.append(E_NUMBER)
                else:
                    out += struct.pack(_B_FMT[sub], x)
        if errs:
            return b"", min(errs)
        return tag + b"B" + sub + struct.pack("<I", len(items)) + out, 0
    return b"", E_TAG_TYPE


def record(line: bytes, ref_id: Dict[bytes, int]) -> Tuple[bytes, int]:
    """(the record's bytes with its block_size, 0), or (b"", the code of the fault furthest left)."""
    f = line.split(b"\t")
    if len(f) < 11:
        return b"", E_FIELDS
    errs = []
    if not f[0]:
        errs.append(E_QNAME_EMPTY)
    if len(f[0]) > 254:
        errs.append(E_QNAME_LONG)

    def number(b, code, hi, neg=False, lo=0):
        x = _dec(b, neg)
        if x is None or not lo <= x <= hi:
            errs.append(code)
            return 0
        return x

    def ref_of(b, code):
        if b == b"*":
            return -1
        if b not in ref_id:
            errs.append(code)
            return -1
        return ref_id[b]

    flag = number(f[1], E_FLAG, 65535)
    ref = ref_of(f[2], E_RNAME)
    pos = number(f[3], E_POS, 2 ** 31 - 1) - 1
    mapq = number(f[4], E_MAPQ, 255)
    ops = []
    if f[5] != b"*":
        pieces = re.findall(rb"([0-9]*)([^0-9])", f[5])
        if not f[5] or f[5][-1:].isdigit():
            errs.append(E_CIGAR_DIGITS)
        for num, op in pieces:
            if not num:
                errs.append(E_CIGAR_DIGITS)
            if op not in CIGAR_OPS:
                errs.append(E_CIGAR_OP)
            if num and int(num) >= 1 << 28:
                errs.append(E_CIGAR_LEN)
            ops.append((int(num or 0) & 0x0FFFFFFF) << 4 | max(CIGAR_OPS.find(op), 0))
    nref = ref if f[6] == b"=" else ref_of(f[6], E_RNEXT)
    npos = number(f[7], E_PNEXT, 2 ** 31 - 1) - 1
    tlen = number(f[8], E_TLEN, 2 ** 31 - 1, True, -2 ** 31)
    seq = b"" if f[9] == b"*" else f[9].upper()
    if f[9] != b"*" and (not seq or any(c not in SEQ_CODES for c in seq)):
        errs.append(E_SEQ)
    l_seq = len(seq)
    nib = [max(SEQ_CODES.find(bytes([c])), 0) for c in seq] + [0]
    packed = bytes(nib[k] << 4 | nib[k + 1] for k in range(0, l_seq, 2))
    if f[10] == b"*":
        qual = b"\xff" * l_seq
    else:
        if f[9] == b"*":
            errs.append(E_QUAL_NO_SEQ)
        elif len(f[10]) != l_seq:
            errs.append(E_QUAL_LEN)
        if any(not 33 <= c <= 126 for c in f[10]):
            errs.append(E_QUAL_CHAR)
        qual = bytes((c - 33) & 255 for c in f[10])
    aux = b""
    for t in f[11:]:
        b, code = _tag(t)
        if code:
            errs.append(code)
            break
        aux += b
    if errs:
        return b"", min(errs)
    span = sum(c >> 4 for c in ops if c & 15 in (0, 2, 3, 7, 8))
    if len(ops) > 65535:  # SAM specification 4.2.2, as bamio.record_bytes writes it
        aux += b"CGBI" + struct.pack("<I", len(ops)) + struct.pack(f"<{len(ops)}I", *ops)
        ops = [l_seq << 4 | 4, (span << 4 | 3) & 0xFFFFFFFF]
    bin_ = bamio.reg2bin(pos, pos + max(span, 1)) & 0xFFFF if pos >= 0 else 4680
    name = f[0] + b"\0"
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name), mapq, bin_, len(ops), flag, l_seq, nref, npos, tlen)
    body += name + struct.pack(f"<{len(ops)}I", *ops) + packed + qual + aux
    if len(body) + 4 > 1 << 31:
        return b"", E_TOO_LARGE
    return struct.pack("<I", len(body)) + body, 0


def body_lines(body: bytes) -> List[bytes]:
    """The record lines: a last line without its newline is a line; a `\\r` is not treated specially."""
    lines = body.split(b"\n")
    return lines[:-1] if lines[-1] == b"" else lines


def bam_records(sam: bytes, max_records: int = 0) -> List[bytes]:
    header, body = split_header(sam)
    ref_id = {n: k for k, (n, _l) in enumerate(references(header))}
    out = []
    for k, line in enumerate(body_lines(body)):
        if max_records and k >= max_records:
            break
        b, code = record(line, ref_id)
        if code:
            raise TextError(k, code)
        out.append(b)
    return out


def bam_stream(sam: bytes, max_records: int = 0) -> bytes:
    """The decompressed BAM stream of the SAM text (max_records: the library's, 0 = all).  Raises HeaderError, TextError."""
    header, _body = split_header(sam)
    return header_stream(header, references(header)) + b"".join(bam_records(sam, max_records))


def bam_file(stream: bytes, block_payload: int = 65280) -> bytes:
    """A BAM file of the stream, its blocks written by zlib (tests/bamio.bgzf_block)."""
    return b"".join(bamio.bgzf_block(stream[k:k + block_payload]) for k in range(0, len(stream), block_payload)) + bamio.EOF_BLOCK
