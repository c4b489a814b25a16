"""A restatement of `ngs view <BAM> [QUERY]` in plain Python: the bytes the command writes.

Its own query parser (split at the last ':'; a suffix that reads as S or S-E makes the prefix the name) and its own reg2bins;
the index is read through bai_model.parse, the records with their virtual offsets through bai_model.read_file, and the lines
come from sam_model.record_line.  A record is written iff its virtual offset lies in a merged chunk of the query, its sequence
is the region's, pos >= 0 and [pos+1, pos+max(span, 1)] meets [S, E]; a record that is not selected is not examined for SAM text.

Nothing here calls the library: the tests hold the library's chunk query and the device's selection against this."""
from __future__ import annotations

import bisect
import re
import struct
from typing import List, Optional, Tuple

from tests import bai_model as bm
from tests import sam_model as sm

END_MAX = 1 << 29
MODES = ("full", "header-only", "records-only")


class ViewError(ValueError):
    """A refused view: .context is the reference's context ("parsing query", "querying BAM file", "reading BAM index",
    "writing record to stream")."""

    def __init__(self, context: str, what: str = ""):
        self.context = context
        super().__init__(f"{context}: {what}")


_INTERVAL = re.compile(r"\A([0-9]{1,18})(?:-([0-9]{1,18}))?\Z", re.ASCII)


def parse_query(query: str, names: List[str]) -> Tuple[int, int, int]:
    """(ref_id, S, E), 1-based inclusive, E = END_MAX for an interval without an end."""
    if query == "":
        raise ViewError("parsing query", "empty input")
    name, s, e = query, 1, END_MAX
    head, colon, tail = query.rpartition(":")
    m = _INTERVAL.match(tail) if colon else None
    if m:
        s2 = int(m.group(1))
        e2 = int(m.group(2)) if m.group(2) is not None else END_MAX
        if s2 >= 1 and (m.group(2) is None or e2 >= s2):
            name, s, e = head, s2, e2
    if name not in names:
        raise ViewError("querying BAM file", f"no sequence {name!r}")
    return names.index(name), s, e


def reg2bins(beg: int, end: int) -> List[int]:
    """SAM specification 5.3: the bins that may hold records overlapping the 0-based [beg, end)."""
    out = [0]
    end -= 1
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


def query_chunks(bai: bytes, ref_id: int, s: int, e: int) -> List[Tuple[int, int]]:
    """The merged chunks of the 1-based [s, e] on sequence ref_id."""
    try:
        refs, _ = bm.parse(bai)
    except (AssertionError, struct.error) as x:
        raise ViewError("reading BAM index", repr(x))
    if ref_id >= len(refs):
        raise ViewError("reading BAM index", "fewer sequences than the region's id")
    bins, lin = refs[ref_id]
    beg, lim = s - 1, min(e, END_MAX)
    if beg >= lim:
        return []
    w = beg >> 14
    min_offset = lin[w] if w < len(lin) else 0
    found = []
    for b in reg2bins(beg, lim):
        if b != bm.META_BIN:
            found += [c for c in bins.get(b, []) if c[1] > min_offset and c[1] > c[0]]
    merged: List[List[int]] = []
    for c0, c1 in sorted(found):
        if merged and c0 <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], c1)
        else:
            merged.append([c0, c1])
    return [tuple(c) for c in merged]


def selected(path: str, ref_id: int, s: int, e: int, chunks) -> List[int]:
    """The indices in the file of the records the query writes."""
    recs, _lens, _text = bm.read_file(path)
    # a record's virtual offset is where its first byte lies (the readers' record_id).  bai_model's chunk start v0 is the
    # position behind the record in front, which names the same byte except behind an empty BGZF member, where no record lies
    offs = record_offsets(path)
    keep = []
    for i, r in enumerate(recs):
        if not any(c0 <= offs[i] < c1 for c0, c1 in chunks):
            continue
        if r.ref != ref_id or r.pos < 0:
            continue
        if r.pos + 1 <= e and r.pos + max(r.span, 1) >= s:
            keep.append(i)
    return keep


def record_offsets(path: str) -> List[int]:
    """The virtual offset of every record's first byte (block file offset << 16 | offset in the block's data): the record_id
    of the readers.  A first byte is never at a block's end, so it lies in the last block that starts at or before it and has data."""
    blocks, s, _size = bm.read_blocks(path)
    data_blocks = [b for b in blocks if b.isize]
    outs = [b.out for b in data_blocks]
    _text, _names, s2, p = sm.read_bam(path)
    offs = []
    while p < len(s2):
        k = bisect.bisect_right(outs, p) - 1
        offs.append(data_blocks[k].coff << 16 | (p - data_blocks[k].out))
        p += 4 + struct.unpack_from("<I", s2, p)[0]
    return offs


def header_bytes(path: str) -> bytes:
    """The header text exactly as the file holds it (trailing NULs dropped, as the library's reader keeps it; no newline added)."""
    text, _names, _s, _p = sm.read_bam(path)
    return text.rstrip(b"\0")


def expected_view(path: str, query: Optional[str] = None, mode: str = "full", bai: Optional[bytes] = None) -> bytes:
    """The bytes `ngs view [-m mode] <path> [query]` writes.  Raises ViewError."""
    assert mode in MODES
    head = header_bytes(path)
    if mode == "header-only":
        return head
    text, names, s, p = sm.read_bam(path)
    keep = None
    if query is not None:
        if bai is None:
            try:
                bai = open(path + ".bai", "rb").read()
            except OSError as x:
                raise ViewError("reading BAM index", str(x))
        ref_id, qs, qe = parse_query(query, [n.decode("latin-1") for n in names])
        keep = set(selected(path, ref_id, qs, qe, query_chunks(bai, ref_id, qs, qe)))
    out = [head] if mode == "full" else []
    k = 0
    while p < len(s):
        if keep is None or k in keep:
            line, p, err = sm.record_line(s, p, names)
            if err:
                raise ViewError("writing record to stream", f"record {k}: {sm.ERROR_TEXT[err]}")
            out.append(line)
        else:
            p += 4 + struct.unpack_from("<I", s, p)[0]
        k += 1
    return b"".join(out)
