"""A restatement of `ngs depth <BAM> [QUERY]` (include/ngsq_depth.h) in plain Python: the bytes the command
writes and the counts of its report.

The records are read here (the inflated stream through bai_model.read_blocks, then a record walk of its own that keeps the mapq;
a long CIGAR's operations come from CG:B,I), every sequence gets a numpy difference array, and the text is the runs of its
running sum.  A record counts iff ref >= 0, pos >= 0, (flag & exclude_flags) == 0 and mapq >= min_mapq; it covers
[pos, min(pos + span, L)) and nothing without a span.  With a query the records are those `ngs view` finds (view_model: the
merged chunks of the index, the region's sequence, [pos + 1, pos + max(span, 1)] meeting [S, E]) and the interval
[S - 1, min(E, L)) is tiled.

Nothing here calls the library: the GPU tests hold the library's bytes against this."""
from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests import bai_model as bm
from tests import view_model as vm

EXCLUDE_FLAGS = 1796   # unmapped 0x4, secondary 0x100, QC-fail 0x200, duplicate 0x400
NOT_SORTED = "the input BAM must be coordinate-sorted to compute depth"


class DepthError(ValueError):
    """A refused call: the message of the library."""


@dataclass
class Rec:
    ref: int
    pos: int
    flag: int
    mapq: int
    span: int   # reference bases of the resolved CIGAR: M D N = X


def read(path: str) -> Tuple[List[bytes], List[int], List[Rec], str]:
    """The names and lengths of the binary reference list, every record in file order, the header text."""
    _blocks, s, _size = bm.read_blocks(path)
    assert s[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", s, 4)[0]
    text = s[8:8 + l_text].decode()
    n_ref = struct.unpack_from("<i", s, 8 + l_text)[0]
    p = 12 + l_text
    names, lens = [], []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", s, p)[0]
        names.append(s[p + 4:p + 4 + l_name - 1])
        lens.append(struct.unpack_from("<i", s, p + 4 + l_name)[0])
        p += 8 + l_name
    recs: List[Rec] = []
    while p < len(s):
        bs, ref, pos, l_rn, mapq, _bin, n_op, flag, l_seq = struct.unpack_from("<iiiBBHHHi", s, p)
        body = p + 4
        cig_at = body + 32 + l_rn
        ops = list(struct.unpack_from(f"<{n_op}I", s, cig_at))
        if n_op == 2 and l_seq and ops[0] == (l_seq << 4 | 4) and (ops[1] & 15) == 3:   # the long-CIGAR placeholder (SAM 4.2.2)
            cg = bm._cg_tag(s[cig_at + 4 * n_op + (l_seq + 1) // 2 + l_seq:body + bs])
            if cg is not None and len(cg) >= 2:
                ops = cg
        recs.append(Rec(ref, pos, flag, mapq, sum(c >> 4 for c in ops if (c & 15) in (0, 2, 3, 7, 8))))
        p = body + bs
    return names, lens, recs, text


def sorted_header(text: str) -> bool:
    """The @HD line says SO:coordinate."""
    for line in text.split("\n"):
        if line.startswith("@HD"):
            return "SO:coordinate" in line.split("\t")[1:]
    return False


def first_out_of_order(recs: Sequence[Rec]) -> Optional[int]:
    """The index of the first record that breaks the order of `ngs index`: (sequence, position), unplaced records last."""
    last, seen_unplaced = None, False
    for i, r in enumerate(recs):
        if not (r.ref >= 0 and r.pos >= 0):
            seen_unplaced = True
            continue
        if seen_unplaced or (last is not None and (r.ref, r.pos) < last):
            return i
        last = (r.ref, r.pos)
    return None


def counts(r: Rec, exclude_flags: int = EXCLUDE_FLAGS, min_mapq: int = 0) -> bool:
    return r.ref >= 0 and r.pos >= 0 and (r.flag & exclude_flags) == 0 and r.mapq >= min_mapq


def depths(recs: Sequence[Rec], ref: int, lo: int, hi: int) -> np.ndarray:
    """The depth of every position of [lo, hi) on sequence ref under the records given (all of them count)."""
    d = np.zeros(hi - lo + 1, dtype=np.int64)
    for r in recs:
        if r.ref != ref or r.span < 1:
            continue
        a, e = max(r.pos, lo), min(r.pos + r.span, hi)
        if a < e:
            d[a - lo] += 1
            d[e - lo] -= 1
    return np.cumsum(d[:-1])


def runs(depth: np.ndarray) -> List[Tuple[int, int, int]]:
    """(start, end, depth) of the maximal runs of equal depth, positions relative to the array."""
    if depth.size == 0:
        return []
    starts = np.concatenate([[0], np.flatnonzero(depth[1:] != depth[:-1]) + 1])
    ends = np.concatenate([starts[1:], [depth.size]])
    return [(int(s), int(e), int(depth[s])) for s, e in zip(starts, ends)]


def text_of(name: bytes, lo: int, depth: np.ndarray) -> Tuple[bytes, int]:
    """The bedGraph lines of one tiled interval that begins at coordinate lo, and their number."""
    rs = runs(depth)
    return b"".join(b"%s\t%d\t%d\t%d\n" % (name, lo + s, lo + e, d) for s, e, d in rs), len(rs)


def expected(path: str, query: Optional[str] = None, exclude_flags: int = EXCLUDE_FLAGS, min_mapq: int = 0,
             bai: Optional[bytes] = None) -> Tuple[bytes, Dict[str, int]]:
    """The bytes `ngs depth` writes, and the counts of its report: records_scanned (None with a query: the walks decide),
    records_counted, runs, sequences.  Raises DepthError with the library's message; view_model.ViewError for a bad query or index."""
    names, lens, recs, text = read(path)
    if not sorted_header(text):
        raise DepthError(NOT_SORTED)
    if query is None:
        bad = first_out_of_order(recs)
        if bad is not None:
            raise DepthError(f"reading BAM record: record {bad} (0-based) is out of coordinate order: {NOT_SORTED}")
        kept = [r for r in recs if counts(r, exclude_flags, min_mapq)]
        out, n_runs, n_seq = [], 0, 0
        for ref, (name, ln) in enumerate(zip(names, lens)):
            t, k = text_of(name, 0, depths(kept, ref, 0, ln))
            out.append(t)
            n_runs += k
            n_seq += k > 0
        return b"".join(out), dict(records_scanned=len(recs), records_counted=len(kept), runs=n_runs, sequences=n_seq)
    if bai is None:
        try:
            bai = open(path + ".bai", "rb").read()
        except OSError as x:
            raise vm.ViewError("reading BAM index", str(x))
    ref, s, e = vm.parse_query(query, [n.decode("latin-1") for n in names])
    chunks = vm.query_chunks(bai, ref, s, e)
    lo, hi = min(s - 1, lens[ref]), min(e, lens[ref])
    if lo >= hi:
        return b"", dict(records_scanned=None, records_counted=0, runs=0, sequences=0)
    kept = [recs[i] for i in vm.selected(path, ref, s, e, chunks) if counts(recs[i], exclude_flags, min_mapq)]
    t, k = text_of(names[ref], lo, depths(kept, ref, lo, hi))
    return t, dict(records_scanned=None, records_counted=len(kept), runs=k, sequences=1)
