"""The mean depth per window or BED interval, `ngs depth --by <N|BED> <BAM> [QUERY]` as DESIGN.md section 24 decides it, in plain
Python with exact integers: the bytes the command is to write and the counts of its report.  Of the library, the BED reader
(ngsq_depth_read_bed, include/ngsq_depth.h) is held to read_bed() here; the device path is not part of the build yet.

The depth of a position is tests/depth_model.py's, unchanged.  A line is "<name>\\t<start>\\t<end>\\t<mean>\\n" for one interval:
with a window size N the windows [kN, min((k + 1)N, L)) of every sequence in header order (with a query: aligned to position 0
and clipped to [S - 1, min(E, L))), with a BED file its intervals, sequences in header order and the file's order within one.
The mean is the sum of the interval's depths over its length with two decimals, rounded half up, in integers.

Nothing here calls the library: the tests hold the library's bytes and refusals against this."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests import depth_model as dm
from tests import view_model as vm

MAX = 2 ** 31 - 1


class BedError(ValueError):
    """A refused BED file: the message of the library."""


def mean_text(total: int, length: int) -> bytes:
    """sum / len with exactly two decimals, rounded half up: w = sum // len, r = sum % len, f = (100 r + len // 2) // len, and
    f == 100 carries into w."""
    w, r = divmod(total, length)
    f = (100 * r + length // 2) // length
    if f == 100:
        w, f = w + 1, 0
    return b"%d.%02d" % (w, f)


def _number(t: bytes) -> Optional[int]:
    if not t or any(c not in b"0123456789" for c in t) or int(t) > MAX:
        return None
    return int(t)


def read_bed(data: bytes, names: Sequence[bytes], lens: Sequence[int]) -> List[Tuple[int, int, int]]:
    """(sequence index, start, end) of every interval of a BED file's bytes, in the file's order; BedError as the library says it."""
    index: Dict[bytes, int] = {}
    for r, n in enumerate(names):
        index.setdefault(n, r)
    out = []
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for no, line in enumerate(lines, 1):
        if line.endswith(b"\r"):
            line = line[:-1]
        if not line or line.startswith((b"#", b"track", b"browser")):
            continue
        f = line.split(b"\t")

        def refuse(why: str):
            raise BedError(f"reading BED file: line {no}: {why}")

        if len(f) < 3:
            refuse(f"expected at least 3 tab-separated fields, found {len(f)}")
        start, end = _number(f[1]), _number(f[2])
        if start is None:
            refuse(f"invalid start '{f[1].decode('latin-1')}': expected a decimal number of at most 2147483647")
        if end is None:
            refuse(f"invalid end '{f[2].decode('latin-1')}': expected a decimal number of at most 2147483647")
        if start >= end:
            refuse(f"start {start} is not below end {end}")
        if f[0] not in index:
            refuse(f"sequence '{f[0].decode('latin-1')}' is not in the header")
        r = index[f[0]]
        if start >= lens[r]:
            refuse(f"start {start} lies at or beyond the end of '{f[0].decode('latin-1')}' ({lens[r]} positions)")
        if len(out) >= MAX:
            refuse("more than 2147483647 intervals")
        out.append((r, start, min(end, lens[r])))
    return out


def windows(lo: int, hi: int, n: int) -> List[Tuple[int, int]]:
    """The windows of n positions, aligned to position 0, clipped to [lo, hi)."""
    return [(max(k * n, lo), min((k + 1) * n, hi)) for k in range(lo // n, (hi - 1) // n + 1)] if lo < hi else []


def _lines(name: bytes, lo: int, depth: np.ndarray, ivs: Sequence[Tuple[int, int]]) -> Tuple[bytes, int]:
    """The lines of intervals (start, end) over the depths of positions [lo, lo + len(depth)), and the sum of their sums."""
    pre = [0]
    for d in depth.tolist():            # exact Python integers
        pre.append(pre[-1] + d)
    out, total = [], 0
    for s, e in ivs:
        t = pre[e - lo] - pre[s - lo]
        total += t
        out.append(b"%s\t%d\t%d\t%s\n" % (name, s, e, mean_text(t, e - s)))
    return b"".join(out), total


def expected(path: str, window: int = 0, intervals: Optional[Sequence[Tuple[int, int, int]]] = None, query: Optional[str] = None,
             exclude_flags: int = dm.EXCLUDE_FLAGS, min_mapq: int = 0) -> Tuple[bytes, Dict[str, Optional[int]]]:
    """The bytes `ngs depth --by` writes and the counts of its report: records_scanned (None with a query), records_counted,
    lines, sequences, depth_sum.  Exactly one of window and intervals (as read_bed gives them); raises as depth_model.expected."""
    assert (window > 0) != (intervals is not None) and not (intervals is not None and query)
    names, lens, recs, text = dm.read(path)
    if not dm.sorted_header(text):
        raise dm.DepthError(dm.NOT_SORTED)
    if intervals is not None and not intervals:
        return b"", dict(records_scanned=0, records_counted=0, lines=0, sequences=0, depth_sum=0)
    if query is None:
        bad = dm.first_out_of_order(recs)
        if bad is not None:
            raise dm.DepthError(f"reading BAM record: record {bad} (0-based) is out of coordinate order: {dm.NOT_SORTED}")
        kept = [r for r in recs if dm.counts(r, exclude_flags, min_mapq)]
        out, n_lines, n_seq, total = [], 0, 0, 0
        for ref, (name, ln) in enumerate(zip(names, lens)):
            ivs = windows(0, ln, window) if window else [(s, e) for r, s, e in intervals if r == ref]
            if not ivs:
                continue
            t, k = _lines(name, 0, dm.depths(kept, ref, 0, ln), ivs)
            out.append(t)
            n_lines += len(ivs)
            n_seq += 1
            total += k
        return b"".join(out), dict(records_scanned=len(recs), records_counted=len(kept), lines=n_lines, sequences=n_seq, depth_sum=total)
    bai = open(path + ".bai", "rb").read()
    ref, s, e = vm.parse_query(query, [n.decode("latin-1") for n in names])
    chunks = vm.query_chunks(bai, ref, s, e)
    lo, hi = min(s - 1, lens[ref]), min(e, lens[ref])
    if lo >= hi:
        return b"", dict(records_scanned=None, records_counted=0, lines=0, sequences=0, depth_sum=0)
    kept = [recs[i] for i in vm.selected(path, ref, s, e, chunks) if dm.counts(recs[i], exclude_flags, min_mapq)]
    ivs = windows(lo, hi, window)
    t, k = _lines(names[ref], lo, dm.depths(kept, ref, lo, hi), ivs)
    return t, dict(records_scanned=None, records_counted=len(kept), lines=len(ivs), sequences=1, depth_sum=k)
