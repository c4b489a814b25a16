"""Positions at or above each depth per window or BED interval, `ngs depth --by <N|BED> --thresholds <T[,T...]> <BAM> [QUERY]` as
DESIGN.md section 25 decides it, in plain Python with exact integers: the bytes the command is to write and the counts of its
report.  It sits on top of tests/depth_windows_model.py (the intervals, their order, the mean's text) and of
tests/depth_model.py's depths(), both unchanged.

A line is "<name>\\t<start>\\t<end>\\t<mean>\\t<n_1>\\t...\\t<n_K>\\n": section 24's line of the same interval, then for each of the K
thresholds the number of the interval's positions whose depth is at least T_k.  An interval without a counted record gives "0.00"
and K zeros.  `covered[k]` of the report is the sum of n_k over all lines.

Nothing here calls the library: the tests hold the library's bytes and refusals against this."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests import depth_model as dm
from tests import depth_windows_model as wm
from tests import view_model as vm

MAX = 2 ** 31 - 1
MAX_THRESHOLDS = 8


class ThresholdsError(ValueError):
    """A refused --thresholds value: the message of the command line."""


def _rust_int(t: str, maximum: int) -> int:
    """An unsigned integer as the command's other integers are parsed (Rust's words): an optional '+', decimal digits."""
    if t == "":
        raise ValueError("cannot parse integer from empty string")
    body = t[1:] if t[0] == "+" else t
    if body == "" or any(c not in "0123456789" for c in body):
        raise ValueError("invalid digit found in string")
    if int(body) > maximum:
        raise ValueError("number too large to fit in target type")
    return int(body)


def parse_thresholds(text: str) -> List[int]:
    """The list of a --thresholds value; ThresholdsError with the command line's message (without the "Error: " in front)."""
    opt = "'--thresholds <T,...>'"
    out = []
    for element in text.split(","):
        try:
            v = _rust_int(element, MAX)
        except ValueError as x:
            raise ThresholdsError(f"invalid value '{element}' for {opt}: {x}")
        if v == 0:
            raise ThresholdsError(f"invalid value '0' for {opt}: a threshold must be at least 1")
        out.append(v)
    if len(out) > MAX_THRESHOLDS:
        raise ThresholdsError(f"invalid value '{text}' for {opt}: at most 8 thresholds")
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ThresholdsError(f"invalid value '{text}' for {opt}: thresholds must be strictly ascending")
    return out


def valid(thresholds: Optional[Sequence[int]]) -> bool:
    """What the library accepts: 1 to 8 depths from 1 to 2^31 - 1, strictly ascending."""
    if thresholds is None or not 1 <= len(thresholds) <= MAX_THRESHOLDS:
        return False
    return all(1 <= t <= MAX for t in thresholds) and all(a < b for a, b in zip(thresholds, thresholds[1:]))


def interval_counts(depth: np.ndarray, lo: int, ivs: Sequence[Tuple[int, int]], thresholds: Sequence[int]) -> List[List[int]]:
    """Per interval (start, end) over the depths of positions [lo, lo + len(depth)): its K counts, n_k = the positions whose depth
    is at least thresholds[k]."""
    pre = [np.concatenate([[0], np.cumsum(depth >= t, dtype=np.int64)]) for t in thresholds]   # C_k in front of every position
    return [[int(c[e - lo] - c[s - lo]) for c in pre] for s, e in ivs]


def _lines(name: bytes, lo: int, depth: np.ndarray, ivs: Sequence[Tuple[int, int]], thresholds: Sequence[int]):
    """The lines of the intervals, the sum of their sums, the sums of their counts, and the counts themselves."""
    pre = [0]
    for d in depth.tolist():            # exact Python integers
        pre.append(pre[-1] + d)
    counts = interval_counts(depth, lo, ivs, thresholds)
    out, total = [], 0
    for (s, e), n in zip(ivs, counts):
        t = pre[e - lo] - pre[s - lo]
        total += t
        out.append(b"%s\t%d\t%d\t%s" % (name, s, e, wm.mean_text(t, e - s)) + b"".join(b"\t%d" % c for c in n) + b"\n")
    covered = [sum(n[k] for n in counts) for k in range(len(thresholds))]
    return b"".join(out), total, covered, counts


def expected(path: str, thresholds: Sequence[int], window: int = 0, intervals: Optional[Sequence[Tuple[int, int, int]]] = None,
             query: Optional[str] = None, exclude_flags: int = dm.EXCLUDE_FLAGS, min_mapq: int = 0) -> Tuple[bytes, Dict[str, object]]:
    """The bytes `ngs depth --by ... --thresholds` writes and the counts of its report: those of depth_windows_model.expected
    (records_scanned, records_counted, lines, sequences, depth_sum), `covered` (a list of K totals) and `counts` (the K counts of
    every line, in the order of the lines).  Exactly one of window and intervals; raises as depth_windows_model.expected."""
    assert valid(thresholds)
    assert (window > 0) != (intervals is not None) and not (intervals is not None and query)
    K = len(thresholds)
    names, lens, recs, text = dm.read(path)
    if not dm.sorted_header(text):
        raise dm.DepthError(dm.NOT_SORTED)
    if intervals is not None and not intervals:
        return b"", dict(records_scanned=0, records_counted=0, lines=0, sequences=0, depth_sum=0, covered=[0] * K, counts=[])
    if query is None:
        bad = dm.first_out_of_order(recs)
        if bad is not None:
            raise dm.DepthError(f"reading BAM record: record {bad} (0-based) is out of coordinate order: {dm.NOT_SORTED}")
        kept = [r for r in recs if dm.counts(r, exclude_flags, min_mapq)]
        out, n_lines, n_seq, total, covered, counts = [], 0, 0, 0, [0] * K, []
        for ref, (name, ln) in enumerate(zip(names, lens)):
            ivs = wm.windows(0, ln, window) if window else [(s, e) for r, s, e in intervals if r == ref]
            if not ivs:
                continue
            t, k, c, n = _lines(name, 0, dm.depths(kept, ref, 0, ln), ivs, thresholds)
            out.append(t)
            n_lines += len(ivs)
            n_seq += 1
            total += k
            covered = [a + b for a, b in zip(covered, c)]
            counts += n
        return b"".join(out), dict(records_scanned=len(recs), records_counted=len(kept), lines=n_lines, sequences=n_seq, depth_sum=total,
                                   covered=covered, counts=counts)
    bai = open(path + ".bai", "rb").read()
    ref, s, e = vm.parse_query(query, [n.decode("latin-1") for n in names])
    chunks = vm.query_chunks(bai, ref, s, e)
    lo, hi = min(s - 1, lens[ref]), min(e, lens[ref])
    if lo >= hi:
        return b"", dict(records_scanned=None, records_counted=0, lines=0, sequences=0, depth_sum=0, covered=[0] * K, counts=[])
    kept = [recs[i] for i in vm.selected(path, ref, s, e, chunks) if dm.counts(recs[i], exclude_flags, min_mapq)]
    ivs = wm.windows(lo, hi, window)
    t, k, c, n = _lines(names[ref], lo, dm.depths(kept, ref, lo, hi), ivs, thresholds)
    return t, dict(records_scanned=None, records_counted=len(kept), lines=len(ivs), sequences=1, depth_sum=k, covered=c, counts=n)


def first_columns(text: bytes, K: int) -> bytes:
    """The text with the last K columns of every line cut off: section 24's bytes of the same question."""
    return b"".join(b"\t".join(ln.split(b"\t")[:-K]) + b"\n" for ln in text.splitlines())
