"""A restatement of `ngs markdup` (include/ngsq_markdup.h) in plain Python, one record at a time, with
dictionaries keyed by name and by end tuples.  It deliberately packs nothing, hashes no name and sorts no keys, so that it
shares no shape with the device path:

* candidate: none of 0x4, 0x100, 0x800 and refID >= 0 and pos >= 0; nothing else is ever marked;
* end (ref, u, s): s = flag & 0x10; forward u = pos - leading S/H run; reverse u = pos + reference length of M D N = X - 1 +
  trailing S/H run; zero operations: u = pos; u outside [-2^30, 2^31 - 2^30): the message of the smallest index;
* score: the sum of the QUAL bytes >= 15 modulo 2^32, 0 with QUAL missing (first byte 0xFF);
* pair candidate: 0x1, not 0x8, exactly one of 0x40 and 0x80; a name with exactly one read one and one read two among its pair
  candidates is a pair, every other candidate a fragment;
* pairs of the same two ends (in ascending order): the largest score sum (modulo 2^32) survives, ties to the smaller index of
  the earlier record; both records of the others are duplicates;
* candidates of one end: if a pair member has it every fragment there is a duplicate, otherwise all fragments but the one of
  the largest score (ties to the smaller index);
* output: the header (text without NUL padding, reference list) and every record, 0x400 cleared, then set on the duplicates, or
  with remove the duplicates left out.

Nothing here calls the library."""
from __future__ import annotations

import struct
from typing import Dict, List, Optional, Tuple, Union

from tests import sam_model as sm

METRIC_KEYS = ("records", "candidates", "pairs", "fragments", "duplicate_pairs", "duplicate_fragments", "duplicate_records", "cleared", "ambiguous")
U_MIN, U_END = -(1 << 30), (1 << 31) - (1 << 30)


def error_message(index: int) -> str:
    return f"reading BAM record: record {index} (0-based): unclipped end outside what markdup can hold"


def unclipped_end(pos: int, reverse: bool, ops: List[Tuple[int, int]]) -> int:
    """ops: (length, code) with the codes of "MIDNSHP=X"."""
    if not ops:
        return pos
    if not reverse:
        u = pos
        for length, code in ops:
            if code not in (4, 5):
                break
            u -= length
        return u
    u = pos - 1
    for length, code in ops:
        if code in (0, 2, 3, 7, 8):
            u += length
    for length, code in reversed(ops):
        if code not in (4, 5):
            break
        u += length
    return u


def parse_records(path: str, max_records: Optional[int]):
    """(header bytes, [record dict])."""
    text, _names, s, p = sm.read_bam(path)
    stripped = text.rstrip(b"\0")
    head = s[:4] + struct.pack("<i", len(stripped)) + stripped + s[8 + len(text):p]
    recs = []
    while p < len(s) and (max_records is None or len(recs) < max_records):
        bs, ref, pos, l_rn, _mapq, _bin, n_op, flag, l_seq = struct.unpack_from("<IiiBBHHHI", s, p)
        body = p + 4
        name = bytes(s[body + 32:body + 32 + l_rn - 1])
        ops = [(v >> 4, v & 15) for v in struct.unpack_from(f"<{n_op}I", s, body + 32 + l_rn)]
        qual_at = body + 32 + l_rn + 4 * n_op + (l_seq + 1) // 2
        qual = s[qual_at:qual_at + l_seq]
        recs.append(dict(raw=bytes(s[p:body + bs]), ref=ref, pos=pos, flag=flag, name=name, ops=ops, qual=qual))
        p = body + bs
    return bytes(head), recs


def expected_markdup(path: str, *, remove: bool = False, max_records: Optional[int] = None) -> Union[Tuple[bytes, Dict[str, object]], str]:
    """(the decompressed bytes of the output, the metrics) of `ngs markdup`, or the error message."""
    head, recs = parse_records(path, max_records)
    end: Dict[int, Tuple[int, int, int]] = {}
    score: Dict[int, int] = {}
    names: Dict[bytes, Tuple[list, list]] = {}
    cleared = 0
    for i, r in enumerate(recs):
        f = r["flag"]
        cleared += 1 if f & 0x400 else 0
        if f & 0x904 or r["ref"] < 0 or r["pos"] < 0:
            continue
        u = unclipped_end(r["pos"], bool(f & 0x10), r["ops"])
        if not U_MIN <= u < U_END:
            return error_message(i)
        end[i] = (r["ref"], u, f & 0x10)
        q = r["qual"]
        score[i] = 0 if (len(q) and q[0] == 0xFF) else sum(b for b in q if b >= 15) & 0xFFFFFFFF
        if f & 0x1 and not f & 0x8 and (f & 0xC0) in (0x40, 0x80):
            names.setdefault(r["name"], ([], []))[0 if f & 0x40 else 1].append(i)
    mate: Dict[int, int] = {}
    ambiguous = 0
    for ones, twos in names.values():
        if len(ones) == 1 and len(twos) == 1:
            mate[ones[0]], mate[twos[0]] = twos[0], ones[0]
        elif len(ones) > 1 or len(twos) > 1:
            ambiguous += len(ones) + len(twos)
    dup = set()
    # pairs: the best of every two-end group stays
    groups: Dict[tuple, Tuple[int, int]] = {}                     # key -> (score sum, earlier record) of the best pair so far
    pair_of = lambda a: ((score[a] + score[mate[a]]) & 0xFFFFFFFF, a)
    better = lambda x, y: x[0] > y[0] or (x[0] == y[0] and x[1] < y[1])
    leads = [a for a in mate if a < mate[a]]
    for a in leads:
        key = (min(end[a], end[mate[a]]), max(end[a], end[mate[a]]))
        if key not in groups or better(pair_of(a), groups[key]):
            groups[key] = pair_of(a)
    duplicate_pairs = 0
    for a in leads:
        key = (min(end[a], end[mate[a]]), max(end[a], end[mate[a]]))
        if groups[key][1] != a:
            duplicate_pairs += 1
            dup |= {a, mate[a]}
    # fragments: beside a pair member all go; among themselves the best stays
    has_pair = {end[i] for i in mate}
    best: Dict[tuple, Tuple[int, int]] = {}
    frags = [i for i in end if i not in mate]
    for i in frags:
        if end[i] not in best or better((score[i], i), best[end[i]]):
            best[end[i]] = (score[i], i)
    duplicate_fragments = 0
    for i in frags:
        if end[i] in has_pair or best[end[i]][1] != i:
            duplicate_fragments += 1
            dup.add(i)
    out = [head]
    for i, r in enumerate(recs):
        if i in dup and remove:
            continue
        raw = bytearray(r["raw"])
        raw[19] = (raw[19] & ~0x4 & 0xFF) | (0x4 if i in dup else 0)
        out.append(bytes(raw))
    pairs = len(leads)
    total = len(end)
    metrics = dict(records=len(recs), candidates=total, pairs=pairs, fragments=total - 2 * pairs, duplicate_pairs=duplicate_pairs,
                   duplicate_fragments=duplicate_fragments, duplicate_records=len(dup), cleared=cleared, ambiguous=ambiguous,
                   duplication=(duplicate_fragments + 2 * duplicate_pairs) / total if total else 0.0)
    return b"".join(out), metrics


def metrics_json(m: Dict[str, object], name_collisions: int = 0) -> str:
    """The document `--metrics <FILE>` receives."""
    rows = [f'  "{k}": {m[k]}' for k in METRIC_KEYS] + [f'  "name_collisions": {name_collisions}', f'  "duplication": {m["duplication"]:.6f}']
    return "{\n" + ",\n".join(rows) + "\n}\n"
