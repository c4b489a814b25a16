"""Test-side model of `ngs derive instrument`: the read names of a BAM by its own BGZF walk, the
name splitting (src/derive/instrument/reads.rs:35-64), the `-n` rule (src/derive/command/instrument.rs:92-97), and the resolve
logic (src/derive/instrument/compute.rs:141-267) restated in Python.  What a query's machines are is not restated: the
model looks a query up in the recorded results of tests/golden/instrument_cases.json and asks `lookup` (the library's own
table, which tests/test_derive.py holds to that fixture) for a query the fixture does not list."""
from __future__ import annotations

import json
import os
import struct
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Set, Tuple

from tests import bai_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INSTRUMENTS, FLOWCELLS = 0, 1
_TABLE_NAMES = {INSTRUMENTS: "instruments", FLOWCELLS: "flowcells"}
_cases: Optional[Dict[int, Dict[str, List[str]]]] = None


def fixture_cases() -> Dict[int, Dict[str, List[str]]]:
    global _cases
    if _cases is None:
        doc = json.load(open(os.path.join(GOLDEN, "instrument_cases.json")))
        _cases = {which: {q: m for q, m in doc["cases"][name]} for which, name in _TABLE_NAMES.items()}
    return _cases


class BadName(Exception):
    """A name that has neither 5 nor 7 segments; .name is the name."""

    def __init__(self, name: bytes):
        super().__init__("Could not parse Illumina-formatted query names for read: " + name.decode("utf-8", "replace"))
        self.name = name


def read_names(path: str) -> List[bytes]:
    """The stored name of every record, without its NUL, in file order."""
    _, s, _ = bai_model.read_blocks(path)
    assert s[:4] == b"BAM\1"
    p = 8 + struct.unpack_from("<i", s, 4)[0]
    n_ref = struct.unpack_from("<i", s, p)[0]
    p += 4
    for _ in range(n_ref):
        p += 4 + struct.unpack_from("<i", s, p)[0] + 4
    names = []
    while p < len(s):
        bs = struct.unpack_from("<I", s, p)[0]
        l_rn = s[p + 12]
        names.append(s[p + 36:p + 36 + max(l_rn - 1, 0)])
        p += 4 + bs
    return names


def examined(names: Sequence[bytes], n: int = 0) -> Sequence[bytes]:
    """The counter is tested behind the record: -n N (N > 0) examines min(records, N + 1) of them; 0: all."""
    return names[:n + 1] if n > 0 else names


def split(name: bytes) -> Tuple[bytes, Optional[bytes]]:
    seg = name.split(b":")
    if len(seg) == 5:
        return seg[0], None
    if len(seg) == 7:
        return seg[0], seg[2]
    raise BadName(name)


def collect(names: Iterable[bytes]) -> Tuple[Set[bytes], Set[bytes], int]:
    """(instrument ids, flowcell ids, names skipped); BadName for the first name that does not split."""
    ins, fcs, skipped = set(), set(), 0
    for name in names:
        if name == b"*":
            skipped += 1
            continue
        i, f = split(name)
        ins.add(i)
        if f is not None:
            fcs.add(f)
    return ins, fcs, skipped


def machines(which: int, query: bytes, lookup: Optional[Callable[[int, bytes], List[str]]] = None) -> Set[str]:
    try:
        return set(fixture_cases()[which][query.decode("ascii")])
    except (KeyError, UnicodeDecodeError):
        if lookup is None:
            raise KeyError(f"{query!r} is not a query of instrument_cases.json and no lookup was given")
        return set(lookup(which, query))


def _detect(which: int, queries: Iterable[bytes], lookup) -> Tuple[Set[str], bool]:
    possible, any_machine = None, False
    for q in queries:
        m = machines(which, q, lookup)
        possible = set(m) if possible is None else possible & m
        any_machine = any_machine or bool(m)
    return possible or set(), any_machine


def predict(instruments: Iterable[bytes], flowcells: Iterable[bytes], lookup=None) -> dict:
    by_iid, iid_any = _detect(INSTRUMENTS, set(instruments), lookup)
    by_fcid, fcid_any = _detect(FLOWCELLS, set(flowcells), lookup)

    def result(succeeded, instruments, confidence, evidence, comment):
        return {"succeeded": succeeded, "instruments": sorted(instruments) if instruments is not None else None,
                "confidence": confidence, "evidence": evidence, "comment": comment}

    if not by_iid and iid_any:
        return result(False, None, "unknown", "instrument id", "multiple instruments were detected in this file via the instrument id")
    if not by_fcid and fcid_any:
        return result(False, None, "unknown", "flowcell id", "multiple instruments were detected in this file via the flowcell id")
    if not by_iid and not by_fcid:
        return result(False, None, "unknown", None, "no matching instruments were found")
    if not by_iid:
        return result(True, by_fcid, "medium" if len(by_fcid) == 1 else "low", "flowcell id", None)
    if not by_fcid:
        return result(True, by_iid, "medium" if len(by_iid) == 1 else "low", "instrument id", None)
    both = by_fcid & by_iid
    if not both:
        return result(False, None, "high", "instrument and flowcell id",
                      "Case needs triaging, results from instrument id and flowcell id are mutually exclusive.")
    return result(True, both, "high", "instrument and flowcell id", None)


def document(result: dict) -> str:
    """serde_json::to_string_pretty of the result, `instruments` ascending."""
    return json.dumps(result, indent=2)


def expected(path: str, n: int = 0, lookup=None) -> Tuple[List[bytes], List[bytes], int, dict]:
    """(instrument ids, flowcell ids, skipped, result) of a file, the sets ascending by bytes; BadName as the command reports it."""
    ins, fcs, skipped = collect(examined(read_names(path), n))
    return sorted(ins), sorted(fcs), skipped, predict(ins, fcs, lookup)
