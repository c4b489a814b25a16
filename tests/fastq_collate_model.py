"""A restatement of `ngs fastq --collate` (include/ngsq_collate.h) in plain Python, on top of
tests/fastq_model.py: which records are kept, their class and their four lines are that model's; this one groups the kept read
ones and read twos by name in a dict and emits by the header's rules:

* name: the bytes in front of the NUL, compared exactly ("x/1" and "x/2" are two names); others never take part;
* a name with exactly one read one and exactly one read two is a pair; every other kept one or two is a singleton, and
  ambiguous too if its name has more than one one or more than one two;
* pairs in the order of the file index of their earlier record; two-file mode: pair p's one is record p of the first output,
  its two record p of the second; one-file mode: the first output interleaved, one then two;
* singletons, ones and twos together, in file order to the fourth output, or dropped and counted; others in file order to
  the third (two-file mode only), or dropped and counted;
* every kept record, written or dropped, is checked for a present score above 93: the message of the smallest index.

Nothing here calls the library, and nothing here knows of hashes."""
from __future__ import annotations

import struct
from typing import Dict, Optional, Tuple, Union

import numpy as np

from tests import fastq_model as fm
from tests import sam_model as sm

COUNT_KEYS = fm.COUNT_KEYS + ("pairs", "singletons", "ambiguous", "dropped_singletons")


def kept_records(path: str, *, exclude: int, require: int, suffix: bool, default_quality: int, max_records: Optional[int], counts: Dict[str, int]):
    """[(file index, name, class, text or None)] of the kept records, in file order, by fastq_model's rules and functions."""
    _text, _names, s, p = sm.read_bam(path)
    kept = []
    k = 0
    while p < len(s) and (max_records is None or k < max_records):
        bs, _ref, _pos, l_rn, _mapq, _bin, n_op, flag, l_seq = struct.unpack_from("<IiiBBHHHI", s, p)
        body = p + 4
        index, k, p = k, k + 1, body + bs
        counts["records_scanned"] += 1
        if (flag & exclude) != 0 or (flag & require) != require:
            counts["excluded"] += 1
            continue
        if l_seq == 0:
            counts["no_sequence"] += 1
            continue
        name = bytes(s[body + 32:body + 32 + l_rn - 1])
        seq_at = body + 32 + l_rn + 4 * n_op
        qual_at = seq_at + (l_seq + 1) // 2
        packed = np.frombuffer(s, np.uint8, qual_at - seq_at, seq_at)
        codes = np.stack([packed >> 4, packed & 15], axis=1).reshape(-1)[:l_seq]
        text = fm.record_text(name, flag, codes, s[qual_at:qual_at + l_seq], suffix=suffix, default_quality=default_quality)
        cls = fm.record_class(flag)
        counts[("reads_one", "reads_two", "reads_other")[cls]] += 1
        kept.append((index, name, cls, text))
    return kept


def expected_collated(path: str, *, two_files: bool, other: bool = False, singletons: bool = False, exclude: int = 2304, require: int = 0,
                      suffix: bool = False, default_quality: int = 1,
                      max_records: Optional[int] = None) -> Union[Tuple[bytes, bytes, bytes, bytes, Dict[str, int]], str]:
    """(bytes_one, bytes_two, bytes_other, bytes_singletons, counts) of `ngs fastq --collate`, or the error message.  other,
    singletons: that output is given."""
    assert two_files or not other
    counts = dict.fromkeys(COUNT_KEYS, 0)
    kept = kept_records(path, exclude=exclude, require=require, suffix=suffix, default_quality=default_quality, max_records=max_records, counts=counts)
    for index, _name, _cls, text in kept:
        if text is None:
            return fm.error_message(index)
    groups: Dict[bytes, Tuple[list, list]] = {}
    for at, (_index, name, cls, _text) in enumerate(kept):
        if cls != fm.OTHER:
            groups.setdefault(name, ([], []))[cls].append(at)
    pairs = sorted((min(ones[0], twos[0]), ones[0], twos[0]) for ones, twos in groups.values() if len(ones) == 1 and len(twos) == 1)
    paired = {at for _first, a, b in pairs for at in (a, b)}
    out = [[], [], [], []]
    for _first, a, b in pairs:
        out[0].append(kept[a][3])
        out[1 if two_files else 0].append(kept[b][3])
    counts["pairs"] = len(pairs)
    for at, (_index, name, cls, text) in enumerate(kept):
        if cls == fm.OTHER:
            if other:
                out[2].append(text)
            else:
                counts["dropped_other"] += 1
        elif at not in paired:
            counts["singletons"] += 1
            ones, twos = groups[name]
            if len(ones) > 1 or len(twos) > 1:
                counts["ambiguous"] += 1
            if singletons:
                out[3].append(text)
            else:
                counts["dropped_singletons"] += 1
    return b"".join(out[0]), b"".join(out[1]), b"".join(out[2]), b"".join(out[3]), counts
