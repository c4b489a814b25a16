"""A restatement of `ngs fastq` (include/ngsq_fastq.h) in plain Python: the FASTQ text of a BAM file.

It reads the file itself (tests/sam_model.read_bam: zlib and its own BGZF walk) and walks the records as
sam_model.record_line does.  Record by record, the header's rules:

* kept iff (flag & exclude) == 0 and (flag & require) == require and l_seq >= 1; a record that passes the flag tests with
  l_seq == 0 is counted as no_sequence, one that fails them as excluded;
* class by the flag: 0x40 without 0x80 is a read one, 0x80 without 0x40 a read two, anything else an other; in one-file mode
  every kept record goes to the first output, in two-file mode ones, twos and others go to the first, second and third, and
  others are dropped and counted when there is no third;
* four lines "@<name>[/1|/2]\\n<SEQ>\\n+\\n<QUAL>\\n": the name without its NUL; with the suffix, /1 behind a read one's name and
  /2 behind a read two's; SEQ through =ACMGRSVTWYHKDBN, with flag 0x10 reversed and every code's four bits reversed; QUAL + 33,
  with flag 0x10 reversed; a QUAL whose first byte is 0xFF is l_seq copies of default_quality + 33;
* a kept record with a present score above 93 is the error "writing FASTQ record: record <i>: quality score above 93", the
  smallest such index; records that are not kept are not checked;
* max_records: only the first max_records records of the file are examined (None: all).

Nothing here calls the library."""
from __future__ import annotations

import struct
from typing import Dict, Optional, Tuple, Union

import numpy as np

from tests import sam_model as sm

SEQ_CODES = b"=ACMGRSVTWYHKDBN"
COMPLEMENT = [int(f"{c:04b}"[::-1], 2) for c in range(16)]       # a code's four bits reversed
_LETTERS = np.frombuffer(SEQ_CODES, np.uint8)
_COMPLEMENT = np.array(COMPLEMENT, np.uint8)
ONE, TWO, OTHER = 0, 1, 2
COUNT_KEYS = ("records_scanned", "excluded", "no_sequence", "reads_one", "reads_two", "reads_other", "dropped_other")


def error_message(index: int) -> str:
    return f"writing FASTQ record: record {index}: quality score above 93"


def record_class(flag: int) -> int:
    return ONE if (flag & 0xC0) == 0x40 else TWO if (flag & 0xC0) == 0x80 else OTHER


def record_text(name: bytes, flag: int, codes, qual: bytes, *, suffix: bool, default_quality: int) -> Optional[bytes]:
    """The four lines of a kept record: name without its NUL, codes the l_seq 4-bit codes, qual the l_seq QUAL bytes.  None:
    a present score above 93."""
    codes, q = np.asarray(codes, np.uint8), np.frombuffer(bytes(qual), np.uint8)
    if flag & 0x10:
        codes = _COMPLEMENT[codes[::-1]]
    if q[0] == 0xFF:
        text_q = bytes([default_quality + 33]) * len(codes)
    else:
        if q.max() > 93:
            return None
        text_q = ((q[::-1] if flag & 0x10 else q) + np.uint8(33)).tobytes()
    cls = record_class(flag)
    tail = (b"/1" if cls == ONE else b"/2") if suffix and cls != OTHER else b""
    return b"@" + name + tail + b"\n" + _LETTERS[codes].tobytes() + b"\n+\n" + text_q + b"\n"


def expected_fastq(path: str, *, two_files: bool, other: bool = False, exclude: int = 2304, require: int = 0, suffix: bool = False,
                   default_quality: int = 1, max_records: Optional[int] = None) -> Union[Tuple[bytes, bytes, bytes, Dict[str, int]], str]:
    """(bytes_one, bytes_two, bytes_other, counts) of `ngs fastq`, or the error message.  other: two-file mode has a third
    output (--other)."""
    assert two_files or not other
    _text, _names, s, p = sm.read_bam(path)
    out = [[], [], []]
    counts = dict.fromkeys(COUNT_KEYS, 0)
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
        name = s[body + 32:body + 32 + l_rn - 1]
        seq_at = body + 32 + l_rn + 4 * n_op
        qual_at = seq_at + (l_seq + 1) // 2
        packed = np.frombuffer(s, np.uint8, qual_at - seq_at, seq_at)
        codes = np.stack([packed >> 4, packed & 15], axis=1).reshape(-1)[:l_seq]      # high nibble first
        text = record_text(name, flag, codes, s[qual_at:qual_at + l_seq], suffix=suffix, default_quality=default_quality)
        if text is None:
            return error_message(index)
        cls = record_class(flag)
        counts[("reads_one", "reads_two", "reads_other")[cls]] += 1
        if not two_files:
            out[ONE].append(text)
        elif cls == OTHER and not other:
            counts["dropped_other"] += 1
        else:
            out[cls].append(text)
    return b"".join(out[0]), b"".join(out[1]), b"".join(out[2]), counts
