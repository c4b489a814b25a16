"""`ngs convert --gzip device --sort coordinate <SAM> <BAM>` restated in Python, on top of
tests/bam_text_model.py: the key of a record, the order (ascending keys, ties in input order), the header text of the sorted
file, and the decompressed stream.  Nothing here calls the library."""
import struct
from typing import List

from tests import bam_text_model as tm

NEW_HD = b"@HD\tVN:1.6\tSO:coordinate\n"


def key(rec: bytes) -> int:
    """hi = 0xFFFFFFFF for a record without a sequence or without a position, else refID; lo = pos + 1."""
    ref_id, pos = struct.unpack_from("<ii", rec, 4)
    hi = 0xFFFFFFFF if ref_id < 0 or pos < 0 else ref_id
    return hi << 32 | ((pos + 1) & 0xFFFFFFFF)


def order(keys: List[int]) -> List[int]:
    """perm[i] = the input index of the i-th key in ascending order; equal keys keep input order."""
    return sorted(range(len(keys)), key=lambda i: (keys[i], i))


def sorted_header(header: bytes) -> bytes:
    """The first SO: field of the @HD line becomes SO:coordinate (appended when there is none), its SS: fields of another order
    go, and a header without an @HD line gets one in front.  The @HD line is the one `ngs index` reads: the text's first
    line when it starts with @HD, else the first later line that does."""
    if header.startswith(b"@HD"):
        beg = 0
    else:
        at = header.find(b"\n@HD")
        if at < 0:
            return NEW_HD + header
        beg = at + 1
    eol = header.find(b"\n", beg)
    if eol < 0:
        eol = len(header)
    fields = header[beg:eol].split(b"\t")
    out, has_so = [fields[0]], False
    for f in fields[1:]:
        if f.startswith(b"SO:") and not has_so:
            out.append(b"SO:coordinate")
            has_so = True
        elif f.startswith(b"SS:") and not f[3:].startswith(b"coordinate:"):
            continue
        else:
            out.append(f)
    if not has_so:
        out.append(b"SO:coordinate")
    return header[:beg] + b"\t".join(out) + header[eol:]


def sorted_records(sam: bytes, max_records: int = 0) -> List[bytes]:
    """The first max_records records of the text (0: all), sorted.  Raises tm.TextError for the lowest faulty record."""
    recs = tm.bam_records(sam, max_records)
    return [recs[i] for i in order([key(r) for r in recs])]


def sorted_lines(sam: bytes, max_records: int = 0) -> List[bytes]:
    """The record lines of the text in the order of sorted_records."""
    lines = tm.body_lines(tm.split_header(sam)[1])
    recs = tm.bam_records(sam, max_records)
    return [lines[i] for i in order([key(r) for r in recs])]


def bam_stream(sam: bytes, max_records: int = 0) -> bytes:
    """The decompressed stream of the sorted file.  Raises tm.HeaderError, tm.TextError."""
    header, _body = tm.split_header(sam)
    refs = tm.references(header)
    return tm.header_stream(sorted_header(header), refs) + b"".join(sorted_records(sam, max_records))
