"""`ngs convert --gzip device --sort coordinate <BAM> <BAM>` restated in Python, on top of
tests/sort_model.py: the input's decompressed stream split into header text, reference table and records; the header text
rewritten by sort_model.sorted_header; the reference table (n_ref and every entry) as the input's bytes; the records, whole and
unchanged, in the order of sort_model.key and sort_model.order.  Nothing here calls the library."""
import gzip
import struct
from typing import List, Tuple

from tests import sort_model as som


def split(stream: bytes) -> Tuple[bytes, bytes, List[bytes]]:
    """(header text as the file holds it, the bytes from n_ref to the last l_ref, the records with their block_size fields)."""
    assert stream[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", stream, 4)[0]
    text = stream[8:8 + l_text]
    p = table_at = 8 + l_text
    n_ref = struct.unpack_from("<i", stream, p)[0]
    p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", stream, p)[0]
    table = stream[table_at:p]
    recs = []
    while p < len(stream):
        n = 4 + struct.unpack_from("<I", stream, p)[0]
        assert p + n <= len(stream)
        recs.append(stream[p:p + n])
        p += n
    return text, table, recs


def sorted_records(recs: List[bytes]) -> List[bytes]:
    return [recs[i] for i in som.order([som.key(r) for r in recs])]


def stream_of(text: bytes, table: bytes, recs: List[bytes]) -> bytes:
    """The decompressed stream of the sorted file of these parts (text: trailing NULs are no text, as the reader drops them)."""
    text = som.sorted_header(text.rstrip(b"\0"))
    return b"BAM\1" + struct.pack("<i", len(text)) + text + table + b"".join(sorted_records(recs))


def bam_stream(bam_file_bytes: bytes, max_records: int = 0) -> bytes:
    """The decompressed stream of the sorted file made from the first max_records records (0: all) of the BAM file."""
    text, table, recs = split(gzip.decompress(bam_file_bytes))
    return stream_of(text, table, recs[:max_records] if max_records else recs)
