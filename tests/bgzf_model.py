"""BGZF as the SAM/BAM specification (4.1) states it, walked member by member in plain Python: what the device encoder's output
is held against.  Every member's framing is checked (magic, FLG.FEXTRA, XLEN 6, the BC subfield, BSIZE landing exactly on the
next member), its payload is inflated with zlib as raw DEFLATE, and CRC32 and ISIZE are checked here, not by zlib."""
from __future__ import annotations

import struct
import zlib
from dataclasses import dataclass
from typing import List, Tuple

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BLOCK_INPUT = 0xFF00


class BgzfError(ValueError):
    pass


@dataclass
class Block:
    offset: int      # of the member in the stream
    size: int        # bytes of the member (BSIZE + 1)
    payload: int     # bytes of raw DEFLATE
    isize: int
    btype: int       # of the payload's first DEFLATE block: 0 stored, 1 fixed, 2 dynamic
    eof: bool        # the member is the specification's EOF block


def walk(stream: bytes, require_eof: bool = True) -> Tuple[bytes, List[Block]]:
    """(data, blocks) of a BGZF stream; BgzfError names the first thing that is wrong."""
    at, data, blocks = 0, [], []
    while at < len(stream):
        if len(stream) - at < 18:
            raise BgzfError(f"member at {at}: truncated header")
        id1, id2, cm, flg, _mtime, _xfl, _os, xlen = struct.unpack_from("<BBBBIBBH", stream, at)
        if (id1, id2, cm) != (31, 139, 8):
            raise BgzfError(f"member at {at}: bad magic")
        if flg != 4:
            raise BgzfError(f"member at {at}: FLG is {flg}, not FEXTRA alone")
        if xlen != 6:
            raise BgzfError(f"member at {at}: XLEN is {xlen}")
        si1, si2, slen, bsize = struct.unpack_from("<BBHH", stream, at + 12)
        if (si1, si2, slen) != (66, 67, 2):
            raise BgzfError(f"member at {at}: no BC subfield")
        size = bsize + 1
        if size < 18 + 8 or at + size > len(stream):
            raise BgzfError(f"member at {at}: BSIZE {bsize} does not land on a member")
        payload = stream[at + 18:at + size - 8]
        crc, isize = struct.unpack_from("<II", stream, at + size - 8)
        d = zlib.decompressobj(-15)
        try:
            raw = d.decompress(payload)
        except zlib.error as e:
            raise BgzfError(f"member at {at}: {e}") from None
        if not d.eof:
            raise BgzfError(f"member at {at}: the DEFLATE stream does not end inside the payload")
        if d.unused_data:
            raise BgzfError(f"member at {at}: {len(d.unused_data)} payload bytes behind the DEFLATE stream")
        if len(raw) != isize:
            raise BgzfError(f"member at {at}: ISIZE {isize}, {len(raw)} bytes inflated")
        if zlib.crc32(raw) & 0xFFFFFFFF != crc:
            raise BgzfError(f"member at {at}: CRC32 mismatch")
        blocks.append(Block(at, size, len(payload), isize, (payload[0] >> 1) & 3 if payload else -1, stream[at:at + size] == EOF_BLOCK))
        data.append(raw)
        at += size
    if require_eof and (not blocks or not blocks[-1].eof):
        raise BgzfError("no EOF block at the end")
    return b"".join(data), blocks


def member(data: bytes, raw: bytes | None = None, level: int = 6) -> bytes:
    """One BGZF member holding `data`; raw: its DEFLATE payload (default: zlib's at `level`)."""
    if raw is None:
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        raw = co.compress(data) + co.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 18 + len(raw) + 8 - 1) + raw +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def stored_member(data: bytes) -> bytes:
    return member(data, b"\x01" + struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data)


def zlib_size(data: bytes, level: int, strategy: int = zlib.Z_DEFAULT_STRATEGY, block: int = BLOCK_INPUT) -> int:
    """Bytes of the BGZF stream (no EOF block) zlib gives for `data` at the encoder's block size."""
    total = 0
    for i in range(0, len(data), block):
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        total += 26 + len(co.compress(data[i:i + block]) + co.flush())
    return total
