"""The device FASTA conversion (ngs_amd/csrc/reference_kernels.hip, reference.cpp) held position by position: FASTA texts
built so that a line terminator, a record's end or a thin tile falls exactly on a thread's 16 bytes, on a tile of
T = ngsq_fasta_tile_bytes() bytes, on a round of k_fasta_scan, on a turn of the grid or on an upload piece; a model of what
the loader must make of a text; probe reads that say for every 1-based position whether its code is right.

    case_*(T, ...) -> Case          the text and, in `holds`, the bytes and lengths it was built around (tests/test_reference.py
                                    asserts each of them against offsets computed here and against the library's index)
    record_spans / sequences        the model: where each record's text lies, what its sequence is (parse_fasta)
    probe_batch                     reads of W bases end to end over every sequence, as numpy columns, rows or offsets layout
    run_probes                      file -> QcContext -> edits_positions / error_counts / reference_wait against the model

The judge: a probe's SEQ is exactly the model's codes, its CIGAR is `WM`.  Where the device's codes are the model's, every
position under a probe counts one `ref` and no `alt` (oracle/oracle.c edits_visit: equal codes, all sixteen of them -- the
small cases run the oracle beside the device to hold that); a probe over a byte Base::try_from refuses fails as a whole
(edits_bad_reference) and leaves zeros.  A dropped, doubled or wrong base shows at its own position; with W = 1 the refused
set is located exactly."""
from __future__ import annotations

import re
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ngs_amd import ffi, host
from ngs_amd.host import HostBatch

LETTERS = "=ACMGRSVTWYHKDBN"
CODE_OF = np.full(256, 0xFF, dtype=np.uint8)                             # the letter table, case folded; 0xFF = refused
for _k, _ch in enumerate(LETTERS):
    CODE_OF[ord(_ch)] = CODE_OF[ord(_ch.lower())] = _k
PIECE = 32 << 20                                                         # one upload of reference.cpp (SLOT)
BAD_CAP = 1 << 16                                                        # positions of refused bytes the loader keeps
SCAN_ROUND = 1024                                                        # tiles k_fasta_scan takes before it carries


@dataclass
class Case:
    text: bytes
    holds: dict                                                          # what the text was built around (per case: see its docstring)
    names: Optional[List[str]] = None                                    # the context's sequences (None: every record, file order)
    lens: Optional[List[int]] = None                                     # their @SQ LN (None: the records' own lengths)


def letters(rng, n, alphabet=b"ACGTacgt") -> bytes:
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def masked_letters(rng, n) -> np.ndarray:
    """n letters of ACGT with soft-masked stretches (a uint8 array)"""
    a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
    edges = np.cumsum(rng.integers(5, 4000, n // 2000 + 2))
    for lo, hi in zip(edges[0::2], edges[1::2]):
        a[lo:hi] |= 0x20
    return a


def lines_of_text(seq: np.ndarray, width: int, text_bytes: int) -> bytes:
    """`seq` in lines of `width` letters and '\\n', exactly text_bytes bytes of them: whole lines, then a shorter one (a blank
    one when a single byte is left).  len(seq) must be bases_for_text(text_bytes, width)."""
    full, rem = divmod(text_bytes, width + 1)
    assert len(seq) == full * width + max(rem - 1, 0)
    body = np.full((full, width + 1), 10, dtype=np.uint8)
    body[:, :width] = seq[:full * width].reshape(full, width)
    tail = seq[full * width:].tobytes() + b"\n" if rem else b""
    return body.tobytes() + tail


def bases_for_text(text_bytes: int, width: int) -> int:
    full, rem = divmod(text_bytes, width + 1)
    return full * width + max(rem - 1, 0)


# ---- the model --------------------------------------------------------------------------------------------------------------
def record_spans(text: bytes) -> List[Tuple[str, int, int]]:
    """[(name, text_begin, text_end)] in file order: a record starts at a '>' in the first column; its text is everything
    behind the definition line up to the next such '>' (the bytes ngsq_fasta_record_text_bytes counts)."""
    starts = [m.start() for m in re.finditer(rb"(?m)^>", text)]
    out = []
    for k, s in enumerate(starts):
        end = starts[k + 1] if k + 1 < len(starts) else len(text)
        nl = text.find(b"\n", s, end)
        begin = nl + 1 if nl >= 0 else end
        name = re.split(rb"[ \t\r]", text[s + 1:nl if nl >= 0 else end], maxsplit=1)[0].decode()
        out.append((name, begin, end))
    return out


def sequences(text: bytes) -> Dict[str, bytes]:
    """name -> sequence bytes by tests/test_reference.py parse_fasta (the first record of a name wins)"""
    from tests.test_reference import parse_fasta
    return dict(reversed(parse_fasta(text)))


def tile_bases(rec_text: bytes, T: int) -> List[int]:
    """sequence bytes in each tile of a record's text (only for texts whose '\\r's all stand in front of a '\\n' or of the end)"""
    a = np.frombuffer(rec_text, dtype=np.uint8)
    keep = (a != 10) & (a != 13)
    return [int(keep[k:k + T].sum()) for k in range(0, len(a), T)]


# ---- a. terminators against a thread's 16 bytes ---------------------------------------------------------------------------
TERMINATORS = {"lf": b"\n", "crlf": b"\r\n", "cr": b"\r", "crcrlf": b"\r\r\n"}


def case_thread_phases(T: int) -> Case:
    """One record per (terminator, phase): 16 + phase letters, the terminator -- its first byte at text offset 16 + phase --
    and a second line of 50 letters (so that `ngs generate` finds a fragment of 42 bases behind a kept '\\r').  "cr" is a lone
    '\\r' with a letter behind it (kept, refused); of "\\r\\r\\n" the first '\\r' is kept.  Phase 15 is the thread that has to look
    at the next thread's first byte.
    holds: {record: (terminator, offset of its first byte)}"""
    rng = np.random.default_rng(101)
    out, holds = [], {}
    for tname, term in TERMINATORS.items():
        for ph in range(16):
            name = f"{tname}{ph}"
            out.append(f">{name} phase {ph}\n".encode() + letters(rng, 16 + ph) + term + letters(rng, 50) + b"\n")
            holds[name] = (term, 16 + ph)
    return Case(b"".join(out), holds)


# ---- b. the same against a tile -------------------------------------------------------------------------------------------
LAST_RECORDS = {"none": b"", "cr": b"\r", "lfcr": b"\n\r"}


def case_tile_edges(T: int, ending: str, residue: int) -> Case:
    """Terminators on the tile's edge, texts of exactly T - 1, T, T + 1 and 2 T bytes, and as the file's last record a text
    of length = residue (mod 16) that ends without a newline ("none"), with a lone '\\r' ("cr") or with "\\n\\r" ("lfcr").
    holds: {"bytes": {record: (offset, the bytes there)}, "length": {record: text bytes}, "last": (record, residue, ending)}"""
    rng = np.random.default_rng(202)
    out, at, length = [], {}, {}

    def add(name, body):
        out.append(f">{name}\n".encode() + body)

    add("nl_Tm1", letters(rng, T - 1) + b"\n" + letters(rng, 50) + b"\n")
    at["nl_Tm1"] = (T - 1, b"\n")
    add("nl_T", letters(rng, T) + b"\n" + letters(rng, 50) + b"\n")
    at["nl_T"] = (T, b"\n")
    add("crnl_Tm1", letters(rng, T - 1) + b"\r\n" + letters(rng, 50) + b"\r\n")
    at["crnl_Tm1"] = (T - 1, b"\r\n")
    add("cr_Tm1", letters(rng, T - 1) + b"\r" + letters(rng, 50) + b"\n")
    at["cr_Tm1"] = (T - 1, b"\r")
    add("crcrnl_Tm2", letters(rng, T - 2) + b"\r\r\n" + letters(rng, 50) + b"\n")
    at["crcrnl_Tm2"] = (T - 2, b"\r\r\n")
    for tag, n in (("Tm1", T - 1), ("T", T), ("Tp1", T + 1), ("2T", 2 * T)):
        seq = np.frombuffer(letters(rng, bases_for_text(n, 60)), dtype=np.uint8)
        add("len_" + tag, lines_of_text(seq, 60, n))
        length["len_" + tag] = n
    end = LAST_RECORDS[ending]
    n = 96 + residue                                                     # 96 = 6 threads' bytes
    body = letters(rng, 40) + b"\n" + letters(rng, n - 41 - len(end)) + end
    assert len(body) == n
    add("last", body)
    length["last"] = n
    return Case(b"".join(out), {"bytes": at, "length": length, "last": ("last", residue, end)})


# ---- c. thin tiles --------------------------------------------------------------------------------------------------------
THIN_GROUPS = (1, 2, 3, 5)


def case_thin_tiles(T: int) -> Case:
    """Four records thin0 .. thin3: v + 1 bases in tile 0 (v = 0 .. 3 bases in front of the one), then groups of 1, 2, 3 and 5
    bases in tiles 2, 4, 6 and 8 with nothing but newlines between them (tiles 1, 3, 5, 7, 9 hold no base), then 60 bases in
    tile 10 so that `ngs generate` can draw from the record.  The codes of the group of g bases go to offset v + (bases in
    front), which over the four records takes every alignment mod 4.  "blank_crlf": blank "\\r\\n" lines only, no base.
    holds: {record: bases per tile}"""
    rng = np.random.default_rng(303)
    out, holds = [], {}
    for v in range(4):
        body = bytearray(b"\n" * (10 * T + 62))
        body[0:v + 1] = letters(rng, v + 1)
        per_tile = [v + 1] + [0] * 10
        for k, g in enumerate(THIN_GROUPS):
            tile = 2 * (k + 1)
            off = tile * T + 13 * k + 5                                  # inside the tile, at another thread and byte each time
            body[off:off + g] = letters(rng, g)
            per_tile[tile] = g
        body[10 * T + 1:10 * T + 61] = letters(rng, 60)
        per_tile[10] = 60
        out.append(f">thin{v}\n".encode() + bytes(body))
        holds[f"thin{v}"] = per_tile
    out.append(b">blank_crlf\n" + b"\r\n" * 40)
    holds["blank_crlf"] = [0]
    return Case(b"".join(out), holds)


# ---- d. every byte value --------------------------------------------------------------------------------------------------
def guarded_lines(seq: bytes, width: int) -> bytes:
    """seq in lines of `width` bytes and '\\n' -- a line grows by a byte rather than end in '\\r' or let '>' start the next"""
    out, k = [], 0
    while k < len(seq):
        e = min(k + width, len(seq))
        while e < len(seq) and (seq[e - 1] == 13 or seq[e] == ord(">")):
            e += 1
        out.append(seq[k:e] + b"\n")
        k = e
    return b"".join(out)


def case_every_byte(T: int) -> Case:
    """all_w1, all_w16, all_w61: each of the 255 byte values other than '\\n' once, in ascending order (value v at 0-based
    position v, or v - 1 behind the missing '\\n'), at three line widths; "letters": the sixteen letters in both cases and
    nothing else -- no refused byte, so the record stays on the window lanes.
    holds: {"all": the 255 bytes, "widths": {record: width}, "letters": that record's sequence}"""
    every = bytes(v for v in range(256) if v != 10)
    widths = {"all_w1": 1, "all_w16": 16, "all_w61": 61}
    out = [f">{name}\n".encode() + guarded_lines(every, w) for name, w in widths.items()]
    both = (LETTERS + LETTERS.lower()).encode() * 5
    out.append(b">letters\n" + guarded_lines(both, 61))
    return Case(b"".join(out), {"all": every, "widths": widths, "letters": both})


# ---- e. many records ------------------------------------------------------------------------------------------------------
def case_many_records(T: int) -> Case:
    """3000 records r0 .. r2999 of 0 .. 40 bases, empty ones in runs of up to five (some with no text at all, some with a
    blank line); the context names every second one, shuffled; LN is the record's length but for 40 records with LN below it
    and 40 with LN above it.
    holds: {"records": 3000, "empty_runs": the longest run of records without a base}"""
    rng = np.random.default_rng(505)
    n = 3000
    length = rng.integers(1, 41, n)
    k = 3
    while k < n - 6:                                                     # runs of 1 .. 5 empty records
        run = int(rng.integers(1, 6))
        length[k:k + run] = 0
        k += run + int(rng.integers(1, 40))
    out = []
    for i in range(n):
        L = int(length[i])
        if L == 0:
            body = b"" if rng.random() < 0.5 else (b"\n" if rng.random() < 0.5 else b"\r\n")
        else:
            w = int(rng.choice([7, 60]))
            s = letters(rng, L)
            body = b"".join(s[j:j + w] + b"\n" for j in range(0, L, w))
        out.append(f">r{i} record {i}\n".encode() + body)
    wanted = np.arange(1, n, 2)
    order = rng.permutation(len(wanted))
    names = [f"r{int(wanted[j])}" for j in order]
    lens = [int(length[wanted[j]]) for j in order]
    changed = 0
    for j in range(len(lens)):                                           # 40 with LN below the record's length, 40 above
        if changed < 80 and lens[j] >= 10:
            lens[j] += -5 if changed % 2 == 0 else 7
            changed += 1
    zero = (length == 0).astype(int)
    longest = max(len(r) for r in "".join(map(str, zero)).split("0"))
    return Case(b"".join(out), {"records": n, "empty_runs": longest, "changed": changed}, names, lens)


# ---- f, g. one long record between two small ones -------------------------------------------------------------------------
def case_long_record(text_bytes: int, width: int, seed: int) -> Case:
    """"front" (700 bases), "long" (exactly text_bytes bytes of text in lines of `width` letters, ACGT with soft-masked
    stretches), "back" (700 bases).
    holds: {"record": "long", "text_bytes": text_bytes}"""
    rng = np.random.default_rng(seed)
    small = lambda: lines_of_text(masked_letters(rng, 700), 70, 710)
    long_ = lines_of_text(masked_letters(rng, bases_for_text(text_bytes, width)), width, text_bytes)
    text = b">front\n" + small() + b">long the record under test\n" + long_ + b">back\n" + small()
    return Case(text, {"record": "long", "text_bytes": text_bytes})


def case_scan_rounds(T: int, extra: int = 1) -> Case:
    """f: 1024 T + extra bytes of text, 1025 tiles: k_fasta_scan takes a second round with the first one's carry.  With
    extra = 1 the one byte of tile 1024 is the record's last '\\n' (another record follows, so the text ends with one): the
    second round runs, but no base is stored by its offset.  extra = 100 puts whole lines of bases there."""
    return case_long_record(SCAN_ROUND * T + extra, 60, 606)


def case_two_pieces(T: int) -> Case:
    """g: 33 MiB + 17 bytes of text: two upload pieces, and more tiles than 16 blocks on each of 256 compute units"""
    return case_long_record((33 << 20) + 17, 70, 707)


# ---- h. the refused-bytes list at its capacity ----------------------------------------------------------------------------
def case_refused_capacity(T: int, refused: int) -> Case:
    """One record "cap": `refused` times a base and a '*', 64 bytes a line.
    holds: {"refused": refused}"""
    seq = np.empty(2 * refused, dtype=np.uint8)
    seq[0::2] = np.frombuffer(b"ACGT", dtype=np.uint8)[np.arange(refused) % 4]
    seq[1::2] = ord("*")
    n = len(seq)
    text = b">cap\n" + lines_of_text(seq, 64, n + -(-n // 64))
    return Case(text, {"refused": refused})


# ---- the probes -----------------------------------------------------------------------------------------------------------
def probe_batch(codes: Sequence[np.ndarray], W: int, layout: str = "rows", only: Optional[Sequence[Tuple[int, int]]] = None):
    """Reads of W bases laid end to end over codes[r] (the model's codes of sequence r as far as reads may lie: min(length,
    LN) of them; 0xFF = refused), the last of a sequence shorter; SEQ = the codes (N over a refused byte), CIGAR = <length>M.
    layout "rows": fixed-pitch rows; "offsets": the offsets layout.  only: [(r, 0-based position)] -- one-base probes at
    these places instead.  Returns (HostBatch, ref_id, pos, l_seq, refused: the probe covers a refused byte)."""
    ref_id, pos, l_seq, rows = [], [], [], []
    if only is not None:
        assert W == 1
        for r, p in only:
            ref_id.append(np.array([r]))
            pos.append(np.array([p]))
            l_seq.append(np.array([1]))
            rows.append(codes[r][p:p + 1].reshape(1, 1))
    else:
        for r, c in enumerate(codes):
            if len(c) == 0:
                continue
            start = np.arange(0, len(c), W)
            ref_id.append(np.full(len(start), r))
            pos.append(start)
            l_seq.append(np.minimum(W, len(c) - start))
            padded = np.zeros(len(start) * W, dtype=np.uint8)
            padded[:len(c)] = c
            rows.append(padded.reshape(len(start), W))
    if not rows:
        ref_id, pos, l_seq, rows = [np.zeros(0, int)], [np.zeros(0, int)], [np.zeros(0, int)], [np.zeros((0, W), np.uint8)]
    ref_id, pos, l_seq, m = np.concatenate(ref_id), np.concatenate(pos), np.concatenate(l_seq), np.concatenate(rows)
    n = len(ref_id)
    refused = (m == 0xFF).any(axis=1)
    m = np.where(m == 0xFF, 15, m).astype(np.uint8)
    if W % 2:
        m = np.concatenate([m, np.zeros((n, 1), dtype=np.uint8)], axis=1)
    packed = ((m[:, 0::2] << 4) | m[:, 1::2]).astype(np.uint8)
    sb = packed.shape[1]
    cols = {
        "flag": np.full(n, 0x40, dtype=np.uint16), "mapq": np.full(n, 60, dtype=np.uint8), "ref_id": ref_id.astype(np.int32),
        "pos": pos.astype(np.int32), "mate_ref_id": np.full(n, -1, dtype=np.int32), "tlen": np.zeros(n, dtype=np.int32),
        "l_seq": l_seq.astype(np.uint32), "n_cigar": np.ones(n, dtype=np.uint16),
        "cigar": (l_seq.astype(np.uint32) << 4).astype(np.uint32),
    }
    if layout == "rows":
        cols.update(seq=np.ascontiguousarray(packed.reshape(-1)), qual=np.full(n * W, 30, dtype=np.uint8), seq_off=None, qual_off=None,
                    cigar_off=None)
        hb = HostBatch(n, cols, sb, W, 1, 0)
    else:
        nb = (l_seq + 1) // 2
        cols.update(seq=np.ascontiguousarray(packed[np.arange(sb)[None, :] < nb[:, None]]), qual=np.full(int(l_seq.sum()), 30, dtype=np.uint8),
                    seq_off=np.concatenate([[0], np.cumsum(nb)]).astype(np.uint64),
                    qual_off=np.concatenate([[0], np.cumsum(l_seq)]).astype(np.uint64), cigar_off=np.arange(n + 1, dtype=np.uint64))
        hb = HostBatch(n, cols, 0, 0, 0, 0)
    return hb, ref_id, pos, l_seq, refused


def expected_refs(lens, ref_id, pos, l_seq, refused) -> List[np.ndarray]:
    """refs_per_position of every sequence (LN + 1 entries): 1 under a probe without a refused byte, 0 elsewhere"""
    out = [np.zeros(int(L) + 1, dtype=np.uint32) for L in lens]
    bounds = np.concatenate([[0], np.flatnonzero(np.diff(ref_id)) + 1, [len(ref_id)]]) if len(ref_id) else [0]
    for a, b in zip(bounds[:-1], bounds[1:]):                            # the probes of one sequence
        r = int(ref_id[a])
        if pos[a] == 0 and np.array_equal(pos[a + 1:b], pos[a:b - 1] + l_seq[a:b - 1]):   # end to end from position 1
            out[r][1:1 + int(pos[b - 1] + l_seq[b - 1])] += np.repeat(~refused[a:b], l_seq[a:b]).astype(np.uint32)
        else:
            for i in range(a, b):
                out[r][int(pos[i]) + 1:int(pos[i] + l_seq[i]) + 1] += np.uint32(not refused[i])
    return out


def model_of(case: Case):
    """(names, lens, seqs: the records' sequences, codes: the model's codes as far as a probe may lie, expected stats)"""
    seqs_by_name = sequences(case.text)
    names = case.names if case.names is not None else [nm for nm, _, _ in record_spans(case.text)]
    seqs = [seqs_by_name[nm] for nm in names]
    lens = case.lens if case.lens is not None else [len(s) for s in seqs]
    codes = [CODE_OF[np.frombuffer(s, dtype=np.uint8)][:L] for s, L in zip(seqs, lens)]
    wanted = set(names)
    text_bytes = sum(e - b for nm, b, e in record_spans(case.text) if nm in wanted)
    stats = dict(sequences=len(names), text_bytes=text_bytes, bases=sum(min(len(s), L) for s, L in zip(seqs, lens)),
                 invalid_bytes=sum(int((CODE_OF[np.frombuffer(s, dtype=np.uint8)] == 0xFF).sum()) for s in seqs),
                 shorter=sum(len(s) < L for s, L in zip(seqs, lens)), longer=sum(len(s) > L for s, L in zip(seqs, lens)))
    return names, lens, seqs, codes, stats


def first_mismatch(got, want):
    k = int(np.flatnonzero(got != want)[0])
    return f"position {k}: device {int(got[k])}, model {int(want[k])} ({int((got != want).sum())} positions differ)"


def run_probes(lib, path, case: Case, W: int, layout: str = "rows", fasta_threads: int = 0, oracle_mod=None, only=None, model=None):
    """The file at `path` (case.text) loaded by a QcContext, the probes processed, everything the device reports held to the
    model.  oracle_mod: run the oracle, fed fasta_codes of the parsed text, on the same probes beside it.  Returns the load's
    stats."""
    names, lens, seqs, codes, want_stats = model if model is not None else model_of(case)
    hb, ref_id, pos, l_seq, refused = probe_batch(codes, W, layout, only)
    want_refs = expected_refs(lens, ref_id, pos, l_seq, refused)
    n_bad = int(refused.sum())
    rc_want = ffi.ERR_MALFORMED_RECORD if n_bad else 0
    with host.QcContext(lens, facets=ffi.FACET_EDITS, ref_fasta=path, ref_names=names, fasta_threads=fasta_threads, lib=lib) as gpu:
        st = gpu.reference_wait()
        got_stats = {k: int(st[k]) for k in want_stats}
        assert got_stats == want_stats
        gpu.process_batch(hb)
        assert gpu.finalize(allow_malformed=True) == rc_want
        errs = gpu.error_counts()
        assert errs["edits_bad_reference"] == n_bad and sum(errs.values()) == n_bad, errs
        for r in range(len(lens)):
            refs, alts = gpu.edits_positions(r)
            assert np.array_equal(refs, want_refs[r]), f"{names[r]}: refs, {first_mismatch(refs, want_refs[r])}"
            assert not alts.any(), f"{names[r]}: alts at position {int(np.flatnonzero(alts)[0])}"
        if oracle_mod is not None:
            from tests.util import compare_contexts
            bases = [oracle_mod.fasta_codes(s) if len(s) else np.full(1, 0xFF, dtype=np.uint8) for s in seqs]
            orc = oracle_mod.Oracle(lens, facets=ffi.FACET_EDITS, ref_bases=bases, ref_bases_len=[len(s) for s in seqs])
            orc.process_batch(hb)
            assert orc.finalize(allow_malformed=True) == rc_want
            compare_contexts(gpu, orc, len(lens), ffi.FACET_EDITS, 50_000, lens)
            r1, r2, _ = orc.edits()
            assert int(r1[0]) == hb.n - n_bad and int(r1.sum()) == hb.n - n_bad   # the oracle too: no probe has an edit, for any code
    return st
