"""Harness-side wrappers over the C ABI (ngs_amd/ffi.py): record batches as numpy
columns, a context object with the reference's facet lifecycle
(process -> finalize -> results), and the synthetic-batch helpers.

Nothing here computes: every number comes out of libngsq.so.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import json
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import ffi

COLUMN_DTYPES = {
    "flag": np.uint16, "mapq": np.uint8, "ref_id": np.int32, "pos": np.int32, "mate_ref_id": np.int32,
    "tlen": np.int32, "l_seq": np.uint32, "n_cigar": np.uint16, "seq": np.uint8, "seq_off": np.uint64,
    "qual": np.uint8, "qual_off": np.uint64, "cigar": np.uint32, "cigar_off": np.uint64,
    "record_id": np.uint64,   # optional (include/ngsq.h): absent -> first_record_index + i
}
FIXED_COLUMNS = ["flag", "mapq", "ref_id", "pos", "mate_ref_id", "tlen", "l_seq", "n_cigar"]


class NgsqError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"ngsq error {code}: {message}")
        self.code = code
        self.message = message


@dataclass
class HostBatch:
    """A batch of records as host numpy columns (see include/ngsq.h ngsq_batch)."""
    n: int
    cols: Dict[str, Optional[np.ndarray]]
    seq_stride: int = 0
    qual_stride: int = 0
    cigar_stride: int = 0
    first_record_index: int = 0

    def struct(self) -> ffi.Batch:
        b = ffi.Batch()
        b.struct_size = C.sizeof(ffi.Batch)
        b.location = ffi.MEM_HOST
        b.n_records = self.n
        b.first_record_index = self.first_record_index
        for name, dt in COLUMN_DTYPES.items():
            a = self.cols.get(name)
            if a is None:
                setattr(b, name, None)
                continue
            assert a.dtype == dt and a.flags["C_CONTIGUOUS"], (name, a.dtype)
            setattr(b, name, a.ctypes.data if a.size else _DUMMY.ctypes.data)
        b.seq_stride, b.qual_stride, b.cigar_stride = self.seq_stride, self.qual_stride, self.cigar_stride
        return b

    def slice(self, lo: int, hi: int) -> "HostBatch":
        """Records [lo, hi) as a new batch (variable-length columns re-based)."""
        cols: Dict[str, Optional[np.ndarray]] = {}
        for name in FIXED_COLUMNS:
            a = self.cols.get(name)
            cols[name] = None if a is None else np.ascontiguousarray(a[lo:hi])
        rid = self.cols.get("record_id")
        cols["record_id"] = None if rid is None else np.ascontiguousarray(rid[lo:hi])
        for data, off, stride in (("seq", "seq_off", self.seq_stride), ("qual", "qual_off", self.qual_stride),
                                  ("cigar", "cigar_off", self.cigar_stride)):
            a, o = self.cols.get(data), self.cols.get(off)
            if a is None:
                cols[data], cols[off] = None, None
            elif o is None:
                cols[data], cols[off] = np.ascontiguousarray(a[lo * stride:hi * stride]), None
            else:
                cols[data] = np.ascontiguousarray(a[int(o[lo]):int(o[hi])])
                cols[off] = np.ascontiguousarray(o[lo:hi + 1] - o[lo])
        return HostBatch(hi - lo, cols, self.seq_stride, self.qual_stride, self.cigar_stride,
                         self.first_record_index + lo)


_DUMMY = np.zeros(16, dtype=np.uint64)


def features_struct(ref_id, name, start, stop, role_name=(0, 1, 2, 3, 4)):
    """ffi.Features over numpy copies of the columns (returned second: keep them alive for the call)."""
    cols = [np.ascontiguousarray(np.asarray(a, dtype=np.uint32)) for a in (ref_id, name, start, stop)]
    f = ffi.Features()
    f.struct_size = C.sizeof(ffi.Features)
    for k in range(5):
        f.role_name[k] = int(role_name[k])
    f.n = len(cols[0])
    f.ref_id, f.name, f.start, f.stop = (c.ctypes.data for c in cols)
    return f, cols


def synth_config(n_total: int, mode: int = ffi.SYNTH_FIXED, read_len: int = 150, min_len: int = 50,
                 max_len: int = 300, ref_len: int = 248_956_422, n_refs: int = 2,
                 seed: int = 0x4E4753, file_style: int = 0, seq_model: int = 0, genome=None, lib=None) -> ffi.SynthConfig:
    """genome: the lengths of the sequences of a GENOME-mode file (include/ngsq_shared.h): the records are spread over them."""
    s = ffi.SynthConfig()
    if genome is not None:
        lib = lib or ffi.load_library()
        glen = np.ascontiguousarray(genome, dtype=np.uint32)
        room = np.zeros(len(glen) + 1, dtype=np.uint64)
        _check(lib.ngsq_synth_genome_room(glen.ctypes.data_as(ffi.u32p), len(glen), room.ctypes.data_as(ffi.u64p)), None, lib)
        s.genome_len, s.genome_room, s.genome_n = glen.ctypes.data_as(ffi.u32p), room.ctypes.data_as(ffi.u64p), len(glen)
        s._keep = (glen, room)   # (the structure holds pointers into them)
    s.file_style, s.seq_model = file_style, seq_model
    s.seed, s.n_total, s.mode, s.read_len = seed, n_total, mode, read_len
    s.min_len, s.max_len, s.ref_len, s.n_refs = min_len, max_len, ref_len, n_refs
    return s


def synth_reference(cfg: ffi.SynthConfig, ref: int, length: int, lib=None) -> np.ndarray:
    """The synthetic reference sequence `ref` (one 4-bit code per byte): what reads of seq_model FROM_REFERENCE are sampled from."""
    lib = lib or ffi.load_library()
    out = np.empty(length, dtype=np.uint8)
    _check(lib.ngsq_synth_fill_reference(C.byref(cfg), ref, out.ctypes.data, length, 0), None, lib)
    return out


def synth_host_batch(cfg: ffi.SynthConfig, first: int, n: int, lib=None) -> HostBatch:
    """Records [first, first+n) of the synthetic file, generated by the library's host loop."""
    lib = lib or ffi.load_library()
    sb, qb, co = C.c_uint64(), C.c_uint64(), C.c_uint64()
    _check(lib.ngsq_synth_sizes(C.byref(cfg), first, n, C.byref(sb), C.byref(qb), C.byref(co)), None, lib)
    cols: Dict[str, Optional[np.ndarray]] = {k: np.zeros(n, dtype=COLUMN_DTYPES[k]) for k in FIXED_COLUMNS}
    cols["seq"] = np.zeros(sb.value, dtype=np.uint8)
    cols["qual"] = np.zeros(qb.value, dtype=np.uint8)
    if cfg.mode == ffi.SYNTH_FIXED:
        cs = 3 if cfg.file_style & ffi.SYNTH_FILE_CIGAR_MIX else 1
        cols["cigar"] = np.zeros(n * cs, dtype=np.uint32)
        cols["seq_off"] = cols["qual_off"] = cols["cigar_off"] = None
        hb = HostBatch(n, cols, (cfg.read_len + 1) // 2, cfg.read_len, cs, first)
    else:
        cols["cigar"] = np.zeros(co.value, dtype=np.uint32)
        for k in ("seq_off", "qual_off", "cigar_off"):
            cols[k] = np.zeros(n + 1, dtype=np.uint64)
        hb = HostBatch(n, cols, 0, 0, 0, first)
    st = hb.struct()
    _check(lib.ngsq_synth_fill_host(C.byref(cfg), first, n, C.byref(st)), None, lib)
    return hb


def _check(rc: int, ctx, lib):
    if rc != ffi.OK:
        msg = (lib.ngsq_last_error(ctx) if ctx else lib.ngsq_last_global_error()) or b""
        raise NgsqError(rc, msg.decode("utf-8", "replace"))


@dataclass
class DeviceBatch:
    """A batch whose columns live in device memory owned by a QcContext."""
    n: int
    ptrs: Dict[str, int]
    seq_stride: int
    qual_stride: int
    cigar_stride: int
    first_record_index: int
    seq_bytes: int
    qual_bytes: int
    cigar_ops: int
    nbytes: int = 0
    max_l_seq: int = 0   # the longest read, when known (include/ngsq.h: the quality table grows to it)

    def struct(self) -> ffi.Batch:
        b = ffi.Batch()
        b.struct_size = C.sizeof(ffi.Batch)
        b.location = ffi.MEM_DEVICE
        b.max_l_seq = self.max_l_seq
        b.n_records = self.n
        b.first_record_index = self.first_record_index
        for name in COLUMN_DTYPES:
            setattr(b, name, self.ptrs.get(name) or None)
        b.seq_stride, b.qual_stride, b.cigar_stride = self.seq_stride, self.qual_stride, self.cigar_stride
        b.seq_bytes, b.qual_bytes, b.cigar_ops = self.seq_bytes, self.qual_bytes, self.cigar_ops
        return b


class QcContext:
    """One `ngs qc` scan on one GPU: create -> process_batch* -> finalize -> results.

    Mirrors the reference driver's lifecycle (src/qc/command.rs:288-418).
    """

    def __init__(self, ref_len: Sequence[int], ref_is_primary: Optional[Sequence[int]] = None,
                 facets: int = ffi.FACETS_DEFAULT, device: int = 0, bin_size: int = 0, tlen_cap: int = 0,
                 cov_cap: int = 0, max_read_len: int = 0, gc_seed: int = 0,
                 ref_bases: Optional[Sequence[Optional[np.ndarray]]] = None, stream: int = 0,
                 timing: bool = False, sorted_input: bool = False, cov_head_guard: int = 0, lib=None,
                 ref_bases_len: Optional[Sequence[int]] = None, ref_fasta: Optional[str] = None,
                 ref_names: Optional[Sequence[str]] = None, ref_wanted: Optional[Sequence[int]] = None, fasta_threads: int = 0):
        """ref_fasta (+ ref_names): the Edits reference from a FASTA FILE (include/ngsq_reference.h) instead of ref_bases."""
        self.lib = lib or ffi.load_library()
        self._ref_len = np.asarray(ref_len, dtype=np.uint32)
        self._primary = np.asarray(ref_is_primary if ref_is_primary is not None else [1] * len(ref_len),
                                   dtype=np.uint8)
        cfg = ffi.Config()
        cfg.struct_size = C.sizeof(ffi.Config)
        cfg.facets, cfg.device, cfg.n_refs = facets, device, len(self._ref_len)
        cfg.ref_len = self._ref_len.ctypes.data_as(ffi.u32p)
        cfg.ref_is_primary = self._primary.ctypes.data_as(ffi.u8p)
        cfg.bin_size, cfg.tlen_cap, cfg.cov_cap, cfg.max_read_len = bin_size, tlen_cap, cov_cap, max_read_len
        cfg.gc_seed = gc_seed
        self._bases_keep = None
        if ref_bases is not None:
            arr = (ffi.u8p * len(self._ref_len))()
            keep = []
            for r, a in enumerate(ref_bases):
                if a is None:
                    arr[r] = None
                else:
                    a = np.ascontiguousarray(a, dtype=np.uint8)
                    # (with ref_bases_len the array may hold the FASTA's whole sequence: only min(its length, LN) bases are read)
                    assert a.size == int(self._ref_len[r]) if ref_bases_len is None else a.size >= min(int(ref_bases_len[r]), int(self._ref_len[r]))
                    keep.append(a)
                    arr[r] = a.ctypes.data_as(ffi.u8p)
            self._bases_keep = (arr, keep)
            cfg.ref_bases = arr
            if ref_bases_len is not None:
                self._bases_len = np.asarray(ref_bases_len, dtype=np.uint32)
                cfg.ref_bases_len = self._bases_len.ctypes.data_as(ffi.u32p)
        self._fasta = None
        if ref_fasta is not None:
            assert ref_bases is None and ref_names is not None and len(ref_names) == len(self._ref_len)
            cfg.ref_bases_deferred = 1
            self._fasta = C.c_void_p()
            if self.lib.ngsq_fasta_open(ref_fasta.encode(), fasta_threads, C.byref(self._fasta)) != 0:
                raise NgsqError(ffi.ERR_INVALID_ARGUMENT, (self.lib.ngsq_fasta_last_error() or b"").decode())
        cfg.stream = stream or None
        cfg.timing = 1 if timing else 0
        cfg.sorted_input = 1 if sorted_input else 0
        cfg.cov_head_guard = cov_head_guard
        self.facets = facets
        self._cfg = cfg
        self._ctx = ffi.ctx_p()
        _check(self.lib.ngsq_create(C.byref(cfg), C.byref(self._ctx)), None, self.lib)
        self._allocs: List[int] = []
        if self._fasta is not None:
            names = (C.c_char_p * len(ref_names))(*[n.encode() for n in ref_names])
            wanted = np.asarray(ref_wanted, dtype=np.uint8) if ref_wanted is not None else None
            _check(self.lib.ngsq_reference_load(self._ctx, self._fasta, names, wanted.ctypes.data_as(ffi.u8p) if wanted is not None else None),
                   self._ctx, self.lib)

    def reference_wait(self) -> Dict[str, float]:
        """Wait for the FASTA load (ngsq_process_batch does so by itself); what it did."""
        _check(self.lib.ngsq_reference_wait(self._ctx), self._ctx, self.lib)
        st = ffi.ReferenceStats()
        _check(self.lib.ngsq_reference_get_stats(self._ctx, C.byref(st)), self._ctx, self.lib)
        return {k: getattr(st, k) for k, _ in ffi.ReferenceStats._fields_ if k != "reserved"}

    # -- lifecycle
    def close(self):
        if self._ctx:
            for p in self._allocs:
                self.lib.ngsq_device_free(self._ctx, p)
            self._allocs = []
            self.lib.ngsq_destroy(self._ctx)   # (waits for a reference load that is still on its way)
            self._ctx = ffi.ctx_p()
            if getattr(self, "_fasta", None) is not None:
                self.lib.ngsq_fasta_close(self._fasta)
                self._fasta = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def process_batch(self, batch, pass_mask: int = ffi.PASS_BOTH):
        st = batch.struct()
        _check(self.lib.ngsq_process_batch(self._ctx, C.byref(st), pass_mask), self._ctx, self.lib)

    def finalize(self, allow_malformed: bool = False) -> int:
        rc = self.lib.ngsq_finalize(self._ctx)
        if rc in (ffi.ERR_MALFORMED_RECORD, ffi.ERR_LIMIT) and allow_malformed:
            return rc
        _check(rc, self._ctx, self.lib)
        return rc

    def reset(self):
        _check(self.lib.ngsq_reset(self._ctx), self._ctx, self.lib)

    def synchronize(self):
        _check(self.lib.ngsq_synchronize(self._ctx), self._ctx, self.lib)

    @property
    def stream(self) -> int:
        return self.lib.ngsq_stream(self._ctx) or 0

    # -- device memory / batches
    def device_malloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        _check(self.lib.ngsq_device_malloc(self._ctx, nbytes, C.byref(p)), self._ctx, self.lib)
        self._allocs.append(p.value)
        return p.value

    def device_free(self, ptr: int):
        self._allocs.remove(ptr)
        _check(self.lib.ngsq_device_free(self._ctx, ptr), self._ctx, self.lib)

    def upload(self, hb: HostBatch) -> DeviceBatch:
        """Copy a host batch into device memory (test helper; the product path
        for host data is process_batch on the HostBatch itself)."""
        ptrs, total = {}, 0
        for name, a in hb.cols.items():
            if a is None:
                continue
            p = self.device_malloc(max(a.nbytes, 16))
            _check(self.lib.ngsq_memcpy_h2d(self._ctx, p, a.ctypes.data, a.nbytes), self._ctx, self.lib)
            ptrs[name] = p
            total += a.nbytes
        def tot(data, off, stride, itemsize=1):
            a, o = hb.cols.get(data), hb.cols.get(off)
            if a is None:
                return 0
            return int(o[hb.n]) if o is not None else hb.n * stride
        return DeviceBatch(hb.n, ptrs, hb.seq_stride, hb.qual_stride, hb.cigar_stride, hb.first_record_index,
                           tot("seq", "seq_off", hb.seq_stride), tot("qual", "qual_off", hb.qual_stride),
                           tot("cigar", "cigar_off", hb.cigar_stride), total,
                           int(hb.cols["l_seq"].max()) if hb.n and hb.cols.get("l_seq") is not None else 0)

    def synth_device_batch(self, cfg: ffi.SynthConfig, first: int, n: int) -> DeviceBatch:
        """Generate records [first, first+n) of the synthetic file directly in HBM."""
        sb, qb, co = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(self.lib.ngsq_synth_sizes(C.byref(cfg), first, n, C.byref(sb), C.byref(qb), C.byref(co)),
               self._ctx, self.lib)
        sizes = {"flag": 2 * n, "mapq": n, "ref_id": 4 * n, "pos": 4 * n, "mate_ref_id": 4 * n, "tlen": 4 * n,
                 "l_seq": 4 * n, "n_cigar": 2 * n, "seq": sb.value, "qual": qb.value}
        if cfg.mode == ffi.SYNTH_FIXED:
            cs = 3 if cfg.file_style & ffi.SYNTH_FILE_CIGAR_MIX else 1    # (an aligner's CIGAR mix: up to three operations, fixed pitch)
            sizes["cigar"] = 4 * n * cs
            strides = ((cfg.read_len + 1) // 2, cfg.read_len, cs)
        else:
            sizes["cigar"] = 4 * co.value
            for k in ("seq_off", "qual_off", "cigar_off"):
                sizes[k] = 8 * (n + 1)
            strides = (0, 0, 0)
        ptrs = {k: self.device_malloc(v + 64) for k, v in sizes.items()}
        db = DeviceBatch(n, ptrs, strides[0], strides[1], strides[2], first, sb.value, qb.value,
                         co.value if cfg.mode != ffi.SYNTH_FIXED else n * strides[2], sum(sizes.values()))
        st = db.struct()
        _check(self.lib.ngsq_synth_fill_device(self._ctx, C.byref(cfg), first, n, C.byref(st)), self._ctx,
               self.lib)
        return db

    def download_column(self, db: DeviceBatch, name: str, count: int) -> np.ndarray:
        out = np.zeros(count, dtype=COLUMN_DTYPES[name])
        _check(self.lib.ngsq_memcpy_d2h(self._ctx, out.ctypes.data, db.ptrs[name], out.nbytes), self._ctx,
               self.lib)
        return out

    def free_batch(self, db: DeviceBatch):
        for p in db.ptrs.values():
            self.device_free(p)
        db.ptrs = {}

    # -- results
    def set_features(self, ref_id, name, start, stop, role_name=(0, 1, 2, 3, 4)):
        """Gene model of the Genomic Features facet: intervals (sequence index, name id, GFF start, GFF end)."""
        f, keep = features_struct(ref_id, name, start, stop, role_name)
        _check(self.lib.ngsq_set_features(self._ctx, C.byref(f)), self._ctx, self.lib)
        del keep

    def features(self) -> Dict[str, int]:
        m = ffi.FeaturesMetrics()
        _check(self.lib.ngsq_get_features(self._ctx, C.byref(m)), self._ctx, self.lib)
        return {k: int(getattr(m, k)) for k in ffi.FEATURES_FIELDS}

    def error_counts(self) -> Dict[str, int]:
        e = ffi.ErrorCounts()
        _check(self.lib.ngsq_get_error_counts(self._ctx, C.byref(e)), self._ctx, self.lib)
        return {k: int(getattr(e, k)) for k in ffi.ERROR_FIELDS}

    def general(self) -> Dict[str, object]:
        g = ffi.GeneralMetrics()
        _check(self.lib.ngsq_get_general(self._ctx, C.byref(g)), self._ctx, self.lib)
        d: Dict[str, object] = {k: int(getattr(g, k)) for k in ffi.GENERAL_FIELDS}
        d["read_one_cigar_ops"] = [int(x) for x in g.read_one_cigar_ops]
        d["read_two_cigar_ops"] = [int(x) for x in g.read_two_cigar_ops]
        return d

    def template_length(self):
        nb = self.lib.ngsq_tlen_bins(self._ctx)
        h = np.zeros(nb, dtype=np.uint64)
        p, i = C.c_uint64(), C.c_uint64()
        _check(self.lib.ngsq_get_template_length(self._ctx, h.ctypes.data_as(ffi.u64p), nb, C.byref(p),
                                                 C.byref(i)), self._ctx, self.lib)
        return h, int(p.value), int(i.value)

    def gc_content(self) -> Dict[str, object]:
        g = ffi.GcMetrics()
        _check(self.lib.ngsq_get_gc_content(self._ctx, C.byref(g)), self._ctx, self.lib)
        d: Dict[str, object] = {"histogram": np.array(list(g.histogram), dtype=np.uint64)}
        for k in ("total_gc_count", "total_at_count", "total_other_count", "processed", "ignored_flags",
                  "ignored_too_short"):
            d[k] = int(getattr(g, k))
        return d

    def quality_scores(self) -> np.ndarray:
        rows = self.lib.ngsq_max_read_len(self._ctx)
        q = np.zeros((rows, ffi.MAX_SCORE + 1), dtype=np.uint64)
        _check(self.lib.ngsq_get_quality_scores(self._ctx, q.ctypes.data_as(ffi.u64p), rows), self._ctx,
               self.lib)
        return q

    def coverage_sequence(self, ref: int):
        nh = self.lib.ngsq_cov_bins(self._ctx)
        nb = int(self.lib.ngsq_coverage_n_bins(self._ctx, ref))
        h = np.zeros(nh, dtype=np.uint64)
        bins = np.zeros(nb, dtype=np.uint64)
        seen, ign = C.c_int(), C.c_uint64()
        _check(self.lib.ngsq_get_coverage_sequence(self._ctx, ref, C.byref(seen), h.ctypes.data_as(ffi.u64p),
                                                   nh, C.byref(ign), bins.ctypes.data_as(ffi.u64p), nb),
               self._ctx, self.lib)
        return bool(seen.value), h, int(ign.value), bins

    def coverage_nonsensical(self) -> int:
        v = C.c_uint64()
        _check(self.lib.ngsq_get_coverage_nonsensical(self._ctx, C.byref(v)), self._ctx, self.lib)
        return int(v.value)

    def edits(self):
        r1 = np.zeros(ffi.EDITS_BINS, dtype=np.uint64)
        r2 = np.zeros(ffi.EDITS_BINS, dtype=np.uint64)
        vaf = np.zeros(ffi.VAF_BINS, dtype=np.uint64)
        _check(self.lib.ngsq_get_edits(self._ctx, r1.ctypes.data_as(ffi.u64p), r2.ctypes.data_as(ffi.u64p),
                                       ffi.EDITS_BINS, vaf.ctypes.data_as(ffi.u64p), ffi.VAF_BINS),
               self._ctx, self.lib)
        return r1, r2, vaf

    def edits_positions(self, ref: int):
        """refs_per_position / alts_per_position of one sequence (edits.rs:322-324), ref_len + 1 entries each."""
        n = int(self._ref_len[ref]) + 1
        refs, alts = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        _check(self.lib.ngsq_get_edits_positions(self._ctx, ref, refs.ctypes.data, alts.ctypes.data, n), self._ctx, self.lib)
        return refs, alts

    def results_json(self, ref_names: Sequence[str]) -> str:
        if len(ref_names) < len(self._ref_len):   # (the C entry point reads n_refs names: it cannot know how many it was given)
            raise ValueError(f"{len(ref_names)} names for a context of {len(self._ref_len)} sequences")
        names = (C.c_char_p * max(1, len(ref_names)))(*[n.encode() for n in ref_names])
        need = self.lib.ngsq_results_json(self._ctx, names, None, 0)
        if need < 0:
            _check(int(need), self._ctx, self.lib)
        buf = C.create_string_buffer(int(need) + 1)
        self.lib.ngsq_results_json(self._ctx, names, buf, int(need) + 1)
        return buf.value.decode()

    def results(self, ref_names: Sequence[str]) -> dict:
        return json.loads(self.results_json(ref_names))

    # -- measurement
    def kernel_timing(self) -> Dict[str, Dict[str, float]]:
        out = {}
        for i in range(self.lib.ngsq_kernel_timing_count(self._ctx)):
            kt = ffi.KernelTime()
            _check(self.lib.ngsq_kernel_timing(self._ctx, i, C.byref(kt)), self._ctx, self.lib)
            out[kt.name.decode()] = {"launches": int(kt.launches), "total_ms": float(kt.total_ms),
                                     "algo_bytes": int(kt.algo_bytes)}
        return out

    def kernel_timing_reset(self):
        _check(self.lib.ngsq_kernel_timing_reset(self._ctx), self._ctx, self.lib)

    # -- shard exchange
    def state_block(self, which: int):
        """(device pointer, element count, numpy dtype) of state block 0=counters 1=depth 2=edits 3=teardown
        4=chunk flags (sorted_input contexts)."""
        p, n = C.c_void_p(), C.c_uint64()
        fn = [self.lib.ngsq_state_counters, self.lib.ngsq_state_depth, self.lib.ngsq_state_edits,
              self.lib.ngsq_state_teardown, self.lib.ngsq_state_chunk_flags][which]
        _check(fn(self._ctx, C.byref(p), C.byref(n)), self._ctx, self.lib)
        return (p.value or 0), int(n.value), (np.uint64 if which in (0, 3) else np.uint8 if which == 4 else np.uint32)

    def depth_layout(self):
        """(n_diff, n_chunks, touched_lo, touched_hi): see ngsq_depth_layout."""
        v = [C.c_uint64() for _ in range(4)]
        _check(self.lib.ngsq_depth_layout(self._ctx, *[C.byref(x) for x in v]), self._ctx, self.lib)
        return tuple(int(x.value) for x in v)

    def set_scan_range(self, chunk_lo: int, chunk_hi: int, carry_in: int):
        _check(self.lib.ngsq_set_scan_range(self._ctx, chunk_lo, chunk_hi, carry_in & 0xFFFFFFFF), self._ctx, self.lib)

    def teardown(self):
        _check(self.lib.ngsq_teardown(self._ctx), self._ctx, self.lib)

    def state_download(self, which: int) -> np.ndarray:
        _, n, dt = self.state_block(which)
        a = np.zeros(n, dtype=dt)
        _check(self.lib.ngsq_state_download(self._ctx, which, a.ctypes.data, a.nbytes), self._ctx, self.lib)
        return a

    def state_upload(self, which: int, a: np.ndarray):
        a = np.ascontiguousarray(a)
        _check(self.lib.ngsq_state_upload(self._ctx, which, a.ctypes.data, a.nbytes), self._ctx, self.lib)


@contextlib.contextmanager
def _reader_and_plain_context(lib, path: str, device: int, open_context: str = ""):
    """(reader, context) for the commands that walk a file through the device ingest without any QC facet: the BAM opened, a
    context for its @SQ lengths on GPU `device`; both released on the way out.  open_context: prefix of the open failure."""
    bam = C.c_void_p()
    rc = lib.ngsq_bam_open(path.encode(), 0, C.byref(bam))
    if rc != ffi.OK:
        raise NgsqError(rc, open_context + (lib.ngsq_bam_last_error() or b"").decode("utf-8", "replace"))
    try:
        n_refs = lib.ngsq_bam_n_refs(bam)
        lens = np.array([lib.ngsq_bam_ref_len(bam, r) for r in range(n_refs)], dtype=np.uint32)
        cfg = ffi.Config()
        cfg.struct_size = C.sizeof(ffi.Config)
        cfg.facets, cfg.device, cfg.n_refs = 0, device, n_refs
        cfg.ref_len = lens.ctypes.data_as(ffi.u32p)
        ctx = ffi.ctx_p()
        _check(lib.ngsq_create(C.byref(cfg), C.byref(ctx)), None, lib)
        try:
            yield bam, ctx
        finally:
            lib.ngsq_destroy(ctx)
    finally:
        lib.ngsq_bam_close(bam)


def _check_bam(rc: int, lib):
    if rc != ffi.OK:
        raise NgsqError(rc, (lib.ngsq_bam_last_error() or b"").decode("utf-8", "replace"))


def build_bam_index(path: str, device: int = 0, bai_path: Optional[str] = None, lib=None) -> Dict[str, float]:
    """`ngs index` in process (include/ngsq_index.h): write the BAI of the coordinate-sorted BAM `path` to bai_path
    (default "<path>.bai"), built on GPU `device` from the device ingest.  Returns the report; NgsqError on any refusal."""
    lib = lib or ffi.load_library()
    with _reader_and_plain_context(lib, path, device) as (bam, ctx):
        rep = ffi.IndexReport()
        _check_bam(lib.ngsq_bam_build_index(bam, ctx, (bai_path or path + ".bai").encode(), C.byref(rep)), lib)
        return {k: getattr(rep, k) for k, _ in ffi.IndexReport._fields_}


def bam_to_sam(path: str, out_path: str, device: int = 0, max_records: int = 0, batch_records: int = 0, lib=None) -> Dict[str, float]:
    """`ngs convert <BAM> <SAM>` in process (include/ngsq_sam.h): the SAM text of `path` written to out_path (created or
    truncated), formatted on GPU `device` from the device ingest.  max_records: at most this many records (0: all; the
    command line maps `-n N` to max(N, 1)); batch_records: records per ingest batch (0: the library's default).  Returns the
    report; NgsqError on an open failure or a record without SAM text."""
    lib = lib or ffi.load_library()
    with _reader_and_plain_context(lib, path, device, "opening BAM input file: ") as (bam, ctx):
        fd = os.open(out_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
        try:
            rep = ffi.SamReport()
            _check_bam(lib.ngsq_bam_write_sam(bam, ctx, fd, max_records, batch_records, C.byref(rep)), lib)
            return {k: getattr(rep, k) for k, _ in ffi.SamReport._fields_}
        finally:
            os.close(fd)


def bam_to_fastq(path: str, path_one: str, path_two: Optional[str] = None, path_other: Optional[str] = None, device: int = 0,
                 exclude_flags: int = ffi.FASTQ_EXCLUDE_FLAGS, require_flags: int = 0, name_suffix: bool = False,
                 default_quality: int = ffi.FASTQ_DEFAULT_QUALITY, bgzf_mask: int = 0, max_records: int = 0, batch_records: int = 0,
                 effort: str = "normal", lib=None) -> Dict[str, object]:
    """`ngs fastq` in process (include/ngsq_fastq.h): the reads of the BAM `path` written as FASTQ to path_one (created or
    truncated), or split by the flag into path_one, path_two and path_other (None with path_two: others are dropped), formatted
    on GPU `device` from the device ingest.  bgzf_mask: bit 0 / 1 / 2: that output is BGZF from the device encoder at `effort`.
    max_records: examine only that many records (0: all); batch_records: records per ingest batch (0: the library's default).
    Returns the report, its three-entry arrays as lists; NgsqError on an open failure, a refused argument or a kept record with
    a quality score above 93."""
    lib = lib or ffi.load_library()
    with _reader_and_plain_context(lib, path, device, "opening BAM input file: ") as (bam, ctx):
        _set_effort(lib, ctx, effort)
        fds = []
        try:
            for p in (path_one, path_two, path_other):
                fds.append(-1 if p is None else os.open(p, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666))
            opt = ffi.FastqOptions()
            opt.struct_size = C.sizeof(ffi.FastqOptions)
            opt.require_flags, opt.exclude_flags, opt.default_quality = require_flags, exclude_flags, default_quality
            opt.name_suffix, opt.bgzf_mask, opt.max_records, opt.batch_records = int(name_suffix), bgzf_mask, max_records, batch_records
            rep = ffi.FastqReport()
            _check_bam(lib.ngsq_bam_write_fastq(bam, ctx, fds[0], fds[1], fds[2], C.byref(opt), C.byref(rep)), lib)
            return {k: (list(getattr(rep, k)) if k in ("text_bytes", "compressed_bytes") else getattr(rep, k)) for k, _ in ffi.FastqReport._fields_}
        finally:
            for fd in fds:
                if fd >= 0:
                    os.close(fd)


def bam_to_fastq_collated(path: str, path_one: str, path_two: Optional[str] = None, path_other: Optional[str] = None,
                          path_single: Optional[str] = None, device: int = 0, exclude_flags: int = ffi.FASTQ_EXCLUDE_FLAGS,
                          require_flags: int = 0, name_suffix: bool = False, default_quality: int = ffi.FASTQ_DEFAULT_QUALITY,
                          bgzf_mask: int = 0, hash_bits: int = 0, max_records: int = 0, batch_records: int = 0, piece_records: int = 0,
                          memory_budget: int = 0, effort: str = "normal", lib=None) -> Dict[str, object]:
    """`ngs fastq --collate` in process (include/ngsq_collate.h): the reads of the BAM `path` as FASTQ with the mates paired by
    name, whatever the order of the file.  With path_two, pair p's read one is record p of path_one and its read two record p of
    path_two; without it path_one is interleaved.  Singletons go to path_single and others to path_other (with path_two only),
    or are dropped and counted.  bgzf_mask: bit 0 / 1 / 2 / 3: that output is BGZF from the device encoder at `effort`.
    hash_bits, batch_records, piece_records and memory_budget change how the work is cut, never what is written (0: the
    library's defaults).  Returns the report, its four-entry arrays as lists; NgsqError on an open failure, a refused argument,
    a kept record with a quality score above 93, records beyond the budget or a run of names beyond the run limit."""
    lib = lib or ffi.load_library()
    with _reader_and_plain_context(lib, path, device, "opening BAM input file: ") as (bam, ctx):
        _set_effort(lib, ctx, effort)
        fds = []
        try:
            for p in (path_one, path_two, path_other, path_single):
                fds.append(-1 if p is None else os.open(p, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666))
            opt = ffi.CollateOptions()
            opt.struct_size = C.sizeof(ffi.CollateOptions)
            opt.require_flags, opt.exclude_flags, opt.default_quality = require_flags, exclude_flags, default_quality
            opt.name_suffix, opt.bgzf_mask, opt.hash_bits = int(name_suffix), bgzf_mask, hash_bits
            opt.max_records, opt.batch_records, opt.piece_records, opt.memory_budget = max_records, batch_records, piece_records, memory_budget
            rep = ffi.CollateReport()
            _check_bam(lib.ngsq_bam_write_fastq_collated(bam, ctx, fds[0], fds[1], fds[2], fds[3], C.byref(opt), C.byref(rep)), lib)
            return {k: (list(getattr(rep, k)) if k in ("text_bytes", "compressed_bytes") else getattr(rep, k)) for k, _ in ffi.CollateReport._fields_}
        finally:
            for fd in fds:
                if fd >= 0:
                    os.close(fd)


def bam_mark_duplicates(path: str, out_path: str, remove: bool = False, device: int = 0, hash_bits: int = 0, max_records: int = 0,
                        batch_records: int = 0, piece_bytes: int = 0, memory_budget: int = 0, effort: str = "normal", lib=None) -> Dict[str, object]:
    """`ngs markdup` in process (include/ngsq_markdup.h): the records of the BAM `path` written to out_path as BAM with flag 0x400
    set on the duplicates and cleared on every other record, or with `remove` the duplicates left out.  hash_bits, batch_records,
    piece_bytes, memory_budget and effort change how the work is cut and compressed, never the decompressed bytes (0: the
    library's defaults).  out_path is created or truncated.  Returns the report; NgsqError on an open failure, a refused
    argument, an unclipped end that cannot be packed, records beyond the budget or a run of names beyond the run limit."""
    lib = lib or ffi.load_library()
    with _reader_and_plain_context(lib, path, device, "opening BAM input file: ") as (bam, ctx):
        _set_effort(lib, ctx, effort)
        fd = os.open(out_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
        try:
            opt = ffi.MarkdupOptions()
            opt.struct_size = C.sizeof(ffi.MarkdupOptions)
            opt.remove, opt.hash_bits, opt.max_records = int(remove), hash_bits, max_records
            opt.batch_records, opt.piece_bytes, opt.memory_budget = batch_records, piece_bytes, memory_budget
            rep = ffi.MarkdupReport()
            _check_bam(lib.ngsq_bam_mark_duplicates(bam, ctx, fd, C.byref(opt), C.byref(rep)), lib)
            return {k: getattr(rep, k) for k, _ in ffi.MarkdupReport._fields_}
        finally:
            os.close(fd)


BGZF_EFFORTS = {"normal": ffi.BGZF_EFFORT_NORMAL, "high": ffi.BGZF_EFFORT_HIGH}


def _set_effort(lib, ctx, effort: str):
    """`--gzip-effort` for every encoder launch of ctx (ngsq_bgzf_set_effort): "normal" or "high"."""
    if effort not in BGZF_EFFORTS:
        raise ValueError(f"effort {effort!r}: one of {sorted(BGZF_EFFORTS)}")
    _check(lib.ngsq_bgzf_set_effort(ctx, BGZF_EFFORTS[effort]), ctx, lib)


def sam_to_bam(path: str, out_path: str, device: int = 0, max_records: int = 0, chunk_bytes: int = 0, lib=None,
               effort: str = "normal") -> Dict[str, float]:
    """`ngs convert --gzip device <SAM> <BAM>` in process (include/ngsq_samtext.h): the BAM of the SAM text at `path` written to
    out_path (created or truncated), the lines parsed and the BGZF blocks written on GPU `device`.  max_records: at most this
    many records (0: all; the command line maps `-n N` to max(N, 1)); chunk_bytes: text bytes per chunk (0: the library's
    default); effort: `--gzip-effort`.  Returns the report; NgsqError on an open failure, a refused header or a line without a
    record."""
    lib = lib or ffi.load_library()
    why = C.create_string_buffer(1024)
    rc = lib.ngsq_sam_check_header(path.encode(), None, why, len(why))   # (before any GPU work, and before out_path exists)
    if rc != ffi.OK:
        raise NgsqError(rc, why.value.decode("utf-8", "replace"))
    cfg = ffi.Config()
    cfg.struct_size = C.sizeof(ffi.Config)
    cfg.facets, cfg.device, cfg.n_refs = 0, device, 0
    ctx = ffi.ctx_p()
    _check(lib.ngsq_create(C.byref(cfg), C.byref(ctx)), None, lib)
    try:
        _set_effort(lib, ctx, effort)
        fd = os.open(out_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
        try:
            rep = ffi.SamTextReport()
            _check(lib.ngsq_sam_write_bam(ctx, path.encode(), fd, max_records, chunk_bytes, C.byref(rep)), ctx, lib)
            return {k: getattr(rep, k) for k, _ in ffi.SamTextReport._fields_}
        finally:
            os.close(fd)
    finally:
        lib.ngsq_destroy(ctx)


def _index_report(rep, lib) -> Dict[str, float]:
    """The index report of an indexed sort, with the device times of its three steps (ngsq_sort_index_split)."""
    out = {k: getattr(rep, k) for k, _ in ffi.IndexReport._fields_}
    ms = [C.c_double(0), C.c_double(0), C.c_double(0)]
    lib.ngsq_sort_index_split(*[C.byref(m) for m in ms])
    out["pass_ms"], out["blocks_ms"], out["translate_ms"] = (m.value for m in ms)
    return out


def sam_to_sorted_bam(path: str, out_path: str, device: int = 0, max_records: int = 0, chunk_bytes: int = 0, piece_bytes: int = 0,
                      max_resident_bytes: int = 0, lib=None, bai_path: Optional[str] = None, index_tile_records: int = 0,
                      effort: str = "normal"):
    """`ngs convert --gzip device --sort coordinate <SAM> <BAM>` in process (include/ngsq_samtext.h, ngsq_sam_write_sorted_bam): as
    sam_to_bam, the records in coordinate order, unplaced ones last.  piece_bytes: sorted record bytes gathered and compressed at
    a time; max_resident_bytes: device memory the records may take (0 each: the library's defaults).  Returns the report.
    bai_path: `--write-index` (ngsq_sam_write_sorted_bam_indexed): the BAI of out_path is written there, index_tile_records sorted
    records per launch of the index pass (0: the library's default); returns (sort report, index report).  effort: `--gzip-effort`."""
    lib = lib or ffi.load_library()
    why = C.create_string_buffer(1024)
    rc = lib.ngsq_sam_check_header(path.encode(), None, why, len(why))   # (before any GPU work, and before out_path exists)
    if rc != ffi.OK:
        raise NgsqError(rc, why.value.decode("utf-8", "replace"))
    cfg = ffi.Config()
    cfg.struct_size = C.sizeof(ffi.Config)
    cfg.facets, cfg.device, cfg.n_refs = 0, device, 0
    ctx = ffi.ctx_p()
    _check(lib.ngsq_create(C.byref(cfg), C.byref(ctx)), None, lib)
    try:
        _set_effort(lib, ctx, effort)
        fd = os.open(out_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
        try:
            rep = ffi.SamSortReport()
            if bai_path is None:
                _check(lib.ngsq_sam_write_sorted_bam(ctx, path.encode(), fd, max_records, chunk_bytes, piece_bytes, max_resident_bytes,
                                                     C.byref(rep)), ctx, lib)
                return {k: getattr(rep, k) for k, _ in ffi.SamSortReport._fields_}
            irep = ffi.IndexReport()
            _check(lib.ngsq_sam_write_sorted_bam_indexed(ctx, path.encode(), fd, max_records, chunk_bytes, piece_bytes, max_resident_bytes,
                                                         C.byref(rep), bai_path.encode(), index_tile_records, C.byref(irep)), ctx, lib)
            return {k: getattr(rep, k) for k, _ in ffi.SamSortReport._fields_}, _index_report(irep, lib)
        finally:
            os.close(fd)
    finally:
        lib.ngsq_destroy(ctx)


def bam_to_sorted_bam(path: str, out_path: str, device: int = 0, max_records: int = 0, batch_records: int = 0, piece_bytes: int = 0,
                      max_resident_bytes: int = 0, lib=None, bai_path: Optional[str] = None, index_tile_records: int = 0,
                      rounds: bool = False, effort: str = "normal"):
    """`ngs convert --gzip device --sort coordinate <BAM> <BAM>` in process (include/ngsq_bamsort.h): the records of the BAM at
    `path`, in any order, written to out_path (created or truncated) in coordinate order, unplaced ones last, inflated, sorted
    and compressed on GPU `device`.  max_records: the first so many records are sorted (0: all; the command line maps `-n N` to
    max(N, 1)); batch_records: records per ingest batch; piece_bytes: sorted record bytes gathered and compressed at a time;
    max_resident_bytes: device memory the records may take (0 each: the library's defaults).  Returns the report; NgsqError on
    an open failure, a file the ingest refuses or records beyond the limits.
    bai_path: `--write-index` (ngsq_bam_write_sorted_bam_indexed): the BAI of out_path is written there, index_tile_records sorted
    records per launch of the index pass (0: the library's default); returns (sort report, index report).
    rounds: ngsq_bam_write_sorted_bam_rounds -- records beyond max_resident_bytes are no refusal: the input is walked again and
    sorted in rounds, to the same bytes; returns (sort report, rounds report), or (sort report, index report, rounds report).
    effort: `--gzip-effort`."""
    lib = lib or ffi.load_library()
    with _reader_and_plain_context(lib, path, device, "opening BAM input file: ") as (bam, ctx):
        _set_effort(lib, ctx, effort)
        fd = os.open(out_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
        try:
            rep = ffi.BamSortReport()
            if rounds:
                irep, rrep = ffi.IndexReport(), ffi.BamSortRounds()
                _check_bam(lib.ngsq_bam_write_sorted_bam_rounds(bam, ctx, fd, max_records, batch_records, piece_bytes, max_resident_bytes,
                                                                C.byref(rep), None if bai_path is None else bai_path.encode(),
                                                                index_tile_records, C.byref(irep), C.byref(rrep)), lib)
                sort_report = {k: getattr(rep, k) for k, _ in ffi.BamSortReport._fields_}
                rounds_report = {k: getattr(rrep, k) for k, _ in ffi.BamSortRounds._fields_}
                if bai_path is None:
                    return sort_report, rounds_report
                return sort_report, _index_report(irep, lib), rounds_report
            if bai_path is None:
                _check_bam(lib.ngsq_bam_write_sorted_bam(bam, ctx, fd, max_records, batch_records, piece_bytes, max_resident_bytes,
                                                         C.byref(rep)), lib)
                return {k: getattr(rep, k) for k, _ in ffi.BamSortReport._fields_}
            irep = ffi.IndexReport()
            _check_bam(lib.ngsq_bam_write_sorted_bam_indexed(bam, ctx, fd, max_records, batch_records, piece_bytes, max_resident_bytes,
                                                             C.byref(rep), bai_path.encode(), index_tile_records, C.byref(irep)), lib)
            return {k: getattr(rep, k) for k, _ in ffi.BamSortReport._fields_}, _index_report(irep, lib)
        finally:
            os.close(fd)


def sam_sorted_header(text: bytes, cap: Optional[int] = None, lib=None) -> bytes:
    """The header text `--sort coordinate` writes for the header text `text` (ngsq_sam_sorted_header, host only).  cap: the
    output buffer's size (default: what the result takes); NgsqError(BUFFER_TOO_SMALL) when it is too small."""
    lib = lib or ffi.load_library()
    text = bytes(text)
    n = C.c_size_t(0)
    if cap is None:
        rc = lib.ngsq_sam_sorted_header(text, len(text), None, 0, C.byref(n))
        cap = n.value
    out = C.create_string_buffer(max(cap, 1))
    rc = lib.ngsq_sam_sorted_header(text, len(text), out, cap, C.byref(n))
    if rc != ffi.OK:
        raise NgsqError(rc, f"header text of {n.value} bytes does not fit {cap}")
    return out.raw[:n.value]


def sort_u64(keys, device: int = 0, lib=None):
    """(perm, report): perm[i] = the index in `keys` (uint64) of the i-th key in ascending order, equal keys in input order --
    the stable radix sort of `--sort coordinate` alone, on GPU `device` (include/ngsq_sort.h: ngsq_sort_u64_device)."""
    lib = lib or ffi.load_library()
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    perm = np.empty(len(keys), np.uint32)
    rep = ffi.SortReport()
    rc = lib.ngsq_sort_u64_device(device, keys.ctypes.data, len(keys), perm.ctypes.data, C.byref(rep))
    if rc != ffi.OK:
        raise NgsqError(rc, (lib.ngsq_sort_last_error() or b"").decode("utf-8", "replace"))
    return perm, {k: getattr(rep, k) for k, _ in ffi.SortReport._fields_}


def sam_parse_f32(text, lib=None) -> int:
    """The bits of the f32 an `f` value of SAM text reads as (ngsq_sam_parse_f32: the kernels' parser, on the host)."""
    lib = lib or ffi.load_library()
    t = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    bits = C.c_uint32(0)
    rc = lib.ngsq_sam_parse_f32(t, len(t), C.byref(bits))
    if rc != ffi.OK:
        raise NgsqError(rc, f"not an f32 value: {t!r}")
    return bits.value


def bam_query_chunks(path: str, query: str, bai_path: Optional[str] = None, lib=None):
    """The region and the merged chunks of a `ngs view` query (include/ngsq_view.h): (ref_id, start, end, [(begin, end), ...])
    with the 1-based inclusive interval (end = ffi.VIEW_END_MAX for one without an end) and the chunks' virtual offsets, from
    the index bai_path (default "<path>.bai").  Host only.  NgsqError on an empty query, an unknown sequence, a bad index."""
    lib = lib or ffi.load_library()
    bam = C.c_void_p()
    _check_bam(lib.ngsq_bam_open(path.encode(), 1, C.byref(bam)), lib)
    try:
        ref, start, end, n = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        bai = bai_path.encode() if bai_path else None
        _check_bam(lib.ngsq_bam_query_chunks(bam, bai, query.encode(), C.byref(ref), C.byref(start), C.byref(end), None, 0, C.byref(n)), lib)
        chunks = (ffi.ViewChunk * max(n.value, 1))()
        _check_bam(lib.ngsq_bam_query_chunks(bam, bai, query.encode(), None, None, None, chunks, n.value, C.byref(n)), lib)
        return ref.value, start.value, end.value, [(chunks[k].begin, chunks[k].end) for k in range(n.value)]
    finally:
        lib.ngsq_bam_close(bam)


def bam_view(path: str, out_path: str, query: Optional[str] = None, mode: str = "full", device: int = 0, bai_path: Optional[str] = None,
             batch_records: int = 0, coalesce_gap: int = 0, lib=None) -> Dict[str, float]:
    """`ngs view <BAM> [QUERY]` in process (include/ngsq_view.h): the view of `path` written to out_path (created or truncated).
    query None: every record; mode "full" | "header-only" | "records-only" ("header-only" needs no GPU); bai_path: the index of
    a query (default "<path>.bai"); batch_records: records per ingest batch (0: the library's default); coalesce_gap: merged
    chunks nearer than this many compressed bytes share a range walk (0: the default, 1: a walk each).  Returns the report;
    NgsqError on an open failure, a bad query or index, or a selected record without SAM text."""
    lib = lib or ffi.load_library()
    m = ffi.VIEW_MODES[mode]
    q = query.encode() if query is not None else None
    bai = bai_path.encode() if bai_path else None

    def run(bam, ctx):
        fd = os.open(out_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
        try:
            rep = ffi.ViewReport()
            _check_bam(lib.ngsq_bam_view(bam, ctx, fd, q, bai, m, batch_records, coalesce_gap, C.byref(rep)), lib)
            return {k: getattr(rep, k) for k, _ in ffi.ViewReport._fields_}
        finally:
            os.close(fd)

    if m == ffi.VIEW_HEADER_ONLY:
        bam = C.c_void_p()
        rc = lib.ngsq_bam_open(path.encode(), 1, C.byref(bam))
        if rc != ffi.OK:
            raise NgsqError(rc, "opening BAM input file: " + (lib.ngsq_bam_last_error() or b"").decode("utf-8", "replace"))
        try:
            return run(bam, None)
        finally:
            lib.ngsq_bam_close(bam)
    with _reader_and_plain_context(lib, path, device, "opening BAM input file: ") as (bam, ctx):
        return run(bam, ctx)


def depth_tile_positions(requested: int = 0, lib=None) -> int:
    """The tile size `ngs depth` takes a sequence by for a request (include/ngsq_depth.h): 0 asks for the default, anything else
    is rounded up to the kernels' granule.  Pure, needs no GPU."""
    lib = lib or ffi.load_library()
    return int(lib.ngsq_depth_tile_positions(requested))


def bam_depth(path: str, out_path: str, query: Optional[str] = None, exclude_flags: int = ffi.DEPTH_EXCLUDE_FLAGS, min_mapq: int = 0,
              batch_records: int = 0, coalesce_gap: int = 0, tile_positions: int = 0, device: int = 0, bai_path: Optional[str] = None,
              lib=None) -> Dict[str, float]:
    """`ngs depth <BAM> [QUERY]` in process (include/ngsq_depth.h): the per-base depth of the coordinate-sorted BAM `path`, or of
    one region of it, written to out_path (created or truncated) as bedGraph lines, one per run of equal depth.  exclude_flags:
    records with any of these flag bits do not count; min_mapq: nor do records below it.  batch_records / coalesce_gap /
    tile_positions: records per ingest batch, the gap below which a query's chunks share a range walk, positions per tile of
    the run path (0: the library's defaults); the bytes do not depend on them.  bai_path: the index of a query (default
    "<path>.bai").  Returns the report; NgsqError on an open failure, an unsorted file, a bad query or index, a failed write."""
    lib = lib or ffi.load_library()
    q = query.encode() if query is not None else None
    bai = bai_path.encode() if bai_path else None
    with _reader_and_plain_context(lib, path, device) as (bam, ctx):
        fd = os.open(out_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
        try:
            rep = ffi.DepthReport()
            _check_bam(lib.ngsq_bam_depth(bam, ctx, fd, q, bai, exclude_flags, min_mapq, batch_records, coalesce_gap, tile_positions,
                                          C.byref(rep)), lib)
            return {k: getattr(rep, k) for k, _ in ffi.DepthReport._fields_}
        finally:
            os.close(fd)


def _read_bed(lib, bam, bed_path: str) -> List[Tuple[int, int, int]]:
    """ngsq_depth_read_bed on an open reader: (sequence index, start, end) of every interval, in the file's order."""
    iv, n = C.POINTER(ffi.DepthInterval)(), C.c_uint64()
    _check_bam(lib.ngsq_depth_read_bed(bam, bed_path.encode(), C.byref(iv), C.byref(n)), lib)
    try:
        return [(iv[k].ref, iv[k].start, iv[k].end) for k in range(n.value)]
    finally:
        lib.ngsq_depth_free_intervals(iv)


def bam_depth_windows(path: str, out_path: str, window: int = 0, intervals: Optional[Sequence[Tuple[int, int, int]]] = None, bed: Optional[str] = None,
                      query: Optional[str] = None, exclude_flags: int = ffi.DEPTH_EXCLUDE_FLAGS, min_mapq: int = 0, batch_records: int = 0,
                      coalesce_gap: int = 0, tile_positions: int = 0, lines_per_pass: int = 0, device: int = 0, lib=None,
                      thresholds: Optional[Sequence[int]] = None) -> Dict[str, float]:
    """`ngs depth --by <N|BED> [--thresholds T,...] <BAM> [QUERY]` in process (ngsq_bam_depth_windows, include/ngsq_depth.h): the mean depth of the
    coordinate-sorted BAM `path` per window of `window` positions, or per interval -- `intervals` as (sequence index, start, end),
    or the BED file `bed`, read through ngsq_depth_read_bed on the same open reader -- written to out_path (created or
    truncated) as "<name> <start> <end> <mean>" lines, two decimals, rounded half up.  The filters and batch_records /
    coalesce_gap / tile_positions are bam_depth's; lines_per_pass: lines the format pass takes at a time (0: the default); the
    bytes do not depend on any of the four.  thresholds: a list of 1 to 8 strictly ascending depths calls
    ngsq_bam_depth_thresholds instead: every line gains, per depth, the number of the interval's positions at or above it, and
    the report `covered`, a list of their K totals.  Returns the report; NgsqError as bam_depth, and for a BED line that is refused."""
    lib = lib or ffi.load_library()
    q = query.encode() if query is not None else None
    with _reader_and_plain_context(lib, path, device) as (bam, ctx):
        if bed is not None:
            intervals = list(intervals or []) + _read_bed(lib, bam, bed)
        iv = list(intervals or [])
        arr = (ffi.DepthInterval * max(len(iv), 1))(*[ffi.DepthInterval(r, s, e) for r, s, e in iv])
        fd = os.open(out_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
        try:
            if thresholds is not None:
                t = [int(x) for x in thresholds]
                trep = ffi.DepthThresholdsReport()
                _check_bam(lib.ngsq_bam_depth_thresholds(bam, ctx, fd, window, arr if iv else None, len(iv), (C.c_uint32 * max(len(t), 1))(*t), len(t), q, None,
                                                         exclude_flags, min_mapq, batch_records, coalesce_gap, tile_positions, lines_per_pass, C.byref(trep)), lib)
                out = {k: getattr(trep, k) for k, _ in ffi.DepthWindowsReport._fields_}
                out["covered"] = list(trep.covered)[:len(t)]
                return out
            rep = ffi.DepthWindowsReport()
            _check_bam(lib.ngsq_bam_depth_windows(bam, ctx, fd, window, arr if iv else None, len(iv), q, None, exclude_flags, min_mapq, batch_records,
                                                  coalesce_gap, tile_positions, lines_per_pass, C.byref(rep)), lib)
            return {k: getattr(rep, k) for k, _ in ffi.DepthWindowsReport._fields_}
        finally:
            os.close(fd)


def depth_read_bed(path: str, bed_path: str, lib=None) -> List[Tuple[int, int, int]]:
    """The intervals of the BED file bed_path against the reference list of the BAM `path`, in the file's
    order: (sequence index, start, end), 0-based half-open, the end clipped to the sequence (ngsq_depth_read_bed).  Host only;
    NgsqError with the line number for a line that is refused."""
    lib = lib or ffi.load_library()
    bam = C.c_void_p()
    rc = lib.ngsq_bam_open(path.encode(), 1, C.byref(bam))
    if rc != ffi.OK:
        raise NgsqError(rc, (lib.ngsq_bam_last_error() or b"").decode("utf-8", "replace"))
    try:
        return _read_bed(lib, bam, bed_path)
    finally:
        lib.ngsq_bam_close(bam)


def _c_strings(items: Sequence[bytes]):
    """(char **, uint32_t *, n) for byte strings that may be empty or hold any byte; keep the result while they are in use."""
    bufs = [C.create_string_buffer(bytes(x), len(x) + 1) for x in items]
    ptrs = (C.c_char_p * max(len(bufs), 1))(*[C.cast(b, C.c_char_p) for b in bufs])
    lens = (C.c_uint32 * max(len(bufs), 1))(*[len(x) for x in items])
    return ptrs, lens, len(bufs), bufs


def derive_lookup(which: int, query: bytes, lib=None) -> List[str]:
    """The machines whose pattern `query` matches in the instrument table (which = ffi.DERIVE_INSTRUMENTS) or the flowcell
    table (ffi.DERIVE_FLOWCELLS), ascending (include/ngsq_derive.h).  Host only."""
    lib = lib or ffi.load_library()
    need = C.c_size_t()
    lib.ngsq_derive_lookup(which, query, len(query), None, 0, C.byref(need))
    buf = C.create_string_buffer(need.value)
    _check_bam(lib.ngsq_derive_lookup(which, query, len(query), buf, need.value, C.byref(need)), lib)
    return buf.value.decode().split("\n")[:-1]


def derive_predict(instruments: Sequence[bytes], flowcells: Sequence[bytes], lib=None) -> str:
    """The document `ngs derive instrument` prints for these instrument ids and flowcell ids (include/ngsq_derive.h).  Host only."""
    lib = lib or ffi.load_library()
    pi, li, ni, keep_i = _c_strings(instruments)
    pf, lf, nf, keep_f = _c_strings(flowcells)
    need = C.c_size_t()
    lib.ngsq_derive_predict(pi, li, ni, pf, lf, nf, None, 0, C.byref(need))
    buf = C.create_string_buffer(need.value)
    _check_bam(lib.ngsq_derive_predict(pi, li, ni, pf, lf, nf, buf, need.value, C.byref(need)), lib)
    return buf.value.decode()


def derive_instrument(path: str, device: int = 0, max_records: int = 0, batch_records: int = 0, table_slots: int = 0, lib=None):
    """`ngs derive instrument` in process (include/ngsq_derive.h): the read names of `path` scanned on GPU `device` from the
    device ingest.  max_records: examine at most this many records (0: all; the command line maps `-n N` to N + 1);
    batch_records: records per ingest batch (0: the library's default); table_slots: slots of each set's device table (0: the
    default).  Returns (instruments, flowcells, document, report): the two sets as sorted lists of bytes, the parsed
    document, the report.  NgsqError on a name that is not an Illumina name."""
    lib = lib or ffi.load_library()
    with _reader_and_plain_context(lib, path, device) as (bam, ctx):
        names = C.c_void_p()
        rep = ffi.DeriveReport()
        _check_bam(lib.ngsq_bam_derive_instrument(bam, ctx, max_records, batch_records, table_slots, C.byref(names), C.byref(rep)), lib)
        try:
            sets = []
            for which in (ffi.DERIVE_INSTRUMENTS, ffi.DERIVE_FLOWCELLS):
                got = []
                for i in range(lib.ngsq_derive_names_count(names, which)):
                    n = C.c_uint32()
                    p = lib.ngsq_derive_names_get(names, which, i, C.byref(n))
                    got.append(C.string_at(p, n.value) if n.value else b"")
                sets.append(got)
        finally:
            lib.ngsq_derive_names_free(names)
        doc = json.loads(derive_predict(sets[0], sets[1], lib))
        return sets[0], sets[1], doc, {k: getattr(rep, k) for k, _ in ffi.DeriveReport._fields_}


def _check_generate(rc: int, lib):
    if rc != ffi.OK:
        raise NgsqError(rc, (lib.ngsq_generate_last_error() or b"").decode("utf-8", "replace"))


def generate_inner_table(mu: float, sigma: float, lib=None):
    """(lower, table) of the inner distance of N(mu, sigma) (include/ngsq_generate.h: ngsq_generate_inner_table): the integers
    lower .. lower + len(table) - 1 and their cumulative 64-bit thresholds.  Host only.  NgsqError on a refused distribution."""
    lib = lib or ffi.load_library()
    lower, n = C.c_int64(), C.c_uint64()
    err = C.create_string_buffer(512)
    rc = lib.ngsq_generate_inner_table(mu, sigma, C.byref(lower), None, 0, C.byref(n), err, len(err))
    if rc != ffi.OK:
        raise NgsqError(rc, err.value.decode("utf-8", "replace"))
    table = np.zeros(n.value, dtype=np.uint64)
    lib.ngsq_generate_inner_table(mu, sigma, C.byref(lower), table.ctypes.data_as(ffi.u64p), n.value, C.byref(n), err, len(err))
    return lower.value, table


def parse_provider(text: str, lib=None):
    """A provider string PATH:ERROR_FREQ:MU:SIGMA:READ_LENGTH:WEIGHT as (path, error_freq, mu, sigma, read_length, weight)
    (include/ngsq_generate.h: ngsq_generate_parse_provider).  NgsqError carries the reference's message."""
    lib = lib or ffi.load_library()
    raw = text.encode()
    path, err, p = C.create_string_buffer(len(raw) + 1), C.create_string_buffer(1024), ffi.GenerateProvider()
    rc = lib.ngsq_generate_parse_provider(raw, path, len(path), C.byref(p), err, len(err))
    if rc != ffi.OK:
        raise NgsqError(rc, err.value.decode("utf-8", "replace"))
    return path.value.decode(), p.error_freq, p.mu, p.sigma, p.read_length, p.weight


class Generator:
    """`ngs generate` in process (include/ngsq_generate.h).  providers: (path, error_freq, mu, sigma, read_length, weight) each.
    Opening is host only and raises NgsqError on every up-front refusal; write() brings the FASTAs to GPU `device` the first
    time and writes pairs [first_pair, first_pair + n_pairs) to the two paths (created or truncated; append=True adds to them)."""

    def __init__(self, providers, device: int = 0, lib=None, effort: str = "normal"):
        self.lib = lib or ffi.load_library()
        self.device = device
        self.effort = effort  # `--gzip-effort`: what the encoder of a BGZF output runs at
        self._g, self._ctx = C.c_void_p(), None
        self._paths = [str(p[0]).encode() for p in providers]
        arr = (ffi.GenerateProvider * max(len(providers), 1))()
        for k, (_, ef, mu, sigma, rl, wt) in enumerate(providers):
            arr[k].path, arr[k].error_freq, arr[k].mu, arr[k].sigma, arr[k].read_length, arr[k].weight = self._paths[k], ef, mu, sigma, rl, wt
        _check_generate(self.lib.ngsq_generate_open(arr, len(providers), C.byref(self._g)), self.lib)
        self.n_providers = len(providers)

    def sequences(self, p: int = 0):
        """[(name, bases)] of provider p, in file order."""
        return [(self.lib.ngsq_generate_sequence_name(self._g, p, s), self.lib.ngsq_generate_sequence_length(self._g, p, s))
                for s in range(self.lib.ngsq_generate_n_sequences(self._g, p))]

    def reads_for_coverage(self, coverage: int) -> int:
        return self.lib.ngsq_generate_reads_for_coverage(self._g, coverage)

    def load(self):
        if self._ctx is None:
            cfg = ffi.Config()
            cfg.struct_size = C.sizeof(ffi.Config)
            cfg.facets, cfg.device, cfg.n_refs = 0, self.device, 0
            ctx = ffi.ctx_p()
            _check(self.lib.ngsq_create(C.byref(cfg), C.byref(ctx)), None, self.lib)
            self._ctx = ctx
            _set_effort(self.lib, ctx, self.effort)
            _check_generate(self.lib.ngsq_generate_load(self._g, ctx), self.lib)

    def write_fds(self, fd_one: int, fd_two: int, seed: int, n_pairs: int, first_pair: int = 0, batch_pairs: int = 0,
                  bgzf: bool = False, plain: int = 0) -> Dict[str, float]:
        """bgzf: both descriptors receive BGZF compressed on the device (ngsq_generate_write_bgzf; `plain`: ffi.GENERATE_PLAIN_*
        for a file that stays text); the report then also has the compressed bytes per file and the encoder's GPU time."""
        if bgzf:
            if n_pairs:
                self.load()
            zrep = ffi.GenerateBgzfReport()
            _check_generate(self.lib.ngsq_generate_write_bgzf(self._g, fd_one, fd_two, seed, first_pair, n_pairs, batch_pairs, plain,
                                                              C.byref(zrep)), self.lib)
            out = {k: getattr(zrep.text, k) for k, _ in ffi.GenerateReport._fields_}
            out.update({k: getattr(zrep, k) for k, _ in ffi.GenerateBgzfReport._fields_ if k != "text"})
            return out
        self.load()
        rep = ffi.GenerateReport()
        _check_generate(self.lib.ngsq_generate_write(self._g, fd_one, fd_two, seed, first_pair, n_pairs, batch_pairs, C.byref(rep)), self.lib)
        return {k: getattr(rep, k) for k, _ in ffi.GenerateReport._fields_}

    def write(self, path_one: str, path_two: str, seed: int, n_pairs: int, first_pair: int = 0, batch_pairs: int = 0, append: bool = False,
              bgzf: bool = False):
        flags = os.O_WRONLY | os.O_CREAT | (os.O_APPEND if append else os.O_TRUNC)
        fd1 = os.open(path_one, flags, 0o666)
        try:
            fd2 = os.open(path_two, flags, 0o666)
            try:
                return self.write_fds(fd1, fd2, seed, n_pairs, first_pair, batch_pairs, bgzf=bgzf)
            finally:
                os.close(fd2)
        finally:
            os.close(fd1)

    def close(self):
        if self._g:
            self.lib.ngsq_generate_close(self._g)
            self._g = C.c_void_p()
        if self._ctx is not None:
            self.lib.ngsq_destroy(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def generate(providers, path_one: str, path_two: str, seed: int, n_pairs: int, first_pair: int = 0, batch_pairs: int = 0, device: int = 0, lib=None,
             bgzf: bool = False, effort: str = "normal"):
    """One call of `ngs generate` in process: the report of Generator.write.  bgzf: both files are BGZF written on the device, at
    `effort` (`--gzip-effort`)."""
    with Generator(providers, device=device, lib=lib, effort=effort) as g:
        return g.write(path_one, path_two, seed, n_pairs, first_pair, batch_pairs, bgzf=bgzf)


def bgzf_deflate(data, device: int = 0, eof: bool = True, lib=None, effort: str = "normal"):
    """(bytes, report): `data` as BGZF compressed on GPU `device` (include/ngsq_bgzf.h: ngsq_bgzf_deflate_device), blocks of
    ffi.BGZF_BLOCK_INPUT input bytes, the EOF block behind them with eof.  effort: "normal", or "high" for a harder match search
    (ngsq_bgzf_set_effort)."""
    lib = lib or ffi.load_library()
    data = bytes(data)
    flags = ffi.BGZF_EOF if eof else 0
    cfg = ffi.Config()
    cfg.struct_size = C.sizeof(ffi.Config)
    cfg.facets, cfg.device, cfg.n_refs = 0, device, 0
    ctx = ffi.ctx_p()
    _check(lib.ngsq_create(C.byref(cfg), C.byref(ctx)), None, lib)
    try:
        _set_effort(lib, ctx, effort)
        cap = lib.ngsq_bgzf_deflate_bound(len(data), flags)
        out = np.empty(max(cap, 1), np.uint8)
        n = C.c_uint64(0)
        rep = ffi.BgzfDeflateReport()
        _check(lib.ngsq_bgzf_deflate_device(ctx, data, len(data), out.ctypes.data, cap, C.byref(n), flags, C.byref(rep)), ctx, lib)
        return bytes(out[:n.value]), {k: getattr(rep, k) for k, _ in ffi.BgzfDeflateReport._fields_}
    finally:
        lib.ngsq_destroy(ctx)
