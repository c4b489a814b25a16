// bai_kernel.hip -- `ngs index` on the device: one pass over every batch of the device ingest in file
// order, then one launch that finishes the linear index.  bai.cpp drives them and writes the file.  And the same index for
// `ngs convert --sort coordinate --write-index` (section 21): the pass over resident records in sorted order, the file's block
// table and the translation of stream offsets to virtual positions, driven by sort_resident.h.
#include <hip/hip_runtime.h>

#include "aux_cg.h"
#include "bai_kernels.h"
#include "deflate_kernels.h" // DEFLATE_BLOCK_INPUT

namespace ngsq {

namespace {

constexpr uint32_t BT = 256; // threads per block
constexpr uint32_t BAI_UNPLACED_BIN = 4680; // reg2bin(-1, 0) (SAM specification 4.2.1)
constexpr int64_t BAI_MAX_POS = (int64_t)1 << 29; // the BAI's binning scheme ends here (SAM specification 5.3)

__device__ inline uint32_t bai_reg2bin(int64_t beg, int64_t end) { // SAM specification 5.3, end exclusive
    --end;
    if (beg >> 14 == end >> 14) return 4681u + (uint32_t)(beg >> 14);
    if (beg >> 17 == end >> 17) return 585u + (uint32_t)(beg >> 17);
    if (beg >> 20 == end >> 20) return 73u + (uint32_t)(beg >> 20);
    if (beg >> 23 == end >> 23) return 9u + (uint32_t)(beg >> 23);
    if (beg >> 26 == end >> 26) return 1u + (uint32_t)(beg >> 26);
    return 0;
}

struct RecInfo {
    int32_t ref, pos;
    uint32_t bin, w0, w1, placed;
    int64_t end; // pos + max(reference span, 1)
};

// ---- the rules of a record, stated once: k_bai_records applies them to the columns of an ingest
// batch, k_bai_sorted to the resident records of `ngs convert --sort coordinate --write-index` (section 21)

// is this CIGAR word one of M D N = X, the operations that take reference bases
__device__ inline uint32_t bai_ref_len(uint32_t c) {
    const uint32_t op = c & 15u;
    return op == 0 || op == 2 || op == 3 || op == 7 || op == 8 ? c >> 4 : 0;
}

// span: the lengths of the CIGAR's M D N = X operations (a CIGAR without any counts as 1)
__device__ inline RecInfo bai_rec_info(int32_t ref, int32_t pos, uint64_t span) {
    RecInfo r;
    r.ref = ref;
    r.pos = pos;
    r.placed = r.ref >= 0 && r.pos >= 0;
    r.end = (int64_t)r.pos + (int64_t)max(span, (uint64_t)1);
    r.bin = r.placed && r.end <= BAI_MAX_POS ? bai_reg2bin(r.pos, r.end) : BAI_UNPLACED_BIN;
    r.w0 = r.placed ? (uint32_t)(r.pos >> 14) : 0;
    r.w1 = r.placed ? (uint32_t)min((r.end - 1) >> 14, (int64_t)0xFFFFFFFF) : 0;
    return r;
}

// what a record needs of the one in front of it (has = 0: it is the first)
struct RecPrev {
    int32_t ref, pos;
    uint32_t bin, w1, placed, has;
};
__device__ inline RecPrev bai_prev_of(const RecInfo &p) { return RecPrev{p.ref, p.pos, p.bin, p.w1, p.placed, 1u}; }
__device__ inline RecPrev bai_prev_of(const BaiCarry &c) { return RecPrev{c.ref, c.pos, c.bin, c.w1, c.placed, c.has}; }

// Every thread of a block of BT hands in its record (inactive threads a zeroed one) and gets its predecessor: its neighbour's,
// or for thread 0 `front`, the record in front of the block (only thread 0's value is used).
__device__ inline RecPrev bai_exchange(const RecInfo &me, const RecPrev &front) {
    __shared__ int32_t s_ref[BT], s_pos[BT];
    __shared__ uint32_t s_bin[BT], s_w1[BT], s_placed[BT];
    s_ref[threadIdx.x] = me.ref;
    s_pos[threadIdx.x] = me.pos;
    s_bin[threadIdx.x] = me.bin;
    s_w1[threadIdx.x] = me.w1;
    s_placed[threadIdx.x] = me.placed;
    __syncthreads();
    if (!threadIdx.x) return front;
    const uint32_t q = threadIdx.x - 1;
    return RecPrev{s_ref[q], s_pos[q], s_bin[q], s_w1[q], s_placed[q], 1u};
}

// head: the record starts a run of (sequence, bin); bad: it breaks the coordinate order; limit: the BAI cannot hold it;
// lin_w: it is the first record to overlap the windows [from, w1] of its sequence
struct RecRules {
    bool head, bad, limit, lin_w;
    uint32_t from;
};
// the BAI cannot hold this placed record
__device__ inline bool bai_limit(const RecInfo &me, const BaiLinear &L) {
    return (uint32_t)me.ref >= L.n_refs || me.end > BAI_MAX_POS || me.w1 >= L.lin_cap[me.ref];
}
__device__ inline RecRules bai_rec_rules(const RecInfo &me, const RecPrev &p, const BaiLinear &L) {
    RecRules r{false, false, false, false, 0};
    if (me.placed) {
        r.bad = p.has && (!p.placed || me.ref < p.ref || (me.ref == p.ref && me.pos < p.pos));
        r.head = !p.has || !p.placed || me.ref != p.ref || me.bin != p.bin;
        r.from = p.has && p.placed && p.ref == me.ref && p.w1 + 1 > me.w0 ? p.w1 + 1 : me.w0;
        r.limit = bai_limit(me, L);
    } else {
        r.head = !p.has || p.placed;
    }
    r.lin_w = me.placed && !r.limit && r.from <= me.w1;
    return r;
}

// What a record leaves behind (every thread of the wave calls it; act: the thread has a record).  i: its index in the batch
// or tile, rec: in the file, startv: the position behind the record in front of it (read where r.head or r.lin_w), flag: its
// flag word (read where it is placed).
__device__ inline void bai_apply(bool act, const RecInfo &me, const RecRules &r, uint32_t flag, uint64_t i, uint64_t rec, uint64_t startv,
                                 BaiState *__restrict__ st, const BaiLinear &L, uint64_t *__restrict__ run_flag, BaiRun *__restrict__ tmp) {
    if (r.bad) (void)atomicMin(&st->bad_order, (unsigned long long)rec);
    if (r.limit) (void)atomicMin(&st->bad_limit, (unsigned long long)rec);
    if (act) run_flag[i] = r.head ? 1 : 0;
    if (r.head) {
        BaiRun run;
        run.start = startv;
        run.rec = rec;
        run.ref = me.placed ? me.ref : -1;
        run.bin = me.bin;
        tmp[i] = run;
    }
    if (r.lin_w) { // the windows no record in front of this one overlaps (its predecessor covers everything up to p.w1)
        unsigned long long *w = L.lin + L.lin_base[me.ref];
        for (uint32_t k = r.from; k <= me.w1; k++) (void)atomicMin(&w[k], (unsigned long long)startv);
    }
    // placed records with the unmapped flag, per sequence: one atomic per wave and sequence (sorted: one sequence per wave)
    const bool unm = act && me.placed && !r.limit && (flag & 0x4);
    uint64_t mask = __ballot(unm);
    while (mask) {
        const int leader = __ffsll((unsigned long long)mask) - 1;
        const int32_t lref = __shfl(me.ref, leader, 64);
        const uint64_t same = __ballot(unm && me.ref == lref) & mask;
        if ((int)(threadIdx.x & 63) == leader) (void)atomicAdd(&L.unmapped[lref], (unsigned long long)__popcll(same));
        mask &= ~same;
    }
}

__device__ inline BaiCarry bai_carry_of(const RecInfo &me, uint64_t endv) {
    BaiCarry c;
    c.ref = me.ref;
    c.pos = me.pos;
    c.bin = me.bin;
    c.w1 = me.w1;
    c.placed = me.placed;
    c.has = 1;
    c.endv = endv;
    return c;
}

// a record of an ingest batch: its columns
__device__ inline RecInfo bai_info(const ngsq_batch &b, uint64_t i) {
    uint64_t span = 0;
    uint64_t k0, k1;
    if (b.cigar_off) {
        k0 = b.cigar_off[i];
        k1 = b.cigar_off[i + 1];
    } else {
        k0 = i * b.cigar_stride;
        k1 = k0 + min((uint32_t)b.n_cigar[i], b.cigar_stride);
    }
    for (uint64_t k = k0; k < k1; k++) span += bai_ref_len(b.cigar[k]);
    return bai_rec_info(b.ref_id[i], b.pos[i], span);
}

// The virtual position behind the byte in front of view offset e (e > o.carry: in this chunk): inside the byte's block,
// or -- the block's last byte -- the start of the block behind it, empty or not (htslib's reader)
__device__ inline uint64_t bai_pos_after(const BatchOrigin &o, uint64_t e) {
    const uint64_t u = e - o.carry;
    uint32_t lo = 0, hi = o.n_blocks; // the last block with out_off <= u - 1: the one that holds that byte
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (o.blocks[mid].out_off <= u - 1) lo = mid;
        else hi = mid;
    }
    const uint64_t beg = o.blocks[lo].out_off, len = o.blocks[lo].isize;
    if (u >= beg + len) return (lo + 1 < o.n_blocks ? o.coff[lo + 1] : o.next_coff) << 16;
    return o.coff[lo] << 16 | (u - beg);
}

__device__ inline uint32_t ld32u(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

__global__ __launch_bounds__(BT) void k_bai_records(ngsq_batch b, BatchOrigin o, BaiState *__restrict__ st, uint32_t parity, BaiLinear L,
                                                    uint64_t *__restrict__ run_flag, BaiRun *__restrict__ tmp) {
    const uint64_t n = b.n_records;
    const uint64_t i0 = (uint64_t)blockIdx.x * BT, i = i0 + threadIdx.x;
    const bool act = i < n;
    RecInfo me{};
    if (act) me = bai_info(b, i);
    RecPrev front{};
    if (threadIdx.x == 0) front = i0 == 0 ? bai_prev_of(st->carry[parity]) : bai_prev_of(bai_info(b, i0 - 1)); // the record in front of the block
    const RecPrev p = bai_exchange(me, front);
    RecRules r{};
    if (act) r = bai_rec_rules(me, p, L);
    uint64_t startv = 0;
    if (r.head || r.lin_w) startv = i == 0 ? st->carry[parity].endv : bai_pos_after(o, o.rec_off[i]);
    bai_apply(act, me, r, act && me.placed ? b.flag[i] : 0u, i, b.first_record_index + i, startv, st, L, run_flag, tmp);
    if (act && i == n - 1) {
        run_flag[n] = 0;
        const uint64_t at = o.rec_off[i];
        // behind the record's last byte (block_size + 4 bytes)
        st->carry[parity ^ 1u] = bai_carry_of(me, bai_pos_after(o, at + 4 + ld32u(o.raw + at)));
    }
}

// ---- `ngs convert --sort coordinate --write-index`: the resident records in sorted order

// the four bytes at byte offset sh / 8 of the aligned words lo, hi
__device__ inline uint32_t bai_shift(uint32_t lo, uint32_t hi, uint32_t sh) { return __builtin_amdgcn_alignbit(hi, lo, sh); }
// the four bytes at p, any alignment, as two aligned words (a byte load per byte is what the compiler makes of a memcpy here)
__device__ inline uint32_t bai_ld32(const uint8_t *p) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>((uintptr_t)p & ~(uintptr_t)3);
    return bai_shift(w[0], w[1], (uint32_t)((uintptr_t)p & 3u) * 8u);
}
// the sum of bai_ref_len over the n CIGAR words at p, any alignment: one aligned load per word
__device__ inline uint64_t bai_span(const uint8_t *p, uint32_t n) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>((uintptr_t)p & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)((uintptr_t)p & 3u) * 8u;
    uint64_t span = 0;
    uint32_t lo = w[0];
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t hi = w[k + 1];
        span += bai_ref_len(bai_shift(lo, hi, sh));
        lo = hi;
    }
    return span;
}

// The record at p (any byte alignment), read where phase 1 left it or in the ingest's view: block_size, refID, pos, l_read_name | mapq | bin, n_cigar_op | flag,
// l_seq are its first 24 bytes -- seven aligned words, shifted -- then the CIGAR, or the CG:B,I tag's operations behind the
// placeholder (as k_rec_fixed resolves it).  The reads stay inside the record and the slab's slack (SORT_GATHER_SLACK; the
// view's buffer has more behind it).
__device__ inline RecInfo bai_info_at(const uint8_t *p, uint32_t *flag) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>((uintptr_t)p & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)((uintptr_t)p & 3u) * 8u;
    uint32_t a[7];
#pragma unroll
    for (int q = 0; q < 7; q++) a[q] = w[q];
    const uint32_t bs = bai_shift(a[0], a[1], sh), lrn = bai_shift(a[3], a[4], sh) & 0xFFu, nf = bai_shift(a[4], a[5], sh);
    const uint32_t l = bai_shift(a[5], a[6], sh), n_ops = nf & 0xFFFFu;
    *flag = nf >> 16;
    const uint8_t *cig = p + 36 + lrn;
    uint32_t real_ops = n_ops;
    if (n_ops == 2 && l) {
        const uint32_t op0 = bai_ld32(cig), op1 = bai_ld32(cig + 4);
        if (op0 == (l << 4 | 4u) && (op1 & 15u) == 3u) {
            const uint64_t need = 32ull + lrn + 8ull + ((uint64_t)l + 1) / 2 + l;
            uint32_t cnt = 0;
            const uint64_t at = need <= bs ? aux_find_cg(p + 4 + need, p + 4 + bs, &cnt) : 0;
            if (at && cnt >= 2) {
                cig = p + 4 + need + at;
                real_ops = cnt;
            }
        }
    }
    return bai_rec_info((int32_t)bai_shift(a[1], a[2], sh), (int32_t)bai_shift(a[2], a[3], sh), bai_span(cig, real_ops));
}

// record k of the sorted order
__device__ inline RecInfo bai_sorted_info(const BaiSorted &t, uint64_t k, uint32_t *flag) {
    return bai_info_at(reinterpret_cast<const uint8_t *>(t.addr[t.perm[k]]), flag);
}

// The survey of a BAM sorted in rounds: the limit test of bai_rec_rules on every record of a batch, in
// input order, before any record is resident; a record that fails it gets the mark in its survey length.
__global__ __launch_bounds__(BT) void k_bai_survey(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ rec_off, uint64_t n, uint64_t first,
                                                   BaiLinear L, uint32_t mark, uint32_t *__restrict__ len) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (i >= n) return;
    uint32_t flag = 0;
    const RecInfo me = bai_info_at(raw + rec_off[i], &flag);
    if (me.placed && bai_limit(me, L)) len[first + i] |= mark;
}

// One thread per record of the tile [first, first + n) of the sorted order.  A position is the record's offset in the sorted
// stream plus one (0 stays "no record" for k_bai_finish's fill); k_bai_translate makes virtual positions of them.
__global__ __launch_bounds__(BT) void k_bai_sorted(BaiSorted t, BaiState *__restrict__ st, uint32_t parity, BaiLinear L,
                                                   uint64_t *__restrict__ run_flag, BaiRun *__restrict__ tmp) {
    const uint64_t i0 = (uint64_t)blockIdx.x * BT, i = i0 + threadIdx.x;
    const bool act = i < t.n;
    RecInfo me{};
    uint32_t flag = 0, front_flag = 0;
    if (act) me = bai_sorted_info(t, t.first + i, &flag);
    RecPrev front{};
    if (threadIdx.x == 0) front = i0 == 0 ? bai_prev_of(st->carry[parity]) : bai_prev_of(bai_sorted_info(t, t.first + i0 - 1, &front_flag));
    const RecPrev p = bai_exchange(me, front);
    RecRules r{};
    if (act) r = bai_rec_rules(me, p, L);
    uint64_t startv = 0;
    if (r.head || r.lin_w) startv = t.pos0 + t.soff[t.first + i] + 1;
    bai_apply(act, me, r, flag, i, t.rec0 + t.first + i, startv, st, L, run_flag, tmp);
    if (act && i == t.n - 1) {
        run_flag[t.n] = 0;
        st->carry[parity ^ 1u] = bai_carry_of(me, t.pos0 + t.soff[t.first + i + 1] + 1);
    }
}

// the member offsets the encoder left for a job, rebased to the file, appended to the file's block table
__global__ __launch_bounds__(BT) void k_bai_blocks(const uint64_t *__restrict__ off, uint64_t n_blocks, uint64_t base, uint64_t *__restrict__ table) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (i < n_blocks) table[i] = base + off[i];
}

// v - 1 = a byte offset x of the sorted stream -> the virtual position of that byte; 0 stays 0.  x at a block's end is the
// next block's first byte, at a piece's end the next piece's first block, at the stream's end the EOF block (section 12.1).
__device__ inline uint64_t bai_flat_to_virtual(const BaiBlocks &B, uint64_t v) {
    if (!v) return 0;
    const uint64_t x = v - 1;
    if (x >= B.total) return B.eof_coff << 16;
    const uint64_t piece = x / B.piece_bytes, in_piece = x - piece * B.piece_bytes;
    const uint64_t blk = in_piece / DEFLATE_BLOCK_INPUT;
    return B.coff[piece * B.blocks_per_piece + blk] << 16 | (in_piece - blk * DEFLATE_BLOCK_INPUT);
}
__global__ __launch_bounds__(BT) void k_bai_translate(BaiBlocks B, BaiRun *__restrict__ runs, uint64_t n_runs, unsigned long long *__restrict__ lin,
                                                      uint64_t n_win) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (i < n_runs) runs[i].start = bai_flat_to_virtual(B, runs[i].start);
    if (i < n_win) lin[i] = bai_flat_to_virtual(B, lin[i]);
}

__global__ __launch_bounds__(BT) void k_bai_gather(const uint64_t *__restrict__ off, const BaiRun *__restrict__ tmp, uint64_t n,
                                                   BaiRun *__restrict__ runs, uint64_t base, unsigned long long *host_count) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (i >= n) return;
    if (off[i + 1] != off[i]) runs[base + off[i]] = tmp[i];
    if (i == n - 1) host_count[0] = base + off[n];
}

// one block per sequence: the windows in order, a tile of BT at a time; an empty window takes the value of the last window
// in front of it that a record overlaps (0: none)
__global__ __launch_bounds__(BT) void k_bai_finish(BaiLinear L, const BaiState *__restrict__ st, uint32_t parity,
                                                   unsigned long long *host) {
    __shared__ unsigned long long s_val[BT];
    __shared__ int32_t s_wave[BT / 64];
    __shared__ unsigned long long s_carry;
    __shared__ int32_t s_last;
    const uint32_t r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (r == 0 && threadIdx.x == 0) {
        host[0] = st->bad_order;
        host[1] = st->bad_limit;
        host[2] = st->carry[parity].endv;
        host[3] = st->carry[parity].has;
    }
    if (r >= L.n_refs) return; // (a header without sequences: one block for the words above)
    unsigned long long *w = L.lin + L.lin_base[r];
    const uint32_t cap = L.lin_cap[r];
    if (threadIdx.x == 0) {
        s_carry = 0;
        s_last = -1;
    }
    __syncthreads();
    for (uint32_t t0 = 0; t0 < cap; t0 += BT) {
        const uint32_t k = t0 + threadIdx.x;
        const unsigned long long v = k < cap ? w[k] : ~0ull;
        const bool filled = v != ~0ull;
        s_val[threadIdx.x] = v;
        int32_t idx = filled ? (int32_t)threadIdx.x : -1; // inclusive prefix max: the last filled window of the tile so far
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t y = __shfl_up(idx, d, 64);
            if ((int)lane >= d) idx = max(idx, y);
        }
        if (lane == 63) s_wave[wave] = idx;
        __syncthreads();
        for (uint32_t q = 0; q < wave; q++) idx = max(idx, s_wave[q]);
        const unsigned long long out = idx >= 0 ? s_val[idx] : s_carry;
        if (k < cap) w[k] = out;
        __syncthreads();
        if (threadIdx.x == BT - 1) {
            s_carry = out;
            if (idx >= 0 && t0 + (uint32_t)idx < cap) s_last = (int32_t)(t0 + (uint32_t)idx);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        host[BAI_HOST_STATE_WORDS + r] = L.unmapped[r];
        host[BAI_HOST_STATE_WORDS + L.n_refs + r] = (unsigned long long)(s_last + 1);
    }
}

} // namespace

hipError_t launch_bai_records(const ngsq_batch &b, const BatchOrigin &o, BaiState *state, uint32_t parity, const BaiLinear &lin,
                              uint64_t *run_flag, BaiRun *tmp_runs, hipStream_t s) {
    if (!b.n_records) return hipSuccess;
    const uint64_t blocks = (b.n_records + BT - 1) / BT;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bai_records, dim3((uint32_t)blocks), dim3(BT), 0, s, b, o, state, parity, lin, run_flag, tmp_runs);
    return hipGetLastError();
}

hipError_t launch_bai_sorted(const BaiSorted &t, BaiState *state, uint32_t parity, const BaiLinear &lin, uint64_t *run_flag, BaiRun *tmp_runs,
                             hipStream_t s) {
    if (!t.n) return hipSuccess;
    const uint64_t blocks = (t.n + BT - 1) / BT;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bai_sorted, dim3((uint32_t)blocks), dim3(BT), 0, s, t, state, parity, lin, run_flag, tmp_runs);
    return hipGetLastError();
}

hipError_t launch_bai_survey(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, uint64_t first, const BaiLinear &lin, uint32_t mark,
                             uint32_t *len, hipStream_t s) {
    if (!n) return hipSuccess;
    const uint64_t blocks = (n + BT - 1) / BT;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bai_survey, dim3((uint32_t)blocks), dim3(BT), 0, s, raw, rec_off, n, first, lin, mark, len);
    return hipGetLastError();
}

hipError_t launch_bai_blocks(const uint64_t *off, uint64_t n_blocks, uint64_t base, uint64_t *table, hipStream_t s) {
    if (!n_blocks) return hipSuccess;
    const uint64_t blocks = (n_blocks + BT - 1) / BT;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bai_blocks, dim3((uint32_t)blocks), dim3(BT), 0, s, off, n_blocks, base, table);
    return hipGetLastError();
}

hipError_t launch_bai_translate(const BaiBlocks &b, BaiRun *runs, uint64_t n_runs, unsigned long long *lin, uint64_t n_win, hipStream_t s) {
    const uint64_t n = n_runs > n_win ? n_runs : n_win;
    if (!n) return hipSuccess;
    const uint64_t blocks = (n + BT - 1) / BT;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bai_translate, dim3((uint32_t)blocks), dim3(BT), 0, s, b, runs, n_runs, lin, n_win);
    return hipGetLastError();
}

hipError_t launch_bai_gather(const uint64_t *run_off, const BaiRun *tmp_runs, uint64_t n, BaiRun *runs, uint64_t base,
                             unsigned long long *host_count, hipStream_t s) {
    if (!n) return hipSuccess;
    const uint64_t blocks = (n + BT - 1) / BT;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bai_gather, dim3((uint32_t)blocks), dim3(BT), 0, s, run_off, tmp_runs, n, runs, base, host_count);
    return hipGetLastError();
}

hipError_t launch_bai_finish(const BaiLinear &lin, const BaiState *state, uint32_t parity, unsigned long long *host, hipStream_t s) {
    hipLaunchKernelGGL(k_bai_finish, dim3(lin.n_refs ? lin.n_refs : 1), dim3(BT), 0, s, lin, state, parity, host);
    return hipGetLastError();
}

} // namespace ngsq
