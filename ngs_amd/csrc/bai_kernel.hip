// bai_kernel.hip -- `ngs index` on the device: one pass over every batch of the device ingest in file
// order, then one launch that finishes the linear index.  bai.cpp drives them and writes the file.
#include <hip/hip_runtime.h>

#include "bai_kernels.h"

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

// reference span: the lengths of the CIGAR's M D N = X operations (a CIGAR without any counts as 1)
__device__ inline RecInfo bai_info(const ngsq_batch &b, uint64_t i) {
    RecInfo r;
    r.ref = b.ref_id[i];
    r.pos = b.pos[i];
    r.placed = r.ref >= 0 && r.pos >= 0;
    uint64_t span = 0;
    uint64_t k0, k1;
    if (b.cigar_off) {
        k0 = b.cigar_off[i];
        k1 = b.cigar_off[i + 1];
    } else {
        k0 = i * b.cigar_stride;
        k1 = k0 + min((uint32_t)b.n_cigar[i], b.cigar_stride);
    }
    for (uint64_t k = k0; k < k1; k++) {
        const uint32_t c = b.cigar[k], op = c & 15u;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += c >> 4;
    }
    r.end = (int64_t)r.pos + (int64_t)max(span, (uint64_t)1);
    r.bin = r.placed && r.end <= BAI_MAX_POS ? bai_reg2bin(r.pos, r.end) : BAI_UNPLACED_BIN;
    r.w0 = r.placed ? (uint32_t)(r.pos >> 14) : 0;
    r.w1 = r.placed ? (uint32_t)min((r.end - 1) >> 14, (int64_t)0xFFFFFFFF) : 0;
    return r;
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
    __shared__ int32_t s_ref[BT], s_pos[BT];
    __shared__ uint32_t s_bin[BT], s_w1[BT], s_placed[BT];
    __shared__ BaiCarry s_prev;
    const uint64_t n = b.n_records;
    const uint64_t i0 = (uint64_t)blockIdx.x * BT, i = i0 + threadIdx.x;
    const bool act = i < n;
    RecInfo me{};
    if (act) me = bai_info(b, i);
    s_ref[threadIdx.x] = me.ref;
    s_pos[threadIdx.x] = me.pos;
    s_bin[threadIdx.x] = me.bin;
    s_w1[threadIdx.x] = me.w1;
    s_placed[threadIdx.x] = me.placed;
    if (threadIdx.x == 0) {
        if (i0 == 0) {
            s_prev = st->carry[parity];
        } else { // the record in front of the block
            const RecInfo p = bai_info(b, i0 - 1);
            s_prev.ref = p.ref;
            s_prev.pos = p.pos;
            s_prev.bin = p.bin;
            s_prev.w1 = p.w1;
            s_prev.placed = p.placed;
            s_prev.has = 1;
            s_prev.endv = 0;
        }
    }
    __syncthreads();
    int32_t p_ref, p_pos;
    uint32_t p_bin, p_w1, p_placed, p_has;
    if (threadIdx.x) {
        p_ref = s_ref[threadIdx.x - 1];
        p_pos = s_pos[threadIdx.x - 1];
        p_bin = s_bin[threadIdx.x - 1];
        p_w1 = s_w1[threadIdx.x - 1];
        p_placed = s_placed[threadIdx.x - 1];
        p_has = 1;
    } else {
        p_ref = s_prev.ref;
        p_pos = s_prev.pos;
        p_bin = s_prev.bin;
        p_w1 = s_prev.w1;
        p_placed = s_prev.placed;
        p_has = s_prev.has;
    }
    bool head = false, bad = false, limit = false;
    uint32_t from = 0;
    if (act) {
        if (me.placed) {
            bad = p_has && (!p_placed || me.ref < p_ref || (me.ref == p_ref && me.pos < p_pos));
            head = !p_has || !p_placed || me.ref != p_ref || me.bin != p_bin;
            from = p_has && p_placed && p_ref == me.ref && p_w1 + 1 > me.w0 ? p_w1 + 1 : me.w0;
            limit = (uint32_t)me.ref >= L.n_refs || me.end > BAI_MAX_POS || me.w1 >= L.lin_cap[me.ref];
        } else {
            head = !p_has || p_placed;
        }
    }
    const bool lin_w = act && me.placed && !limit && from <= me.w1;
    if (bad) (void)atomicMin(&st->bad_order, (unsigned long long)(b.first_record_index + i));
    if (limit) (void)atomicMin(&st->bad_limit, (unsigned long long)(b.first_record_index + i));
    uint64_t startv = 0;
    if (head || lin_w) startv = i == 0 ? st->carry[parity].endv : bai_pos_after(o, o.rec_off[i]);
    if (act) run_flag[i] = head ? 1 : 0;
    if (head) {
        BaiRun r;
        r.start = startv;
        r.rec = b.first_record_index + i;
        r.ref = me.placed ? me.ref : -1;
        r.bin = me.bin;
        tmp[i] = r;
    }
    if (lin_w) { // the windows no record in front of this one overlaps (its predecessor covers everything up to p_w1)
        unsigned long long *w = L.lin + L.lin_base[me.ref];
        for (uint32_t k = from; k <= me.w1; k++) (void)atomicMin(&w[k], (unsigned long long)startv);
    }
    // placed records with the unmapped flag, per sequence: one atomic per wave and sequence (sorted: one sequence per wave)
    const bool unm = act && me.placed && !limit && (b.flag[i] & 0x4);
    uint64_t mask = __ballot(unm);
    while (mask) {
        const int leader = __ffsll((unsigned long long)mask) - 1;
        const int32_t lref = __shfl(me.ref, leader, 64);
        const uint64_t same = __ballot(unm && me.ref == lref) & mask;
        if ((int)(threadIdx.x & 63) == leader) (void)atomicAdd(&L.unmapped[lref], (unsigned long long)__popcll(same));
        mask &= ~same;
    }
    if (act && i == n - 1) {
        run_flag[n] = 0;
        const uint64_t at = o.rec_off[i];
        BaiCarry c;
        c.ref = me.ref;
        c.pos = me.pos;
        c.bin = me.bin;
        c.w1 = me.w1;
        c.placed = me.placed;
        c.has = 1;
        c.endv = bai_pos_after(o, at + 4 + ld32u(o.raw + at)); // behind the record's last byte (block_size + 4 bytes)
        st->carry[parity ^ 1u] = c;
    }
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
