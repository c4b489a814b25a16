// depth_kernel.hip -- `ngs depth` on the device.
//   k_depth_order   one thread per record: the coordinate order against the record in front, the batch's first and last sequence
//   k_depth_add     one thread per record: filter, reference span of the resolved CIGAR, +1 / -1 into the difference array
//   k_depth_count   one thread per record: the same filter alone, a ballot and one atomic a wave (sequences without an array, section 24)
//   k_depth_sums    a tile of the array, DEPTH_GRANULE positions per block: the block's sum of differences and count of run starts
//   k_depth_offsets one block: both turned into running values over the tile's blocks, from the carry of the tile in front
//   k_depth_runs    the tile again: every run start's coordinate and depth, compacted behind the run held back
//   k_depth_size    one thread per line: its bytes (a run ends where the next one starts)
//   k_depth_write   one thread per line: the text, staged per block in LDS and stored as aligned words
// A position starts a run exactly when its difference is not 0 (and the window's first position always does), so the run
// starts need no scan of the depths: the depths come from the same sums that carry the running depth from block to block.
// All stores are vector stores of plain C++.
#include <hip/hip_runtime.h>

#include "depth_kernels.h"

namespace ngsq {

namespace {

constexpr uint32_t BT = DEPTH_BT;

// The exclusive prefix of (s, c) over the block's threads, and the block's totals.  Two barriers; may be called again.
__device__ inline void block_exclusive(int32_t &s, uint32_t &c, int32_t *total_s, uint32_t *total_c) {
    __shared__ int32_t ws[BT / 64];
    __shared__ uint32_t wc[BT / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    int32_t is = s;
    uint32_t ic = c;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const int32_t ts = __shfl_up(is, d);
        const uint32_t tc = __shfl_up(ic, d);
        if (lane >= d) is += ts, ic += tc;
    }
    if (lane == 63) ws[wave] = is, wc[wave] = ic;
    __syncthreads();
    int32_t bs = 0, as = 0;
    uint32_t bc = 0, ac = 0;
    for (uint32_t k = 0; k < BT / 64; k++) {
        if (k < wave) bs += ws[k], bc += wc[k];
        as += ws[k], ac += wc[k];
    }
    s = bs + is - s;
    c = bc + ic - c;
    *total_s = as;
    *total_c = ac;
    __syncthreads();
}

__global__ __launch_bounds__(BT) void k_depth_order(ngsq_batch b, DepthState *st, uint32_t parity) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (i >= b.n_records) return;
    const int32_t ref = b.ref_id[i], pos = b.pos[i];
    const bool placed = ref >= 0 && pos >= 0;
    DepthCarry p;
    if (i > 0) {
        p.ref = b.ref_id[i - 1];
        p.pos = b.pos[i - 1];
        p.placed = p.ref >= 0 && p.pos >= 0;
        p.has = 1;
    } else {
        p = st->carry[parity];
    }
    if (placed && p.has && (!p.placed || ref < p.ref || (ref == p.ref && pos < p.pos)))
        (void)atomicMin(&st->bad_order, (unsigned long long)(b.first_record_index + i));
    if (placed && (i == 0 || !p.placed || p.ref != ref)) { // (sorted input: once per sequence of the batch)
        (void)atomicMin(&st->lo_ref, ref);
        (void)atomicMax(&st->hi_ref, ref);
    }
    if (i == b.n_records - 1) st->carry[parity ^ 1u] = DepthCarry{ref, pos, placed, 1u};
}

__global__ void k_depth_order_report(DepthState *st, unsigned long long *host) {
    host[0] = st->bad_order;
    host[1] = (unsigned long long)(uint32_t)st->lo_ref;
    host[2] = (unsigned long long)(uint32_t)st->hi_ref;
    st->lo_ref = INT32_MAX;
    st->hi_ref = -1;
}

__global__ __launch_bounds__(BT) void k_depth_add(ngsq_batch b, const uint8_t *__restrict__ keep, DepthWindow w, uint32_t exclude, uint32_t min_mapq,
                                                  DepthState *st) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    bool counts = false;
    if (i < b.n_records) {
        const int32_t pos = b.pos[i];
        counts = b.ref_id[i] == w.ref && pos >= 0 && ((uint32_t)b.flag[i] & exclude) == 0 && (uint32_t)b.mapq[i] >= min_mapq && (!keep || keep[i]);
        if (counts && (uint64_t)pos < (uint64_t)w.lo + w.len) {
            uint64_t k0, n_ops; // the operations as k_view_select takes them
            if (b.cigar_off) {
                k0 = b.cigar_off[i];
                n_ops = b.cigar_off[i + 1] - k0;
            } else {
                k0 = i * (uint64_t)b.cigar_stride;
                n_ops = min((uint32_t)b.n_cigar[i], b.cigar_stride);
            }
            uint64_t span = 0;
            for (uint64_t c = 0; c < n_ops; c++) {
                const uint32_t op = b.cigar[k0 + c];
                if ((0x18Du >> (op & 15u)) & 1u) span += op >> 4; // M D N = X
            }
            // clipped to the window: [from, to) of diff, to <= len
            const uint64_t from = max((uint64_t)pos, (uint64_t)w.lo), to = min((uint64_t)pos + span, (uint64_t)w.lo + w.len);
            if (from < to) {
                (void)atomicAdd(&w.diff[from - w.lo], 1);
                (void)atomicAdd(&w.diff[to - w.lo], -1);
            }
        }
    }
    const unsigned long long m = __ballot(counts);
    if ((threadIdx.x & 63u) == 0 && m) (void)atomicAdd(&st->counted, (unsigned long long)__popcll(m));
}

// k_depth_add's test alone, for a sequence that has no difference array (`ngs depth --by`)
__global__ __launch_bounds__(BT) void k_depth_count(ngsq_batch b, const uint8_t *__restrict__ keep, int32_t ref, uint32_t exclude, uint32_t min_mapq,
                                                    DepthState *st) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    bool counts = false;
    if (i < b.n_records)
        counts = b.ref_id[i] == ref && b.pos[i] >= 0 && ((uint32_t)b.flag[i] & exclude) == 0 && (uint32_t)b.mapq[i] >= min_mapq && (!keep || keep[i]);
    const unsigned long long m = __ballot(counts);
    if ((threadIdx.x & 63u) == 0 && m) (void)atomicAdd(&st->counted, (unsigned long long)__popcll(m));
}

// a thread's four differences of the tile (0 beyond its n positions) and which of them start a run
struct Items {
    int32_t v[DEPTH_ITEMS];
    bool f[DEPTH_ITEMS];
    int32_t sum;
    uint32_t count;
};
__device__ inline Items load_items(const int32_t *__restrict__ diff, uint64_t t0, uint32_t n, uint32_t p) {
    Items it;
    int4 q = make_int4(0, 0, 0, 0);
    if (p < n) q = *reinterpret_cast<const int4 *>(diff + t0 + p); // (16-byte aligned: t0 and p are multiples of 4; the array is padded to the granule)
    it.v[0] = q.x, it.v[1] = q.y, it.v[2] = q.z, it.v[3] = q.w;
    it.sum = 0, it.count = 0;
    for (uint32_t j = 0; j < DEPTH_ITEMS; j++) {
        if (p + j >= n) it.v[j] = 0;
        it.f[j] = p + j < n && (it.v[j] != 0 || t0 + p + j == 0);
        it.sum += it.v[j];
        it.count += it.f[j];
    }
    return it;
}

__global__ __launch_bounds__(BT) void k_depth_sums(const int32_t *__restrict__ diff, uint64_t t0, uint32_t n, int32_t *__restrict__ bsum,
                                                   uint32_t *__restrict__ bcnt) {
    const Items it = load_items(diff, t0, n, blockIdx.x * DEPTH_GRANULE + threadIdx.x * DEPTH_ITEMS);
    int32_t s = it.sum, ts;
    uint32_t c = it.count, tc;
    block_exclusive(s, c, &ts, &tc);
    if (threadIdx.x == 0) bsum[blockIdx.x] = ts, bcnt[blockIdx.x] = tc;
}

__global__ __launch_bounds__(BT) void k_depth_offsets(uint32_t n_blocks, int32_t *__restrict__ bsum, uint32_t *__restrict__ bcnt,
                                                      uint32_t *__restrict__ rstart, int32_t *__restrict__ rdepth, DepthState *st) {
    int32_t run_s = st->depth;
    const uint32_t open = st->open;
    uint32_t run_c = open;
    for (uint32_t base = 0; base < n_blocks; base += BT) {
        const uint32_t i = base + threadIdx.x;
        int32_t s = i < n_blocks ? bsum[i] : 0, ts;
        uint32_t c = i < n_blocks ? bcnt[i] : 0, tc;
        block_exclusive(s, c, &ts, &tc);
        if (i < n_blocks) bsum[i] = run_s + s, bcnt[i] = run_c + c;
        run_s += ts;
        run_c += tc;
    }
    __syncthreads(); // (every thread has read the state)
    if (threadIdx.x == 0) {
        if (open) rstart[0] = st->open_start, rdepth[0] = st->open_depth;
        st->depth = run_s;
        st->n_runs = run_c;
    }
}

__global__ __launch_bounds__(BT) void k_depth_runs(const int32_t *__restrict__ diff, uint64_t t0, uint32_t n, uint32_t lo, const int32_t *__restrict__ bsum,
                                                   const uint32_t *__restrict__ bcnt, uint32_t *__restrict__ rstart, int32_t *__restrict__ rdepth) {
    const uint32_t p = blockIdx.x * DEPTH_GRANULE + threadIdx.x * DEPTH_ITEMS;
    const Items it = load_items(diff, t0, n, p);
    int32_t s = it.sum, ts;
    uint32_t c = it.count, tc;
    block_exclusive(s, c, &ts, &tc);
    int32_t depth = bsum[blockIdx.x] + s;
    uint32_t at = bcnt[blockIdx.x] + c; // < open + the tile's run starts <= n + 1
    for (uint32_t j = 0; j < DEPTH_ITEMS; j++) {
        depth += it.v[j];
        if (it.f[j]) {
            rstart[at] = lo + (uint32_t)(t0 + p + j);
            rdepth[at] = depth;
            at++;
        }
    }
}

__device__ inline uint32_t digits(uint32_t v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
           (v >= 100000000u) + (v >= 1000000000u);
}

__global__ __launch_bounds__(BT) void k_depth_size(uint64_t entries, uint32_t final, uint32_t final_end, uint32_t name_len, const uint32_t *__restrict__ rstart,
                                                   const int32_t *__restrict__ rdepth, uint64_t *__restrict__ off, DepthState *st) {
    const uint64_t k = (uint64_t)blockIdx.x * BT + threadIdx.x;
    const uint32_t runs = st->n_runs, lines = final ? runs : runs - 1;
    if (k == 0) st->lines = lines;
    if (k >= entries) return;
    uint64_t bytes = 0;
    if (k < lines) {
        const uint32_t end = k + 1 < runs ? rstart[k + 1] : final_end;
        bytes = name_len + 4u + digits(rstart[k]) + digits(end) + digits((uint32_t)rdepth[k]);
    }
    off[k] = bytes;
}

__global__ void k_depth_total(uint32_t final, const uint32_t *rstart, const int32_t *rdepth, const uint64_t *off, DepthState *st, unsigned long long *host) {
    const uint32_t lines = st->lines, runs = st->n_runs;
    host[0] = off[lines];
    host[1] = lines;
    if (final) {
        st->open = 0;
        st->depth = 0;
    } else {
        st->open = 1;
        st->open_start = rstart[runs - 1];
        st->open_depth = rdepth[runs - 1];
    }
}

// v in decimal, its last digit at p[-1]; returns where its first digit lies
__device__ inline char *put_back(char *p, uint32_t v) {
    do {
        *--p = (char)('0' + v % 10u);
        v /= 10u;
    } while (v);
    return p;
}

// "name\tstart\tend\tdepth\n" at dst, `bytes` long
__device__ inline void put_line(char *dst, uint32_t bytes, const char *__restrict__ name, uint32_t name_len, uint32_t start, uint32_t end, uint32_t depth) {
    for (uint32_t j = 0; j < name_len; j++) dst[j] = name[j];
    char *p = dst + bytes;
    *--p = '\n';
    p = put_back(p, depth);
    *--p = '\t';
    p = put_back(p, end);
    *--p = '\t';
    p = put_back(p, start);
    *--p = '\t';
}

// The lines of a block are one contiguous piece of the text.  Where it fits, the block writes them into LDS at the piece's own
// phase against a 4-byte boundary, and stores the piece as aligned words (bytes at its two ends); a piece that does not fit
// (names of several dozen bytes) is stored byte by byte.
__global__ __launch_bounds__(BT) void k_depth_write(char *__restrict__ text, uint32_t lines, uint32_t final, uint32_t final_end, const char *__restrict__ name,
                                                    uint32_t name_len, const uint32_t *__restrict__ rstart, const int32_t *__restrict__ rdepth,
                                                    const uint64_t *__restrict__ off) {
    __shared__ uint32_t stage[DEPTH_STAGE_BYTES / 4];
    const uint32_t k0 = blockIdx.x * BT, k1 = min(k0 + BT, lines), k = k0 + threadIdx.x;
    const uint64_t b0 = off[k0], b1 = off[k1];
    const uintptr_t g0 = reinterpret_cast<uintptr_t>(text) + b0, g1 = reinterpret_cast<uintptr_t>(text) + b1;
    const uint32_t phase = (uint32_t)(g0 & 3u);
    const bool staged = b1 - b0 + phase <= DEPTH_STAGE_BYTES; // (the same in every thread)
    if (k < k1) {
        const uint64_t at = off[k];
        const uint32_t bytes = (uint32_t)(off[k + 1] - at);
        const uint32_t end = (k + 1 < lines || !final) ? rstart[k + 1] : final_end;
        char *dst = staged ? reinterpret_cast<char *>(stage) + phase + (uint32_t)(at - b0) : text + at;
        put_line(dst, bytes, name, name_len, rstart[k], end, (uint32_t)rdepth[k]);
    }
    if (!staged) return;
    __syncthreads();
    const uintptr_t gbase = g0 - phase;
    const uint32_t n_words = (uint32_t)((g1 - gbase + 3u) / 4u);
    for (uint32_t wd = threadIdx.x; wd < n_words; wd += BT) {
        const uintptr_t a = gbase + (uintptr_t)wd * 4u;
        if (a >= g0 && a + 4u <= g1) {
            *reinterpret_cast<uint32_t *>(a) = stage[wd];
        } else {
            const char *src = reinterpret_cast<const char *>(stage) + wd * 4u;
            for (uint32_t j = 0; j < 4; j++)
                if (a + j >= g0 && a + j < g1) *reinterpret_cast<char *>(a + j) = src[j];
        }
    }
}

__global__ void k_depth_zero_line(char *text, const char *name, uint32_t name_len, uint32_t start, uint32_t end) {
    put_line(text, name_len + 4u + digits(start) + digits(end) + 1u, name, name_len, start, end, 0u);
}

inline bool grid_of(uint64_t n, uint32_t per_block, uint32_t *blocks) {
    const uint64_t g = (n + per_block - 1) / per_block;
    *blocks = (uint32_t)g;
    return g >= 1 && g <= 0x7FFFFFFFull;
}

} // namespace

hipError_t launch_depth_order(const ngsq_batch &b, DepthState *state, uint32_t parity, unsigned long long *host, hipStream_t s) {
    uint32_t blocks;
    if (!grid_of(b.n_records, BT, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_depth_order, dim3(blocks), dim3(BT), 0, s, b, state, parity);
    hipLaunchKernelGGL(k_depth_order_report, dim3(1), dim3(1), 0, s, state, host);
    return hipGetLastError();
}

hipError_t launch_depth_add(const ngsq_batch &b, const uint8_t *keep, const DepthWindow &w, uint32_t exclude_flags, uint32_t min_mapq,
                            DepthState *state, hipStream_t s) {
    uint32_t blocks;
    if (!w.len || !grid_of(b.n_records, BT, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_depth_add, dim3(blocks), dim3(BT), 0, s, b, keep, w, exclude_flags, min_mapq, state);
    return hipGetLastError();
}

hipError_t launch_depth_count(const ngsq_batch &b, const uint8_t *keep, int32_t ref, uint32_t exclude_flags, uint32_t min_mapq, DepthState *state,
                              hipStream_t s) {
    uint32_t blocks;
    if (!state || !b.ref_id || !b.pos || !b.flag || !b.mapq || !grid_of(b.n_records, BT, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_depth_count, dim3(blocks), dim3(BT), 0, s, b, keep, ref, exclude_flags, min_mapq, state);
    return hipGetLastError();
}

hipError_t launch_depth_runs(const DepthWindow &w, uint64_t t0, uint32_t n, const DepthTileArrays &a, DepthState *state, hipStream_t s) {
    uint32_t blocks;
    if (t0 % DEPTH_GRANULE || t0 + n > w.len || !grid_of(n, DEPTH_GRANULE, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_depth_sums, dim3(blocks), dim3(BT), 0, s, w.diff, t0, n, a.bsum, a.bcnt);
    hipLaunchKernelGGL(k_depth_offsets, dim3(1), dim3(BT), 0, s, blocks, a.bsum, a.bcnt, a.rstart, a.rdepth, state);
    hipLaunchKernelGGL(k_depth_runs, dim3(blocks), dim3(BT), 0, s, w.diff, t0, n, w.lo, a.bsum, a.bcnt, a.rstart, a.rdepth);
    return hipGetLastError();
}

hipError_t launch_depth_size(uint64_t entries, bool final, uint32_t final_end, uint32_t name_len, const DepthTileArrays &a, DepthState *state, hipStream_t s) {
    uint32_t blocks;
    if (!grid_of(entries, BT, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_depth_size, dim3(blocks), dim3(BT), 0, s, entries, final ? 1u : 0u, final_end, name_len, a.rstart, a.rdepth, a.off, state);
    return hipGetLastError();
}

hipError_t launch_depth_total(bool final, const DepthTileArrays &a, DepthState *state, unsigned long long *host, hipStream_t s) {
    hipLaunchKernelGGL(k_depth_total, dim3(1), dim3(1), 0, s, final ? 1u : 0u, a.rstart, a.rdepth, a.off, state, host);
    return hipGetLastError();
}

hipError_t launch_depth_write(char *text, uint32_t lines, bool final, uint32_t final_end, const char *name, uint32_t name_len, const DepthTileArrays &a,
                              hipStream_t s) {
    uint32_t blocks;
    if (!lines) return hipSuccess;
    if (!grid_of(lines, BT, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_depth_write, dim3(blocks), dim3(BT), 0, s, text, lines, final ? 1u : 0u, final_end, name, name_len, a.rstart, a.rdepth, a.off);
    return hipGetLastError();
}

hipError_t launch_depth_zero_line(char *text, const char *name, uint32_t name_len, uint32_t start, uint32_t end, hipStream_t s) {
    hipLaunchKernelGGL(k_depth_zero_line, dim3(1), dim3(1), 0, s, text, name, name_len, start, end);
    return hipGetLastError();
}

} // namespace ngsq
