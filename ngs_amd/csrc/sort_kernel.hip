// sort_kernel.hip -- the kernels of `ngs convert --sort coordinate`, gfx950, wave64: record keys, a
// stable LSD radix sort of (key, index) pairs, and the gather of resident records into pieces of the sorted stream; for BAM input
// (section 20.3) the copy of a batch of the device ingest into a slab; for a BAM sorted in rounds (section 22.3) the survey's keys,
// the plan's cut and the copy of a round's records out of a batch.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sort_kernels.h"

namespace ngsq {

namespace {

constexpr uint32_t BT = 256;            // threads of the one-thread-per-item kernels
constexpr uint32_t HIST_PER_THREAD = 16; // keys a thread of k_sort_hist takes at least, when the grid is not capped
constexpr uint32_t HIST_MAX_BLOCKS = 2048;
constexpr uint32_t GATHER_WAVES = BT / 64; // records a workgroup of k_sort_gather copies
constexpr uint32_t KEEP_MAX_BLOCKS = 4096; // of k_sort_keep: its threads stride over the words and over the records

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ uint32_t digit_of(uint64_t key, uint32_t digit) { return (uint32_t)(key >> (8u * digit)) & 255u; }
// (a record lies at any byte offset)
__device__ __forceinline__ uint32_t load_u32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// ---- the sort ---------------------------------------------------------------------------------------------------------------

// all eight digit histograms in one read of the keys: LDS counts per workgroup, then one global add per bin in use
__global__ __launch_bounds__(BT) void k_sort_hist(const uint64_t *__restrict__ keys, uint64_t n, unsigned long long *__restrict__ hist) {
    __shared__ uint32_t h[SORT_DIGITS * SORT_BINS];
    for (uint32_t i = threadIdx.x; i < SORT_DIGITS * SORT_BINS; i += BT) h[i] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BT) { // (n < 2^32: a count fits its word)
        const uint64_t k = keys[i];
#pragma unroll
        for (uint32_t d = 0; d < SORT_DIGITS; d++) atomicAdd(&h[d * SORT_BINS + digit_of(k, d)], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < SORT_DIGITS * SORT_BINS; i += BT)
        if (h[i]) atomicAdd(&hist[i], (unsigned long long)h[i]);
}

// the digit counts of a tile, into the digit-major table the scan turns into offsets
__global__ __launch_bounds__(SORT_BT) void k_sort_count(const uint64_t *__restrict__ keys, uint64_t n, uint32_t digit, uint64_t *__restrict__ table,
                                                        uint64_t tiles) {
    __shared__ uint32_t h[SORT_BINS];
    if (threadIdx.x < SORT_BINS) h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * SORT_TILE;
#pragma unroll
    for (uint32_t r = 0; r < SORT_ROUNDS; r++) {
        const uint64_t i = base + (uint64_t)r * SORT_BT + threadIdx.x;
        if (i < n) atomicAdd(&h[digit_of(keys[i], digit)], 1u);
    }
    __syncthreads();
    if (threadIdx.x < SORT_BINS) table[(uint64_t)threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
    if (blockIdx.x == 0 && threadIdx.x == 0) table[(uint64_t)SORT_BINS * tiles] = 0;
}

// A tile's pairs to their slots.  Wave w ranks the tile's keys [w * ROUNDS * 64, (w + 1) * ROUNDS * 64), 64 consecutive ones per
// round: a lane's peers are the lanes of the round with its digit (the AND over the digit's bits of ballot or ~ballot), its rank
// among them the peers below it, and cnt[w][digit] the keys of that digit in the wave's earlier rounds.  Then the waves' counts
// become their bases behind the table's offset, and a pair's slot is base + rank: input order within a digit throughout.
__global__ __launch_bounds__(SORT_BT) void k_sort_scatter(const uint64_t *__restrict__ keys_in, const uint32_t *__restrict__ idx_in, uint64_t n,
                                                          uint32_t digit, const uint64_t *__restrict__ table, uint64_t tiles,
                                                          uint64_t *__restrict__ keys_out, uint32_t *__restrict__ idx_out) {
    __shared__ uint32_t cnt[SORT_BT / 64][SORT_BINS];
    const uint32_t w = threadIdx.x >> 6, lane = lane_id();
    for (uint32_t i = threadIdx.x; i < (SORT_BT / 64) * SORT_BINS; i += SORT_BT) (&cnt[0][0])[i] = 0;
    __syncthreads();
    const uint64_t seg = (uint64_t)blockIdx.x * SORT_TILE + (uint64_t)w * (SORT_ROUNDS * 64);
    const unsigned long long below_mask = (1ull << lane) - 1ull;
    uint64_t key[SORT_ROUNDS];
    uint32_t rank[SORT_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < SORT_ROUNDS; r++) {
        const uint64_t i = seg + r * 64 + lane;
        const bool valid = i < n;
        key[r] = valid ? keys_in[i] : 0;
        const uint32_t d = digit_of(key[r], digit);
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (uint32_t b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            peers &= bit ? bal : ~bal;
        }
        rank[r] = 0;
        if (valid) {
            const uint32_t below = (uint32_t)__popcll(peers & below_mask);
            const uint32_t old = cnt[w][d]; // (every peer reads it before the first of them adds the round's count)
            rank[r] = old + below;
            if (below == 0) cnt[w][d] = old + (uint32_t)__popcll(peers);
        }
    }
    __syncthreads();
    if (threadIdx.x < SORT_BINS) {
        uint32_t run = (uint32_t)table[(uint64_t)threadIdx.x * tiles + blockIdx.x]; // (a slot is below n < 2^32)
        for (uint32_t v = 0; v < SORT_BT / 64; v++) {
            const uint32_t c = cnt[v][threadIdx.x];
            cnt[v][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < SORT_ROUNDS; r++) {
        const uint64_t i = seg + r * 64 + lane;
        if (i < n) {
            const uint32_t dst = cnt[w][digit_of(key[r], digit)] + rank[r];
            keys_out[dst] = key[r];
            idx_out[dst] = idx_in ? idx_in[i] : (uint32_t)i;
        }
    }
}

__global__ __launch_bounds__(BT) void k_sort_iota(uint32_t *__restrict__ idx, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (i < n) idx[i] = (uint32_t)i;
}

// ---- records ----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(BT) void k_sort_keys(const uint8_t *__restrict__ base, const uint64_t *__restrict__ off, uint64_t n, uint64_t first,
                                                  uint64_t *__restrict__ addr, uint32_t *__restrict__ len, uint64_t *__restrict__ key) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (i >= n) return;
    const uint8_t *p = base + off[i];
    const int32_t ref_id = (int32_t)load_u32(p + 4), pos = (int32_t)load_u32(p + 8);
    const uint32_t hi = (ref_id < 0 || pos < 0) ? 0xFFFFFFFFu : (uint32_t)ref_id, lo = (uint32_t)pos + 1u;
    addr[first + i] = (uint64_t)(uintptr_t)p;
    len[first + i] = (uint32_t)(off[i + 1] - off[i]);
    key[first + i] = (uint64_t)hi << 32 | lo;
}

// where the records of a batch of the device ingest lie in its view: they are consecutive, so from the first one's first byte
// to the last one's last
__global__ __launch_bounds__(64) void k_sort_span(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ rec_off, uint64_t n, unsigned long long *host) {
    if (blockIdx.x || threadIdx.x) return;
    const uint64_t last = rec_off[n - 1];
    host[0] = rec_off[0];
    host[1] = last + 4u + (uint64_t)load_u32(raw + last);
}

// The batch's bytes raw[begin, begin + bytes) to dst, which has the source's residue modulo 16 (the launcher checks it): up to 15
// bytes until both are aligned, 16-byte words, up to 15 bytes behind them; nothing outside either range is read or written.  And
// what k_sort_keys leaves per record, read from the record's head in the view (it lies at any byte offset).
__global__ __launch_bounds__(BT) void k_sort_keep(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ rec_off, uint64_t n, uint64_t begin,
                                                  uint64_t bytes, uint8_t *__restrict__ dst, uint64_t first, uint64_t *__restrict__ addr,
                                                  uint32_t *__restrict__ len, uint64_t *__restrict__ key) {
    const uint64_t g = (uint64_t)blockIdx.x * BT + threadIdx.x, stride = (uint64_t)gridDim.x * BT;
    const uint8_t *src = raw + begin;
    uint64_t head = (16u - (uint32_t)((uintptr_t)src & 15u)) & 15u;
    if (head > bytes) head = bytes;
    const uint64_t words = (bytes - head) >> 4, tail_at = head + words * 16, tail = bytes - tail_at;
    if (g < head) dst[g] = src[g];
    if (g < tail) dst[tail_at + g] = src[tail_at + g];
    const uint4 *sw = reinterpret_cast<const uint4 *>(src + head);
    uint4 *dw = reinterpret_cast<uint4 *>(dst + head);
    for (uint64_t k = g; k < words; k += stride) dw[k] = sw[k];
    for (uint64_t i = g; i < n; i += stride) {
        const uint64_t o = rec_off[i];
        const uint8_t *p = raw + o;
        const int32_t ref_id = (int32_t)load_u32(p + 4), pos = (int32_t)load_u32(p + 8);
        const uint32_t hi = (ref_id < 0 || pos < 0) ? 0xFFFFFFFFu : (uint32_t)ref_id, lo = (uint32_t)pos + 1u;
        addr[first + i] = (uint64_t)(uintptr_t)(dst + (o - begin));
        len[first + i] = 4u + load_u32(p);
        key[first + i] = (uint64_t)hi << 32 | lo;
    }
}

__global__ __launch_bounds__(BT) void k_sort_lengths(const uint32_t *__restrict__ len, const uint32_t *__restrict__ perm, uint64_t n,
                                                     uint64_t *__restrict__ slen) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (i < n) slen[i] = len[perm[i]];
    if (i == 0) slen[n] = 0;
}

__global__ __launch_bounds__(BT) void k_sort_bisect(const uint64_t *__restrict__ soff, uint64_t n, uint64_t piece_bytes, uint64_t first_piece,
                                                    uint64_t before, uint64_t pieces, unsigned long long *host) {
    const uint64_t j = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (j > pieces) return;
    const uint64_t at = (first_piece + j) * piece_bytes, target = at > before ? at - before : 0;
    uint64_t lo = 0, hi = n; // the smallest i with soff[i + 1] > target, n when there is none
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (soff[mid + 1] > target) hi = mid;
        else lo = mid + 1;
    }
    host[j] = lo;
}

__global__ __launch_bounds__(BT) void k_sort_gather(const uint64_t *__restrict__ addr, const uint32_t *__restrict__ perm, const uint64_t *__restrict__ soff,
                                                    uint64_t a, uint64_t b, uint64_t lo, uint64_t hi, uint8_t *__restrict__ out) {
    const uint64_t r = a + (uint64_t)blockIdx.x * GATHER_WAVES + (threadIdx.x >> 6);
    if (r >= b) return;
    const uint64_t s0 = soff[r], s1 = soff[r + 1];
    const uint64_t c0 = s0 > lo ? s0 : lo, c1 = s1 < hi ? s1 : hi;
    if (c0 >= c1) return;
    const uint32_t lane = lane_id();
    const uint8_t *src = reinterpret_cast<const uint8_t *>((uintptr_t)addr[perm[r]]) + (c0 - s0);
    uint8_t *dst = out + (c0 - lo);
    uint64_t left = c1 - c0;
    // up to seven bytes until the destination is aligned
    uint64_t head = (8u - (uint32_t)((uintptr_t)dst & 7u)) & 7u;
    if (head > left) head = left;
    if (lane < head) dst[lane] = src[lane];
    src += head, dst += head, left -= head;
    // whole words: the source as aligned words, shifted (the slab is readable SORT_GATHER_SLACK bytes behind its records)
    const uint64_t words = left >> 3;
    const uint32_t mis = (uint32_t)((uintptr_t)src & 7u), sh = mis * 8u;
    const uint64_t *sw = reinterpret_cast<const uint64_t *>(src - mis);
    uint64_t *dw = reinterpret_cast<uint64_t *>(dst);
    for (uint64_t k = lane; k < words; k += 64) {
        uint64_t x = sw[k];
        if (sh) x = x >> sh | sw[k + 1] << (64u - sh);
        dw[k] = x;
    }
    const uint64_t tail = left & 7u;
    if (lane < tail) dst[words * 8 + lane] = src[words * 8 + lane];
}

// ---- rounds: the survey walk keeps a key and a length per record, a round's walk keeps the records
// whose (key, input ordinal) lies inside the round's two boundaries

__device__ __forceinline__ uint64_t key_of(const uint8_t *p) {
    const int32_t ref_id = (int32_t)load_u32(p + 4), pos = (int32_t)load_u32(p + 8);
    const uint32_t hi = (ref_id < 0 || pos < 0) ? 0xFFFFFFFFu : (uint32_t)ref_id, lo = (uint32_t)pos + 1u;
    return (uint64_t)hi << 32 | lo;
}

__global__ __launch_bounds__(BT) void k_sort_survey(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ rec_off, uint64_t n, uint64_t first,
                                                    uint32_t *__restrict__ len, uint64_t *__restrict__ key) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (i >= n) return;
    const uint8_t *p = raw + rec_off[i];
    len[first + i] = 4u + load_u32(p);
    key[first + i] = key_of(p);
}

// the sorted lengths without the mark in their top bit, and the smallest sorted rank that carries it
__global__ __launch_bounds__(BT) void k_sort_survey_lengths(const uint32_t *__restrict__ len, const uint32_t *__restrict__ perm, uint64_t n,
                                                            uint64_t *__restrict__ slen, unsigned long long *__restrict__ marked) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (i < n) {
        const uint32_t l = len[perm[i]];
        slen[i] = l & ~SORT_SURVEY_MARK;
        if (l & SORT_SURVEY_MARK) (void)atomicMin(marked, (unsigned long long)i);
    }
    if (i == 0) slen[n] = 0;
}

// the largest end with soff[end] - soff[start] + per_record * (end - start) <= budget, and the boundary in front of it
__global__ __launch_bounds__(64) void k_sort_plan(const uint64_t *__restrict__ soff, const uint64_t *__restrict__ skey, const uint32_t *__restrict__ perm,
                                                  uint64_t n, uint64_t start, uint64_t budget, uint64_t per_record, unsigned long long *host) {
    if (blockIdx.x || threadIdx.x) return;
    uint64_t lo = start, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (soff[mid] - soff[start] + per_record * (mid - start) <= budget) lo = mid;
        else hi = mid - 1;
    }
    host[SP_END] = lo;
    host[SP_END_OFF] = soff[lo];
    host[SP_KEY] = lo < n ? skey[lo] : ~0ull;
    host[SP_ORD] = lo < n ? perm[lo] : ~0ull;
    host[SP_FIRST_LEN] = start < n ? soff[start + 1] - soff[start] : 0;
}

__global__ __launch_bounds__(BT) void k_sort_round_flag(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ rec_off, uint64_t n, uint64_t first,
                                                        SortBound lo, SortBound hi, uint64_t *__restrict__ cnt, uint64_t *__restrict__ bytes) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (i == 0) cnt[n] = bytes[n] = 0;
    if (i >= n) return;
    const uint8_t *p = raw + rec_off[i];
    const uint64_t k = key_of(p), ord = first + i;
    const bool in = (k > lo.key || (k == lo.key && ord >= lo.ord)) && (k < hi.key || (k == hi.key && ord < hi.ord));
    cnt[i] = in ? 1 : 0;
    bytes[i] = in ? 4u + (uint64_t)load_u32(p) : 0;
}

// A wave per record of the batch; a kept one goes whole to dst + off[r] and leaves address, length and key at first + cnt[r].
// Source and destination lie at any byte offset: up to seven bytes until the destination is aligned, eight-byte stores of the
// source's aligned words, shifted, and the rest by bytes.  The first word's low bytes come by bytes and the last word is left
// to the tail, so that no load reaches in front of the record or behind it.
__global__ __launch_bounds__(BT) void k_sort_take(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ rec_off, uint64_t n,
                                                  const uint64_t *__restrict__ cnt, const uint64_t *__restrict__ off, uint8_t *__restrict__ out,
                                                  uint64_t first, uint64_t *__restrict__ addr, uint32_t *__restrict__ len, uint64_t *__restrict__ key) {
    const uint64_t r = (uint64_t)blockIdx.x * GATHER_WAVES + (threadIdx.x >> 6);
    if (r >= n) return;
    const uint64_t c = cnt[r];
    if (cnt[r + 1] == c) return;
    const uint32_t lane = lane_id();
    const uint8_t *src = raw + rec_off[r];
    uint8_t *dst = out + off[r];
    uint64_t left = off[r + 1] - off[r];
    if (lane == 0) {
        addr[first + c] = (uint64_t)(uintptr_t)dst;
        len[first + c] = (uint32_t)left;
        key[first + c] = key_of(src);
    }
    uint64_t head = (8u - (uint32_t)((uintptr_t)dst & 7u)) & 7u;
    if (head > left) head = left;
    if (lane < head) dst[lane] = src[lane];
    src += head, dst += head, left -= head;
    const uint32_t mis = (uint32_t)((uintptr_t)src & 7u), sh = mis * 8u;
    uint64_t words = left >> 3;
    if (mis && words) words--; // (its second source word would reach behind the record)
    const uint64_t *sw = reinterpret_cast<const uint64_t *>(src - mis);
    uint64_t *dw = reinterpret_cast<uint64_t *>(dst);
    for (uint64_t k = lane; k < words; k += 64) {
        uint64_t x;
        if (!mis) {
            x = sw[k];
        } else {
            uint64_t low = 0;
            if (k == 0) { // (the aligned word begins in front of the record)
                for (uint32_t q = 0; q < 8u - mis; q++) low |= (uint64_t)src[q] << (8u * (mis + q));
            } else {
                low = sw[k];
            }
            x = low >> sh | sw[k + 1] << (64u - sh);
        }
        dw[k] = x;
    }
    const uint64_t done = words * 8, tail = left - done; // (at most 15)
    if (lane < tail) dst[done + lane] = src[done + lane];
}

uint32_t blocks_of(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

} // namespace

hipError_t launch_sort_histogram(const uint64_t *keys, uint64_t n, unsigned long long *hist, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(hist, 0, SORT_DIGITS * SORT_BINS * sizeof(unsigned long long), s);
    if (e != hipSuccess || !n) return e;
    const uint64_t want = (n + (uint64_t)BT * HIST_PER_THREAD - 1) / ((uint64_t)BT * HIST_PER_THREAD);
    hipLaunchKernelGGL(k_sort_hist, dim3((uint32_t)(want < HIST_MAX_BLOCKS ? want : HIST_MAX_BLOCKS)), dim3(BT), 0, s, keys, n, hist);
    return hipGetLastError();
}

hipError_t launch_sort_count(const uint64_t *keys, uint64_t n, uint32_t digit, uint64_t *table, hipStream_t s) {
    const uint64_t tiles = sort_tiles(n);
    if (!tiles || tiles > 0x7FFFFFFFull || digit >= SORT_DIGITS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sort_count, dim3((uint32_t)tiles), dim3(SORT_BT), 0, s, keys, n, digit, table, tiles);
    return hipGetLastError();
}

hipError_t launch_sort_scatter(const uint64_t *keys_in, const uint32_t *idx_in, uint64_t n, uint32_t digit, const uint64_t *table, uint64_t *keys_out,
                               uint32_t *idx_out, hipStream_t s) {
    const uint64_t tiles = sort_tiles(n);
    if (!tiles || tiles > 0x7FFFFFFFull || n > 0xFFFFFFFFull || digit >= SORT_DIGITS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sort_scatter, dim3((uint32_t)tiles), dim3(SORT_BT), 0, s, keys_in, idx_in, n, digit, table, tiles, keys_out, idx_out);
    return hipGetLastError();
}

hipError_t launch_sort_iota(uint32_t *idx, uint64_t n, hipStream_t s) {
    if (!n) return hipSuccess;
    if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sort_iota, dim3(blocks_of(n, BT)), dim3(BT), 0, s, idx, n);
    return hipGetLastError();
}

hipError_t launch_sort_keys(const uint8_t *base, const uint64_t *off, uint64_t n, uint64_t first, uint64_t *addr, uint32_t *len, uint64_t *key,
                            hipStream_t s) {
    if (!n) return hipSuccess;
    if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sort_keys, dim3(blocks_of(n, BT)), dim3(BT), 0, s, base, off, n, first, addr, len, key);
    return hipGetLastError();
}

hipError_t launch_sort_span(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, unsigned long long *host, hipStream_t s) {
    if (!n) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sort_span, dim3(1), dim3(64), 0, s, raw, rec_off, n, host);
    return hipGetLastError();
}

hipError_t launch_sort_keep(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, uint64_t begin, uint64_t bytes, uint8_t *dst, uint64_t first,
                            uint64_t *addr, uint32_t *len, uint64_t *key, hipStream_t s) {
    if (!n) return hipSuccess;
    if (n > 0xFFFFFFFFull || (((uintptr_t)(raw + begin) ^ (uintptr_t)dst) & 15u)) return hipErrorInvalidValue;
    const uint64_t want = std::max<uint64_t>((n + BT - 1) / BT, ((bytes >> 4) + BT - 1) / BT);
    hipLaunchKernelGGL(k_sort_keep, dim3((uint32_t)std::min<uint64_t>(std::max<uint64_t>(want, 1), KEEP_MAX_BLOCKS)), dim3(BT), 0, s, raw, rec_off, n, begin,
                       bytes, dst, first, addr, len, key);
    return hipGetLastError();
}

hipError_t launch_sort_lengths(const uint32_t *len, const uint32_t *perm, uint64_t n, uint64_t *slen, hipStream_t s) {
    if (!n || n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sort_lengths, dim3(blocks_of(n, BT)), dim3(BT), 0, s, len, perm, n, slen);
    return hipGetLastError();
}

hipError_t launch_sort_bisect(const uint64_t *soff, uint64_t n, uint64_t piece_bytes, uint64_t first_piece, uint64_t before, uint64_t pieces,
                              unsigned long long *host, hipStream_t s) {
    if (!piece_bytes || pieces >= 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sort_bisect, dim3(blocks_of(pieces + 1, BT)), dim3(BT), 0, s, soff, n, piece_bytes, first_piece, before, pieces, host);
    return hipGetLastError();
}

hipError_t launch_sort_survey(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, uint64_t first, uint32_t *len, uint64_t *key, hipStream_t s) {
    if (!n) return hipSuccess;
    if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sort_survey, dim3(blocks_of(n, BT)), dim3(BT), 0, s, raw, rec_off, n, first, len, key);
    return hipGetLastError();
}

hipError_t launch_sort_survey_lengths(const uint32_t *len, const uint32_t *perm, uint64_t n, uint64_t *slen, unsigned long long *marked, hipStream_t s) {
    if (!n || n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(marked, 0xFF, sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sort_survey_lengths, dim3(blocks_of(n, BT)), dim3(BT), 0, s, len, perm, n, slen, marked);
    return hipGetLastError();
}

hipError_t launch_sort_plan(const uint64_t *soff, const uint64_t *skey, const uint32_t *perm, uint64_t n, uint64_t start, uint64_t budget,
                            uint64_t per_record, unsigned long long *host, hipStream_t s) {
    if (!n || start >= n) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sort_plan, dim3(1), dim3(64), 0, s, soff, skey, perm, n, start, budget, per_record, host);
    return hipGetLastError();
}

hipError_t launch_sort_round_flag(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, uint64_t first, SortBound lo, SortBound hi, uint64_t *cnt,
                                  uint64_t *bytes, hipStream_t s) {
    if (!n || n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sort_round_flag, dim3(blocks_of(n, BT)), dim3(BT), 0, s, raw, rec_off, n, first, lo, hi, cnt, bytes);
    return hipGetLastError();
}

hipError_t launch_sort_take(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, const uint64_t *cnt, const uint64_t *off, uint8_t *dst,
                            uint64_t first, uint64_t *addr, uint32_t *len, uint64_t *key, hipStream_t s) {
    if (!n || n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sort_take, dim3(blocks_of(n, GATHER_WAVES)), dim3(BT), 0, s, raw, rec_off, n, cnt, off, dst, first, addr, len, key);
    return hipGetLastError();
}

hipError_t launch_sort_gather(const uint64_t *addr, const uint32_t *perm, const uint64_t *soff, uint64_t a, uint64_t b, uint64_t lo, uint64_t hi,
                              uint8_t *out, hipStream_t s) {
    if (a >= b || lo >= hi) return hipSuccess;
    const uint64_t blocks = (b - a + GATHER_WAVES - 1) / GATHER_WAVES;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sort_gather, dim3((uint32_t)blocks), dim3(BT), 0, s, addr, perm, soff, a, b, lo, hi, out);
    return hipGetLastError();
}

} // namespace ngsq
