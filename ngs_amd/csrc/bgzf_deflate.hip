// bgzf_deflate.hip -- the device DEFLATE encoder.  One workgroup per BGZF block of at most 65280 input
// bytes, block after block from a counter as the inflater's decoders take them:
//   (0) the block's byte histogram gives the literal cost (bits per byte) that a match has to beat;
//   (1) match candidates, every position in parallel, in tiles of the workgroup's width: the position hashes its next four bytes
//       into an LDS table of last positions -- all lanes read, a barrier, all lanes update with atomicMax, so the table after a
//       tile does not depend on the order of the lanes -- and looks at two candidates, the table's and p - 1 (every run);
//       each is verified and extended eight bytes at a time, (length, distance) per position is kept (LDS, global scratch);
//   (2) the greedy parse, the serial part: tokens do not span a 4 KiB tile edge (matches are cut there, but still point
//       across it), so the sixteen tiles of a block are walked by sixteen lanes; token starts become a bitmask, then every
//       position tallies its token's symbols into LDS histograms;
//   (3) code lengths limited to 15 bits (a rank sort by the workgroup, then the in-place minimum-redundancy lengths of Moffat and
//       Katajainen and the Kraft-sum repair as miniz applies them, one lane per alphabet), canonical codes, the code-length code
//       (7 bits) the same way; the header lists the 286 + 30 lengths plainly;
//   (4) the exact size from the histograms: a block whose dynamic coding is not smaller than its stored form is left stored;
//   (5) emit: an exclusive scan of the tokens' bit lengths, every lane ORs its token (at most 48 bits) into the zeroed staging
//       words in LDS (the hash table's memory), which then leave for the block's staging area;
// k_deflate_crc computes the blocks' CRC32 (bgzf_crc.h), the ingest's scan turns the member sizes into offsets, and k_deflate_pack
// writes header, payload and trailer contiguously.  Nothing depends on the grid or on the order of arrival: the same input gives
// the same bytes.
// High effort (k_bgzf_deflate<true>) changes (1) and (2): the table is updated wave by wave, so that a position
// sees its own tile; what a position reads there links it to the previous position of its hash, and several candidates are
// walked along the links; the parse looks one position ahead before it takes a short match.  The block is sized both ways and the
// smaller parse is emitted.  Normal effort (k_bgzf_deflate<false>) is the encoder as it was, to the byte.
#include <hip/hip_runtime.h>

#include "bgzf_crc.h"
#include "deflate_kernels.h"

namespace ngsq {

namespace {

constexpr uint32_t DEF_THREADS = 512;
constexpr uint32_t DEF_WAVES = DEF_THREADS / 64;
constexpr uint32_t HASH_BITS = 14;
constexpr uint32_t PARSE_TILE = 4096;
constexpr uint32_t MIN_MATCH = 4, MAX_MATCH = 258, MAX_DIST = 32768;
// high effort: a match of LAZY_BELOW bytes or more is taken at once, a shorter one waits for the look at the
// next position (zlib's max_lazy).  (The candidates a position walks along its hash chain: DEFLATE_CHAIN_K, deflate_kernels.h.)
constexpr uint32_t LAZY_BELOW = 32;
// alphabets inside the unified symbol arrays: literal/length at 0 (286), distance at 288 (30), code lengths at 320 (19)
constexpr uint32_t A_LL = 0, A_D = 288, A_CL = 320, A_END = 340;
constexpr uint32_t N_LL = 286, N_D = 30, N_CL = 19;
constexpr uint32_t HDR_FIXED_BITS = 3 + 5 + 5 + 4 + 19 * 3;

struct DLds {
    union {
        uint32_t hash[1u << HASH_BITS];      // last position + 1 of a hash value (0: none)
        unsigned long long stage[8192];      // the payload's bits, after the parse
    } u;
    uint8_t len8[65536];                     // match length - 3 at every position (0: none)
    uint32_t mask[2048];                     // token starts
    uint32_t bhist[256];
    uint32_t hist[A_END];
    uint16_t code[A_END];                    // canonical codes, bit-reversed
    uint8_t clen[A_END];
    uint32_t key[3][288];
    uint16_t sym[3][288];
    uint32_t numc[3][34];
    uint32_t first[3][16];
    uint32_t nused[3];
    uint32_t wsum[DEF_WAVES];
    uint32_t total_bits, tokens, matches, ticket;
};

__device__ __forceinline__ uint64_t ld64u(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// bytes a[0, maxlen) and b[0, maxlen) have in common from the start; reads up to 7 bytes past a + maxlen (DEFLATE_IN_SLACK)
__device__ __forceinline__ uint32_t match_len(const uint8_t *a, const uint8_t *b, uint32_t maxlen) {
    uint32_t i = 0;
    while (i < maxlen) {
        const uint64_t x = ld64u(a + i) ^ ld64u(b + i);
        if (x) {
            i += (uint32_t)__builtin_ctzll(x) >> 3;
            break;
        }
        i += 8;
    }
    return i < maxlen ? i : maxlen;
}

__device__ __forceinline__ uint32_t ilog2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }
// length 3..258 -> index of its code (symbol 257 + index), extra bits and their value
__device__ __forceinline__ void len_code(uint32_t len, uint32_t *idx, uint32_t *eb, uint32_t *ev) {
    const uint32_t l = len - 3u;
    if (len == 258u) {
        *idx = 28, *eb = 0, *ev = 0;
    } else if (l < 8u) {
        *idx = l, *eb = 0, *ev = 0;
    } else {
        const uint32_t k = ilog2(l), e = k - 2u;
        *idx = 4u * (k - 1u) + ((l >> e) & 3u), *eb = e, *ev = l & ((1u << e) - 1u);
    }
}
// distance 1..32768 -> its code, extra bits and their value
__device__ __forceinline__ void dist_code(uint32_t d, uint32_t *idx, uint32_t *eb, uint32_t *ev) {
    const uint32_t dd = d - 1u;
    if (dd < 4u) {
        *idx = dd, *eb = 0, *ev = 0;
    } else {
        const uint32_t k = ilog2(dd), e = k - 1u;
        *idx = 2u * k + ((dd >> e) & 1u), *eb = e, *ev = dd & ((1u << e) - 1u);
    }
}
__device__ __forceinline__ uint32_t ll_extra_bits(uint32_t s) { return s < 265u || s == 285u ? 0u : (s - 261u) >> 2; }
__device__ __forceinline__ uint32_t d_extra_bits(uint32_t k) { return k < 4u ? 0u : (k >> 1) - 1u; }

// exclusive prefix sum of v over the workgroup; *total = the sum.  Two barriers.
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *wsum, uint32_t tid, uint32_t *total) {
    const uint32_t lane = tid & 63u, w = tid >> 6;
    uint32_t x = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63u) wsum[w] = x;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (uint32_t k = 0; k < DEF_WAVES; k++) {
        const uint32_t s = wsum[k];
        if (k < w) pre += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return pre + x - v;
}

// nb <= 48 bits of val at bit `off` of the zeroed staging words
__device__ __forceinline__ void put_bits(unsigned long long *stage, uint32_t off, uint64_t val, uint32_t nb) {
    if (!nb) return;
    const uint32_t q = off >> 6, sh = off & 63u;
    atomicOr(&stage[q], (unsigned long long)(val << sh));
    if (sh + nb > 64u) atomicOr(&stage[q + 1], (unsigned long long)(val >> (64u - sh)));
}

// the used symbols of an alphabet in ascending order of (count, symbol): thread i of the alphabet's n_sym threads
__device__ __forceinline__ void rank_sort(DLds &L, uint32_t a, uint32_t base, uint32_t n_sym, uint32_t i) {
    if (i >= n_sym) return;
    const uint32_t f = L.hist[base + i];
    if (!f) return;
    uint32_t r = 0;
    for (uint32_t j = 0; j < n_sym; j++) {
        const uint32_t g = L.hist[base + j];
        r += (g != 0u && (g < f || (g == f && j < i))) ? 1u : 0u;
    }
    L.key[a][r] = f;
    L.sym[a][r] = (uint16_t)i;
    atomicAdd(&L.nused[a], 1u);
}

// Code lengths of at most `limit` bits for the n used symbols that rank_sort left (one lane).  The in-place minimum-redundancy
// lengths (Moffat and Katajainen), then miniz's repair of the Kraft sum when a length passes the limit: the longest codes are
// gathered at the limit and codes are lengthened, shortest first, until the sum is one again -- a length-limited code, not a cut.
// An alphabet with fewer than two used symbols declares two codes of one bit: a complete code every reader accepts.
__device__ __noinline__ void huff_lengths(uint32_t *key, const uint16_t *sym, int n, int limit, uint32_t *numc, uint8_t *clen) {
    for (int i = 0; i < 34; i++) numc[i] = 0;
    if (n < 2) {
        const uint32_t s = n ? sym[0] : 0u;
        clen[s] = 1;
        clen[s ? 0u : 1u] = 1;
        numc[1] = 2;
        return;
    }
    key[0] += key[1];
    int root = 0, leaf = 2, next;
    for (next = 1; next < n - 1; next++) {
        if (leaf >= n || key[root] < key[leaf]) {
            key[next] = key[root];
            key[root++] = (uint32_t)next;
        } else key[next] = key[leaf++];
        if (leaf >= n || (root < next && key[root] < key[leaf])) {
            key[next] += key[root];
            key[root++] = (uint32_t)next;
        } else key[next] += key[leaf++];
    }
    key[n - 2] = 0;
    for (next = n - 3; next >= 0; next--) key[next] = key[key[next]] + 1u;
    int avbl = 1, used = 0, dpth = 0;
    root = n - 2;
    next = n - 1;
    while (avbl > 0) {
        while (root >= 0 && (int)key[root] == dpth) {
            used++;
            root--;
        }
        while (avbl > used) {
            key[next--] = (uint32_t)dpth;
            avbl--;
        }
        avbl = 2 * used;
        dpth++;
        used = 0;
    }
    for (int i = 0; i < n; i++) numc[key[i] < 33u ? key[i] : 33u]++;
    for (int i = limit + 1; i < 34; i++) {
        numc[limit] += numc[i];
        numc[i] = 0;
    }
    uint32_t total = 0;
    for (int i = limit; i > 0; i--) total += numc[i] << (limit - i);
    while (total != (1u << limit)) {
        numc[limit]--;
        for (int i = limit - 1; i > 0; i--)
            if (numc[i]) {
                numc[i]--;
                numc[i + 1] += 2;
                break;
            }
        total--;
    }
    int j = n;
    for (int i = 1; i <= limit; i++)
        for (uint32_t l = numc[i]; l > 0; l--) clen[sym[--j]] = (uint8_t)i;
}
// first canonical code of every length (one lane), from the counts huff_lengths left
__device__ __forceinline__ void first_codes(const uint32_t *numc, uint32_t *first) {
    uint32_t c = 0;
    first[0] = 0;
    for (uint32_t b = 1; b < 16; b++) {
        c = (c + (b > 1 ? numc[b - 1] : 0u)) << 1;
        first[b] = c;
    }
}
// the canonical code of symbol i, bit-reversed (DEFLATE sends Huffman codes from their most significant bit)
__device__ __forceinline__ void assign_code(DLds &L, uint32_t a, uint32_t base, uint32_t n_sym, uint32_t i) {
    if (i >= n_sym) return;
    const uint32_t l = L.clen[base + i];
    if (!l) return;
    uint32_t c = L.first[a][l];
    for (uint32_t j = 0; j < i; j++) c += L.clen[base + j] == l ? 1u : 0u;
    L.code[base + i] = (uint16_t)(__builtin_bitreverse32(c) >> (32u - l));
}

// Steps (0) to (4) of one block: the tokens of in[0, n) (L.mask, L.len8, dist), their codes, and the bits of the dynamic block,
// which is the value.  HIGH searches harder in (1) and (2): the table is updated wave by wave, so that a position sees the
// positions of its own tile; the value a position reads there is its link to the previous position of the same hash (`link`,
// position + 1, 0: none), and DEFLATE_CHAIN_K candidates are walked along the links; the parse looks one position ahead.  Everything
// the steps read of L they have written: a block may be taken through them more than once.
template <bool HIGH>
__device__ __forceinline__ uint32_t deflate_tokens(DLds &L, const uint8_t *__restrict__ in, uint32_t n, uint16_t *__restrict__ dist,
                                                   uint16_t *link) {
    const uint32_t tid = threadIdx.x;
    // ---- (0) clear; the byte histogram and the literal cost
    for (uint32_t k = tid; k < (1u << HASH_BITS); k += DEF_THREADS) L.u.hash[k] = 0;
    for (uint32_t k = tid; k < 2048u; k += DEF_THREADS) L.mask[k] = 0;
    if (tid < 256u) L.bhist[tid] = 0;
    if (tid < A_END) {
        L.hist[tid] = 0;
        L.code[tid] = 0;
        L.clen[tid] = 0;
    }
    if (tid < 3u) L.nused[tid] = 0;
    if (tid == 0) {
        L.total_bits = 0;
        L.tokens = 0;
        L.matches = 0;
    }
    __syncthreads();
    for (uint32_t p = tid; p < n; p += DEF_THREADS) atomicAdd(&L.bhist[in[p]], 1u);
    __syncthreads();
    if (tid < 256u) {
        const uint32_t c = L.bhist[tid];
        // (integer partial sums: the order of the additions must not matter)
        if (c) atomicAdd(&L.total_bits, (uint32_t)((float)c * __log2f((float)n / (float)c) * 16.f));
    }
    __syncthreads();
    // bits per literal, in sixteenths; a literal costs one bit at least
    uint32_t hq = L.total_bits / n;
    hq = hq < 16u ? 16u : hq;
    __syncthreads();
    if (tid == 0) L.total_bits = 0;

    // ---- (1) match candidates
    for (uint32_t t0 = 0; t0 < n; t0 += DEF_THREADS) {
        const uint32_t p = t0 + tid;
        const bool act = p + MIN_MATCH <= n;
        uint32_t w = 0, h = 0, cand = 0;
        if (act) {
            w = ld32u(in + p);
            h = (w * 2654435761u) >> (32u - HASH_BITS);
            if (!HIGH) cand = L.u.hash[h];
        }
        if (HIGH) {
            // the waves take turns: all lanes of a wave read, then all update, so the table after a turn depends on the
            // positions alone, and a wave sees every position of the waves before it
            for (uint32_t turn = 0; turn < DEF_WAVES; turn++) {
                if ((tid >> 6) == turn && act) {
                    cand = L.u.hash[h];
                    link[p] = (uint16_t)cand;
                    atomicMax(&L.u.hash[h], p + 1u);
                }
                __syncthreads();
            }
        } else {
            __syncthreads();
            if (act) atomicMax(&L.u.hash[h], p + 1u);
        }
        uint32_t best_len = 0, best_d = 1;
        if (act) {
            const uint32_t maxlen = n - p < MAX_MATCH ? n - p : MAX_MATCH;
            int best_gain = 0;
            if (p >= 1u) {
                const uint32_t l = match_len(in + p, in + p - 1u, maxlen);
                const int gain = (int)(l * hq) - 12 * 16;
                if (l >= MIN_MATCH && gain > 0) best_len = l, best_d = 1, best_gain = gain;
            }
            if (!HIGH && cand) {
                const uint32_t c = cand - 1u, d = p - c; // (c is of an earlier tile: c < t0 <= p)
                if (d >= 2u && d <= MAX_DIST && ld32u(in + c) == w) {
                    const uint32_t l = match_len(in + p, in + c, maxlen);
                    const uint32_t de = d <= 4u ? 0u : ilog2(d - 1u) - 1u;
                    const int gain = (int)(l * hq) - (int)(12u + de) * 16;
                    if (l >= MIN_MATCH && gain > best_gain) best_len = l, best_d = d, best_gain = gain;
                }
            }
            if (HIGH) {
                // Along the links, nearest first (c is of an earlier wave's turn: c < p; links only go further back).  A distance
                // costs no less than a nearer one, so only a longer match can gain more than the best so far: a candidate
                // that differs at the byte behind the best length is not extended, and nothing is longer than maxlen.
                uint32_t next = cand;
                for (uint32_t k = 0; k < DEFLATE_CHAIN_K && next && best_len < maxlen; k++) {
                    const uint32_t c = next - 1u, d = p - c;
                    if (d > MAX_DIST) break;
                    if (d >= 2u && ld32u(in + c) == w && in[c + best_len] == in[p + best_len]) {
                        const uint32_t l = match_len(in + p, in + c, maxlen);
                        const uint32_t de = d <= 4u ? 0u : ilog2(d - 1u) - 1u;
                        const int gain = (int)(l * hq) - (int)(12u + de) * 16;
                        if (l >= MIN_MATCH && gain > best_gain) best_len = l, best_d = d, best_gain = gain;
                    }
                    next = link[c];
                }
            }
        }
        if (p < n) {
            L.len8[p] = (uint8_t)(best_len ? best_len - 3u : 0u);
            dist[p] = (uint16_t)(best_d - 1u);
        }
        __syncthreads();
    }

    // ---- (2) the parse, greedy (at high effort with the lazy step): one lane per 4 KiB tile
    const uint32_t n_tiles = (n + PARSE_TILE - 1u) / PARSE_TILE;
    if (tid < n_tiles) {
        uint32_t p = tid * PARSE_TILE;
        const uint32_t end = p + PARSE_TILE < n ? p + PARSE_TILE : n;
        uint32_t cur = p >> 5, bits = 0;
        while (p < end) {
            const uint32_t wi = p >> 5;
            if (wi != cur) {
                L.mask[cur] = bits;
                bits = 0;
                cur = wi;
            }
            bits |= 1u << (p & 31u);
            const uint32_t v = L.len8[p];
            uint32_t len = v ? v + 3u : 0u;
            if (len > end - p) { // cut at the tile's edge; a rest below the minimum is a literal
                len = end - p >= MIN_MATCH ? end - p : 0u;
                L.len8[p] = (uint8_t)(len ? len - 3u : 0u);
            }
            if (HIGH && len && len < LAZY_BELOW && p + 1u < end) {
                // The lazy step: a longer match at p + 1 makes p a literal.  Both lengths are the cut ones, and p + 1 is of this
                // lane's tile: a match the edge has cut reaches the edge, and none at p + 1 reaches further.
                const uint32_t v1 = L.len8[p + 1u];
                uint32_t l1 = v1 ? v1 + 3u : 0u;
                l1 = l1 < end - p - 1u ? l1 : end - p - 1u;
                if (l1 > len) {
                    len = 0;
                    L.len8[p] = 0;
                }
            }
            p += len ? len : 1u;
        }
        L.mask[cur] = bits;
    }
    __syncthreads();
    // the tokens' symbols
    for (uint32_t p = tid; p < n; p += DEF_THREADS) {
        if (!((L.mask[p >> 5] >> (p & 31u)) & 1u)) continue;
        const uint32_t v = L.len8[p];
        if (!v) {
            atomicAdd(&L.hist[A_LL + in[p]], 1u);
        } else {
            uint32_t li, le, lv, di, de, dv;
            len_code(v + 3u, &li, &le, &lv);
            dist_code((uint32_t)dist[p] + 1u, &di, &de, &dv);
            atomicAdd(&L.hist[A_LL + 257u + li], 1u);
            atomicAdd(&L.hist[A_D + di], 1u);
        }
    }
    if (tid == 0) L.hist[A_LL + 256u] = 1;
    __syncthreads();

    // ---- (3) code lengths and codes: literal/length by threads [0, 286), distance by threads [320, 350)
    rank_sort(L, 0, A_LL, N_LL, tid);
    rank_sort(L, 1, A_D, N_D, tid - 320u);
    __syncthreads();
    if (tid == 0) {
        huff_lengths(L.key[0], L.sym[0], (int)L.nused[0], 15, L.numc[0], L.clen + A_LL);
        first_codes(L.numc[0], L.first[0]);
    }
    if (tid == 320u) {
        huff_lengths(L.key[1], L.sym[1], (int)L.nused[1], 15, L.numc[1], L.clen + A_D);
        first_codes(L.numc[1], L.first[1]);
    }
    __syncthreads();
    assign_code(L, 0, A_LL, N_LL, tid);
    assign_code(L, 1, A_D, N_D, tid - 320u);
    // the code-length code over the 316 lengths the header lists
    if (tid < N_LL) atomicAdd(&L.hist[A_CL + L.clen[A_LL + tid]], 1u);
    else if (tid >= 320u && tid < 320u + N_D) atomicAdd(&L.hist[A_CL + L.clen[A_D + tid - 320u]], 1u);
    __syncthreads();
    rank_sort(L, 2, A_CL, N_CL, tid);
    __syncthreads();
    if (tid == 0) {
        huff_lengths(L.key[2], L.sym[2], (int)L.nused[2], 7, L.numc[2], L.clen + A_CL);
        first_codes(L.numc[2], L.first[2]);
    }
    __syncthreads();
    assign_code(L, 2, A_CL, N_CL, tid);

    // ---- (4) the exact size
    {
        uint32_t bits = 0, tok = 0, mat = 0;
        if (tid < N_LL) {
            const uint32_t c = L.hist[tid], l = L.clen[tid];
            bits = c * (l + ll_extra_bits(tid)) + L.clen[A_CL + l];
            if (tid != 256u) tok = c;
            if (tid > 256u) mat = c;
        } else if (tid >= A_D && tid < A_D + N_D) {
            const uint32_t c = L.hist[tid], l = L.clen[tid];
            bits = c * (l + d_extra_bits(tid - A_D)) + L.clen[A_CL + l];
        }
        if (bits) atomicAdd(&L.total_bits, bits);
        if (tok) atomicAdd(&L.tokens, tok);
        if (mat) atomicAdd(&L.matches, mat);
    }
    __syncthreads();
    return HDR_FIXED_BITS + L.total_bits;
}

// One block: in[0, n) -> its DEFLATE payload at `stage` (dynamic) or nothing (stored); the payload's bytes and the flag.  At high
// effort the block is sized both ways before a bit is written, and the smaller parse is the one emitted (the high one when they
// are equal): a block is never larger than at normal effort.
template <bool HIGH>
__device__ void deflate_block(DLds &L, const uint8_t *__restrict__ in, uint32_t n, uint16_t *__restrict__ dist, uint16_t *link,
                              unsigned long long *__restrict__ stage, uint64_t *__restrict__ size_out, uint32_t *__restrict__ flag_out,
                              unsigned long long *__restrict__ work) {
    const uint32_t tid = threadIdx.x;
    uint32_t total_bits;
    if (HIGH) {
        const uint32_t normal_bits = deflate_tokens<false>(L, in, n, dist, link);
        __syncthreads(); // (the sum has been read before the next pass clears it)
        total_bits = deflate_tokens<true>(L, in, n, dist, link);
        if (normal_bits < total_bits) { // (uniform)
            __syncthreads();
            total_bits = deflate_tokens<false>(L, in, n, dist, link);
        }
    } else {
        total_bits = deflate_tokens<false>(L, in, n, dist, link);
    }
    const uint32_t dyn_bytes = (total_bits + 7u) / 8u, stored_bytes = n + DEFLATE_STORED_EXTRA;
    const bool stored = dyn_bytes >= stored_bytes;
    if (tid == 0) {
        *size_out = (uint64_t)(stored ? stored_bytes : dyn_bytes) + DEFLATE_MEMBER_EXTRA;
        *flag_out = stored ? 1u : 0u;
        if (stored) atomicAdd(&work[1], 1ull);
        atomicAdd(&work[2], (unsigned long long)(stored ? 0u : L.tokens));
        atomicAdd(&work[3], (unsigned long long)(stored ? 0u : L.matches));
    }
    if (stored) return; // (uniform)

    // ---- (5) emit into the zeroed staging words (the hash table's memory: the parse is over)
    for (uint32_t k = tid; k < 8192u; k += DEF_THREADS) L.u.stage[k] = 0;
    __syncthreads();
    if (tid == 0) {
        // BFINAL 1, BTYPE 2, HLIT 29 (286 codes), HDIST 29 (30 codes), HCLEN 15 (19 lengths), then the 19 lengths of three bits
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        put_bits(L.u.stage, 0, 1u | 2u << 1 | 29u << 3 | 29u << 8 | 15u << 13, 17);
        uint32_t off = 17;
        for (uint32_t k = 0; k < 19; k++, off += 3) put_bits(L.u.stage, off, L.clen[A_CL + order[k]], 3);
    }
    uint32_t base = HDR_FIXED_BITS;
    {
        // the 316 code lengths, each as its code-length code
        uint32_t nb = 0, val = 0;
        if (tid < N_LL + N_D) {
            const uint32_t l = L.clen[tid < N_LL ? tid : A_D + tid - N_LL];
            nb = L.clen[A_CL + l];
            val = L.code[A_CL + l];
        }
        uint32_t tot;
        const uint32_t off = block_excl_scan(nb, L.wsum, tid, &tot);
        put_bits(L.u.stage, base + off, val, nb);
        base += tot;
    }
    for (uint32_t t0 = 0; t0 < n; t0 += DEF_THREADS) {
        const uint32_t p = t0 + tid;
        uint32_t nb = 0;
        uint64_t val = 0;
        if (p < n && ((L.mask[p >> 5] >> (p & 31u)) & 1u)) {
            const uint32_t v = L.len8[p];
            if (!v) {
                const uint32_t s = A_LL + in[p];
                val = L.code[s];
                nb = L.clen[s];
            } else {
                uint32_t li, le, lv, di, de, dv;
                len_code(v + 3u, &li, &le, &lv);
                dist_code((uint32_t)dist[p] + 1u, &di, &de, &dv);
                const uint32_t ls = A_LL + 257u + li, ds = A_D + di;
                val = L.code[ls];
                nb = L.clen[ls];
                val |= (uint64_t)lv << nb;
                nb += le;
                val |= (uint64_t)L.code[ds] << nb;
                nb += L.clen[ds];
                val |= (uint64_t)dv << nb;
                nb += de;
            }
        }
        uint32_t tot;
        const uint32_t off = block_excl_scan(nb, L.wsum, tid, &tot);
        put_bits(L.u.stage, base + off, val, nb);
        base += tot;
    }
    if (tid == 0) put_bits(L.u.stage, base, L.code[A_LL + 256u], L.clen[A_LL + 256u]);
    __syncthreads();
    const uint32_t words = (dyn_bytes + 7u) / 8u;
    for (uint32_t k = tid; k < words; k += DEF_THREADS) stage[k] = L.u.stage[k];
}

template <bool HIGH>
__global__ __launch_bounds__(DEF_THREADS) void k_bgzf_deflate(const uint8_t *__restrict__ in, uint64_t n, uint32_t n_blocks,
                                                              uint16_t *__restrict__ dist, uint16_t *link, uint8_t *__restrict__ stage,
                                                              uint64_t *__restrict__ size, uint32_t *__restrict__ flags,
                                                              unsigned long long *__restrict__ work) {
    __shared__ DLds L;
    uint16_t *const my_dist = dist + (size_t)blockIdx.x * 65536u;
    uint16_t *const my_link = HIGH ? link + (size_t)blockIdx.x * 65536u : nullptr;
    for (;;) {
        if (threadIdx.x == 0) L.ticket = (uint32_t)atomicAdd(&work[0], 1ull);
        __syncthreads();
        const uint32_t bi = L.ticket;
        if (bi >= n_blocks) return;
        const uint64_t at = (uint64_t)bi * DEFLATE_BLOCK_INPUT;
        const uint32_t len = (uint32_t)(n - at < DEFLATE_BLOCK_INPUT ? n - at : DEFLATE_BLOCK_INPUT);
        deflate_block<HIGH>(L, in + at, len, my_dist, my_link, reinterpret_cast<unsigned long long *>(stage + (size_t)bi * DEFLATE_STAGE_STRIDE), size + bi,
                      flags + bi, work);
        __syncthreads(); // the next block's first LDS writes (the ticket among them) come after this block's last reads
    }
}

// CRC32 of every block's input bytes, one wave per block, stored for the trailer
__global__ __launch_bounds__(64 * CRC_WAVES) void k_deflate_crc(const uint8_t *__restrict__ in, uint64_t n, uint32_t n_blocks,
                                                                uint32_t *__restrict__ crc, const uint32_t *__restrict__ pow_tab) {
    __shared__ uint32_t s_tab[CRC_SLICES * 256];
    crc_load_tables(s_tab, 64 * CRC_WAVES);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t bi = blockIdx.x * CRC_WAVES + (threadIdx.x >> 6);
    if (bi >= n_blocks) return;
    const uint64_t at = (uint64_t)bi * DEFLATE_BLOCK_INPUT;
    const uint32_t len = __builtin_amdgcn_readfirstlane((uint32_t)(n - at < DEFLATE_BLOCK_INPUT ? n - at : DEFLATE_BLOCK_INPUT));
    const uint32_t c = crc_wave_block(in + at, len, lane, s_tab, pow_tab);
    if (lane == 0) crc[bi] = c;
}

// dst[0, n) = src[0, n) by the workgroup: aligned 32-bit stores, whatever the two alignments are
__device__ __forceinline__ void copy_block_bytes(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t n, uint32_t tid, uint32_t nt) {
    uint32_t head = (uint32_t)((4u - (reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u);
    head = head < n ? head : n;
    if (tid < head) dst[tid] = src[tid];
    const uint32_t body = (n - head) / 4u;
    uint32_t *const dw = reinterpret_cast<uint32_t *>(dst + head);
    for (uint32_t j = tid; j < body; j += nt) dw[j] = ld32u(src + head + 4u * j);
    const uint32_t tail0 = head + 4u * body;
    if (tail0 + tid < n) dst[tail0 + tid] = src[tail0 + tid];
}

constexpr uint32_t PACK_THREADS = 256;
// One workgroup per block: the 18-byte gzip header with the BC field and BSIZE, the payload (staged, or the stored form of the
// input), CRC32 and ISIZE at off[bi].  Block 0 also hands the host its words.
__global__ __launch_bounds__(PACK_THREADS) void k_deflate_pack(const uint8_t *__restrict__ in, uint64_t n, uint32_t n_blocks,
                                                               const uint8_t *__restrict__ stage, const uint64_t *__restrict__ off,
                                                               const uint32_t *__restrict__ flags, const uint32_t *__restrict__ crc,
                                                               uint8_t *__restrict__ out, const unsigned long long *__restrict__ work,
                                                               unsigned long long *__restrict__ host) {
    const uint32_t bi = blockIdx.x, tid = threadIdx.x;
    if (bi == 0 && tid == 0) {
        host[DH_BYTES] = off[n_blocks];
        host[DH_STORED] = work[1];
        host[DH_TOKENS] = work[2];
        host[DH_MATCHES] = work[3];
    }
    const uint64_t o = off[bi];
    const uint32_t member = (uint32_t)(off[bi + 1] - o), payload = member - DEFLATE_MEMBER_EXTRA;
    const uint64_t at = (uint64_t)bi * DEFLATE_BLOCK_INPUT;
    const uint32_t len = (uint32_t)(n - at < DEFLATE_BLOCK_INPUT ? n - at : DEFLATE_BLOCK_INPUT);
    uint8_t *const dst = out + o;
    if (tid < 18u) {
        const uint32_t bsize = member - 1u;
        const uint8_t hdr[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)(bsize & 0xFFu), (uint8_t)(bsize >> 8)};
        dst[tid] = hdr[tid];
    } else if (tid >= 32u && tid < 40u) {
        const uint32_t k = tid - 32u;
        const uint32_t v = k < 4u ? crc[bi] : len;
        dst[18u + payload + k] = (uint8_t)(v >> (8u * (k & 3u)));
    }
    if (flags[bi]) {
        if (tid >= 64u && tid < 69u) {
            const uint32_t k = tid - 64u, nl = ~len & 0xFFFFu;
            const uint8_t sh[5] = {1, (uint8_t)(len & 0xFFu), (uint8_t)(len >> 8), (uint8_t)(nl & 0xFFu), (uint8_t)(nl >> 8)};
            dst[18u + k] = sh[k];
        }
        copy_block_bytes(dst + 18u + DEFLATE_STORED_EXTRA, in + at, len, tid, PACK_THREADS);
    } else {
        copy_block_bytes(dst + 18u, stage + (size_t)bi * DEFLATE_STAGE_STRIDE, payload, tid, PACK_THREADS);
    }
}

} // namespace

hipError_t launch_bgzf_deflate(const uint8_t *in, uint64_t n, uint8_t *out, DeflateScratch &sc, unsigned long long *host, uint32_t effort,
                               hipStream_t s, hipEvent_t *ev) {
    const uint64_t nb64 = deflate_blocks(n);
    if (effort > DEFLATE_EFFORT_HIGH) return hipErrorInvalidValue;
    if (!n || nb64 > 0x7FFFFFFFull) return hipErrorInvalidValue; // (no input: no block, and nothing that would write the host's words)
    const uint32_t n_blocks = (uint32_t)nb64;
    hipError_t e;
#define DTRY(expr)                    \
    do {                              \
        e = (expr);                   \
        if (e != hipSuccess) return e; \
    } while (0)
    static int n_cu_of[64] = {};
    int dev = 0, n_cu = 0;
    DTRY(hipGetDevice(&dev));
    if (dev >= 0 && dev < 64 && n_cu_of[dev]) n_cu = n_cu_of[dev];
    else {
        DTRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
        if (dev >= 0 && dev < 64) n_cu_of[dev] = n_cu;
    }
    // one workgroup per CU is what the LDS holds
    const uint32_t grid = n_blocks < (uint32_t)n_cu ? n_blocks : (uint32_t)n_cu;
    DTRY(sc.work.reserve(4));
    DTRY(hipMemsetAsync(sc.work.p, 0, 4 * sizeof(unsigned long long), s));
    DTRY(sc.off.reserve((size_t)n_blocks + 1));
    if (ev) DTRY(hipEventRecord(ev[0], s));
    if (n_blocks) {
        DTRY(sc.stage.reserve((size_t)n_blocks * DEFLATE_STAGE_STRIDE));
        DTRY(sc.dist.reserve((size_t)grid * 65536u));
        DTRY(sc.crc.reserve(n_blocks));
        DTRY(sc.flags.reserve(n_blocks));
        if (effort == DEFLATE_EFFORT_HIGH) {
            DTRY(sc.link.reserve((size_t)grid * 65536u));
            hipLaunchKernelGGL(k_bgzf_deflate<true>, dim3(grid), dim3(DEF_THREADS), 0, s, in, n, n_blocks, sc.dist.p, sc.link.p, sc.stage.p, sc.off.p,
                               sc.flags.p, sc.work.p);
        } else {
            hipLaunchKernelGGL(k_bgzf_deflate<false>, dim3(grid), dim3(DEF_THREADS), 0, s, in, n, n_blocks, sc.dist.p, (uint16_t *)nullptr, sc.stage.p,
                               sc.off.p, sc.flags.p, sc.work.p);
        }
        DTRY(hipGetLastError());
    }
    DTRY(hipMemsetAsync(sc.off.p + n_blocks, 0, sizeof(uint64_t), s));
    if (ev) DTRY(hipEventRecord(ev[1], s));
    if (n_blocks) {
        const uint32_t *pow_tab = nullptr;
        DTRY(bgzf_crc_pow_table(&pow_tab));
        hipLaunchKernelGGL(k_deflate_crc, dim3((n_blocks + CRC_WAVES - 1) / CRC_WAVES), dim3(64 * CRC_WAVES), 0, s, in, n, n_blocks, sc.crc.p, pow_tab);
        DTRY(hipGetLastError());
    }
    if (ev) DTRY(hipEventRecord(ev[2], s));
    if (n_blocks) {
        DTRY(sc.scan.exclusive_scan(sc.off.p, (uint64_t)n_blocks + 1, s));
        hipLaunchKernelGGL(k_deflate_pack, dim3(n_blocks), dim3(PACK_THREADS), 0, s, in, n, n_blocks, sc.stage.p, sc.off.p, sc.flags.p, sc.crc.p, out,
                           sc.work.p, host);
        DTRY(hipGetLastError());
    }
    if (ev) DTRY(hipEventRecord(ev[3], s));
#undef DTRY
    return hipSuccess;
}

} // namespace ngsq
