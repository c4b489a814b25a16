// samtext_kernel.hip -- `ngs convert --gzip device <SAM> <BAM>` on the device: the BAM record of every
// line of a chunk of SAM text.  The line starts come from a count of the newlines per tile, the ingest's exclusive scan and a
// scatter.  Then one wave per line in both passes: the sizing pass walks the line as the write pass does and only validates
// and counts, so the two agree by construction; the offsets between them come from the same scan.  Inside a line the wave
// spreads what is long across its lanes -- the tabs, CIGAR operations, SEQ and QUAL bytes, Z/H bytes, B array elements -- so
// that a 100 kb read or a 70 000-operation CIGAR costs its own wave some more steps, not one thread the whole chunk.
// samtext.cpp drives them, hands the records to the device DEFLATE encoder and writes its blocks.
#include <hip/hip_runtime.h>

#include "samtext_kernels.h"

namespace ngsq {

namespace {

constexpr uint32_t BT = 256; // threads per block: four lines
constexpr uint32_t LINES_PER_BLOCK = BT / 64;
constexpr uint32_t FLOAT_BLOCKS = 1024; // grid of the kernels over the lines that hold a float (grid-stride)
constexpr uint32_t TILE_PER_THREAD = ST_TILE / BT; // 16 bytes: one aligned load

__host__ __device__ inline uint32_t fnv1a(const uint8_t *p, uint64_t n) {
    uint32_t h = 2166136261u;
    for (uint64_t k = 0; k < n; k++) h = (h ^ p[k]) * 16777619u;
    return h;
}

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ void st32(uint8_t *p, uint32_t v) { __builtin_memcpy(p, &v, 4); }
__device__ __forceinline__ void st16(uint8_t *p, uint32_t v) {
    const uint16_t x = (uint16_t)v;
    __builtin_memcpy(p, &x, 2);
}
__device__ __forceinline__ bool is_digit(uint32_t c) { return c - '0' <= 9u; }

// inclusive prefix sum over the wave
__device__ __forceinline__ uint32_t wave_incl(uint32_t v) {
    const uint32_t lane = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(v, d, 64);
        if (lane >= (uint32_t)d) v += y;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, (uint32_t)__shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d, 64);
    return v;
}
// lanes below this one among the set bits of m
__device__ __forceinline__ uint32_t rank_in(uint64_t m) { return (uint32_t)__popcll(m & ((1ull << lane_id()) - 1ull)); }

// ---- line starts ---------------------------------------------------------------------------------------------------------

// the newlines among a thread's 16 bytes of its tile, as a bit mask (byte j of the group = bit j); the buffer is readable
// ST_TEXT_SLACK bytes past `bytes`
__device__ __forceinline__ uint32_t newline_mask(const uint8_t *text, uint64_t at, uint64_t bytes) {
    if (at >= bytes) return 0;
    const uint4 v = *reinterpret_cast<const uint4 *>(text + at); // (at is a multiple of 16, the buffer a device allocation)
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 16; j++)
        if (((w[j >> 2] >> (8 * (j & 3))) & 255u) == '\n') m |= 1u << j;
    const uint64_t left = bytes - at;
    return left >= 16 ? m : m & ((1u << left) - 1u);
}

__global__ __launch_bounds__(BT) void k_st_count(const uint8_t *__restrict__ text, uint64_t bytes, uint64_t *__restrict__ tile_cnt, uint64_t tiles) {
    __shared__ uint32_t total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const uint64_t at = (uint64_t)blockIdx.x * ST_TILE + (uint64_t)threadIdx.x * TILE_PER_THREAD;
    uint32_t c = (uint32_t)__popc(newline_mask(text, at, bytes));
    c = wave_incl(c);
    if (lane_id() == 63 && c) atomicAdd(&total, c);
    __syncthreads();
    if (threadIdx.x == 0) {
        tile_cnt[blockIdx.x] = total;
        if (blockIdx.x == 0) tile_cnt[tiles] = 0;
    }
}

__global__ __launch_bounds__(BT) void k_st_scatter(const uint8_t *__restrict__ text, uint64_t bytes, const uint64_t *__restrict__ tile_off, uint64_t cap,
                                                   uint64_t *__restrict__ start) {
    __shared__ uint32_t wave_total[BT / 64];
    const uint64_t at = (uint64_t)blockIdx.x * ST_TILE + (uint64_t)threadIdx.x * TILE_PER_THREAD;
    uint32_t m = newline_mask(text, at, bytes);
    const uint32_t c = (uint32_t)__popc(m), incl = wave_incl(c);
    if (lane_id() == 63) wave_total[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint64_t idx = tile_off[blockIdx.x] + (incl - c);
    for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) idx += wave_total[w];
    for (; m; m &= m - 1, idx++)
        if (idx < cap) start[idx + 1] = at + (uint32_t)(__ffs(m) - 1) + 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) start[0] = 0;
}

__global__ void k_st_word(const uint64_t *__restrict__ v, uint64_t n, unsigned long long *host) {
    if (threadIdx.x == 0) host[0] = v[n];
}

// ---- numbers -------------------------------------------------------------------------------------------------------------

// the decimal number t[b, e) (neg_ok: a leading '-' is taken); false: empty or not digits.  The value saturates above 2^40.
__device__ bool parse_dec(const uint8_t *t, uint64_t b, uint64_t e, bool neg_ok, int64_t *out) {
    bool neg = false;
    if (neg_ok && b < e && t[b] == '-') {
        neg = true;
        b++;
    }
    if (b >= e) return false;
    uint64_t v = 0;
    for (uint64_t k = b; k < e; k++) {
        const uint32_t d = (uint32_t)t[k] - '0';
        if (d > 9u) return false;
        if (v < (1ull << 40)) v = v * 10 + d;
    }
    *out = neg ? -(int64_t)v : (int64_t)v;
    return true;
}

// ---- f32 values: Rust's f32::from_str, exactly ----------------------------------------------------
// 576-bit unsigned integers, little-endian limbs.  A text of at most 48 characters holds a decimal D < 10^48 < 2^160 and an
// exponent q; D 10^q is compared with n 2^e (n < 2^25, -151 <= e <= 105) after both are made integers, which takes at most
// 5^94 n 2^199 < 2^443 on one side and 2^160 2^190 on the other.
constexpr int BIG_LIMBS = 18;
struct BigF {
    uint32_t w[BIG_LIMBS];
};
__host__ __device__ inline void bf_set(BigF &a, uint32_t v) {
    for (int k = 0; k < BIG_LIMBS; k++) a.w[k] = 0;
    a.w[0] = v;
}
__host__ __device__ inline void bf_mul_add(BigF &a, uint32_t m, uint32_t add) {
    uint64_t c = add;
    for (int k = 0; k < BIG_LIMBS; k++) {
        c += (uint64_t)a.w[k] * m;
        a.w[k] = (uint32_t)c;
        c >>= 32;
    }
}
__host__ __device__ inline void bf_pow5(BigF &a, int n) {
    for (; n >= 13; n -= 13) bf_mul_add(a, 1220703125u, 0); // 5^13
    uint32_t m = 1;
    for (; n > 0; n--) m *= 5;
    bf_mul_add(a, m, 0);
}
__host__ __device__ inline void bf_shl(BigF &a, int s) {
    const int wq = s >> 5, bq = s & 31;
    for (int k = BIG_LIMBS - 1; k >= 0; k--) {
        const uint32_t hi = k - wq >= 0 ? a.w[k - wq] : 0u, lo = k - wq - 1 >= 0 ? a.w[k - wq - 1] : 0u;
        a.w[k] = bq ? (hi << bq | lo >> (32 - bq)) : hi;
    }
}
__host__ __device__ inline int bf_cmp(const BigF &a, const BigF &b) {
    for (int k = BIG_LIMBS - 1; k >= 0; k--)
        if (a.w[k] != b.w[k]) return a.w[k] < b.w[k] ? -1 : 1;
    return 0;
}
__host__ __device__ inline int bf_bits(const BigF &a) {
    for (int k = BIG_LIMBS - 1; k >= 0; k--)
        if (a.w[k]) {
            int b = 32;
            while (!(a.w[k] >> (b - 1))) b--;
            return 32 * k + b;
        }
    return 0;
}
// sign of A 2^q - B n 2^e
__host__ __device__ inline int cmp_scaled(const BigF &A, int q, const BigF &B, uint32_t n, int e) {
    BigF x = A, y = B;
    bf_mul_add(y, n, 0);
    if (q > e) bf_shl(x, q - e);
    else bf_shl(y, e - q);
    return bf_cmp(x, y);
}
__host__ __device__ inline bool word_is(const uint8_t *p, uint32_t n, const char *w, uint32_t wn) {
    if (n != wn) return false;
    for (uint32_t k = 0; k < n; k++)
        if ((p[k] | 0x20u) != (uint8_t)w[k]) return false;
    return true;
}

// THE float parser of the SAM text (`f` tags and B:f elements): the bits of the f32 that Rust's f32::from_str gives
// p[0, n), n <= ST_FLOAT_TEXT_MAX -- a decimal with optional fraction and exponent, or inf / infinity / nan in any case, each
// with an optional sign; the value rounded to nearest, ties to even, overflow to infinity, underflow through the denormals to
// zero.  false: not a float.  The positive floats are ordered as their bit patterns, so the pattern is found by bisection
// with exact comparisons, and rounded by one more against the midpoint to the next pattern.
__host__ __device__ inline uint32_t dig(uint8_t c) { return (uint32_t)c - (uint32_t)'0'; }
__host__ __device__ __attribute__((noinline)) bool parse_f32(const uint8_t *p, uint32_t n, uint32_t *out) {
    uint32_t i = 0, sign = 0;
    if (n && (p[0] == '+' || p[0] == '-')) {
        sign = p[0] == '-' ? 0x80000000u : 0u;
        i = 1;
    }
    if (i >= n) return false;
    if (word_is(p + i, n - i, "inf", 3) || word_is(p + i, n - i, "infinity", 8)) {
        *out = sign | 0x7F800000u;
        return true;
    }
    if (word_is(p + i, n - i, "nan", 3)) {
        *out = sign | 0x7FC00000u;
        return true;
    }
    BigF D;
    bf_set(D, 0);
    bool any = false;
    int frac = 0;
    for (; i < n && dig(p[i]) <= 9u; i++, any = true) bf_mul_add(D, 10, dig(p[i]));
    if (i < n && p[i] == '.')
        for (i++; i < n && dig(p[i]) <= 9u; i++, any = true, frac++) bf_mul_add(D, 10, dig(p[i]));
    if (!any) return false;
    int ex = 0;
    if (i < n && (p[i] | 0x20) == 'e') {
        i++;
        bool eneg = false;
        if (i < n && (p[i] == '+' || p[i] == '-')) eneg = p[i++] == '-';
        if (i >= n || dig(p[i]) > 9u) return false;
        for (; i < n && dig(p[i]) <= 9u; i++)
            if (ex < 100000) ex = ex * 10 + (int)dig(p[i]);
        if (eneg) ex = -ex;
    }
    if (i != n) return false;
    const int q = ex - frac, bits = bf_bits(D);
    if (!bits) {
        *out = sign;
        return true;
    }
    // 2^(bits - 1) 10^q <= V < 2^bits 10^q, log2(10) in (3.321, 3.322): out of the floats' range without arithmetic
    const long lo_mb = (long)(bits - 1) * 1000 + (long)q * (q >= 0 ? 3321 : 3322), hi_mb = (long)bits * 1000 + (long)q * (q >= 0 ? 3322 : 3321);
    if (lo_mb >= 129000) { // V >= 2^129
        *out = sign | 0x7F800000u;
        return true;
    }
    if (hi_mb <= -151000) { // V < 2^-151, under half the smallest denormal
        *out = sign;
        return true;
    }
    BigF A = D, B;
    bf_set(B, 1);
    if (q >= 0) bf_pow5(A, q);
    else bf_pow5(B, -q);
    // value(u) = m 2^e, which reads 2^128 for the pattern of infinity
    uint32_t lo = 0, hi = 0x7F800001u;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2, mex = mid >> 23, mfr = mid & 0x7FFFFFu;
        const uint32_t m = mex ? (mfr | 0x800000u) : mfr;
        const int e = mex ? (int)mex - 150 : -149;
        if (cmp_scaled(A, q, B, m, e) >= 0) lo = mid;
        else hi = mid;
    }
    if (lo < 0x7F800000u) {
        const uint32_t lex = lo >> 23, lfr = lo & 0x7FFFFFu;
        const uint32_t m = lex ? (lfr | 0x800000u) : lfr;
        const int e = lex ? (int)lex - 150 : -149;
        const int c = cmp_scaled(A, q, B, 2 * m + 1, e - 1);
        if (c > 0 || (c == 0 && (lo & 1u))) lo++;
    }
    *out = sign | lo;
    return true;
}

// ---- one line's record, by one wave --------------------------------------------------------------------------------------

__device__ __forceinline__ void fault(uint32_t *err, uint32_t code) { *err = min(*err, code); }

// nibble of a SEQ letter (either case), 16: none.  The letters' codes sit in two words, four bits per letter from 'a'.
__device__ __forceinline__ uint32_t seq_code(uint32_t c) {
    if (c == '=') return 0;
    const uint32_t u = (c | 0x20u) - 'a';
    if (u >= 26u) return 16;
    const uint32_t v = u < 16u ? (uint32_t)(0x00F30C00B400D2E1ull >> (4 * u)) & 15u : (uint32_t)(0x0A09708650ull >> (4 * (u - 16))) & 15u;
    return v ? v : 16;
}
__device__ __forceinline__ uint32_t reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26));
    return 0;
}
__device__ __forceinline__ uint32_t b_width(uint8_t sub) {
    return sub == 'c' || sub == 'C' ? 1u : sub == 's' || sub == 'S' ? 2u : sub == 'i' || sub == 'I' || sub == 'f' ? 4u : 0u;
}

// the reference id of the name t[b, e): -1 for `*`; *ok = false for a name the header does not hold.  The whole wave.
__device__ int32_t ref_lookup(const uint8_t *t, uint64_t b, uint64_t e, const SamTextRefs &R, bool *ok) {
    const uint64_t n = e - b;
    if (n == 1 && t[b] == '*') return -1;
    if (R.n_refs) {
        uint32_t s = fnv1a(t + b, n) & (R.slots - 1);
        for (uint32_t probes = 0; probes < R.slots; probes++, s = (s + 1) & (R.slots - 1)) {
            const uint32_t v = R.table[s];
            if (!v) break;
            const uint64_t a = R.name_off[v - 1];
            if (R.name_off[v] - a != n) continue;
            bool same = true;
            for (uint64_t c0 = 0; c0 < n && same; c0 += 64) {
                const uint64_t k = c0 + lane_id();
                if (__ballot(k < n && R.names[a + k] != t[b + k])) same = false;
            }
            if (same) return (int32_t)(v - 1);
        }
    }
    *ok = false;
    return -1;
}

// The CIGAR t[b, e) (not `*`), 64 bytes at a time: a ballot of the letters, each letter's lane reads the digits in front of
// it.  W: operation k goes to dst + 4 k.  Returns the reference bases the operations span.
template <bool W> __device__ uint64_t cigar_ops(const uint8_t *t, uint64_t b, uint64_t e, uint8_t *dst, uint32_t *err) {
    uint64_t base = 0, span = 0;
    for (uint64_t c0 = b; c0 < e; c0 += 64) {
        const uint64_t k = c0 + lane_id();
        const bool letter = k < e && !is_digit(t[k]);
        const uint64_t m = __ballot(letter);
        uint64_t mine = 0;
        if (letter) {
            uint64_t j = k;
            while (j > b && is_digit(t[j - 1])) j--;
            if (j == k) fault(err, ST_E_CIGAR_DIGITS);
            uint32_t v = 0;
            for (; j < k; j++)
                if (v < (1u << 28)) v = v * 10 + (t[j] - '0');
            if (v >= (1u << 28)) fault(err, ST_E_CIGAR_LEN);
            const uint8_t c = t[k];
            const uint32_t op = c == 'M' ? 0u : c == 'I' ? 1u : c == 'D' ? 2u : c == 'N' ? 3u : c == 'S' ? 4u : c == 'H' ? 5u : c == 'P' ? 6u : c == '=' ? 7u : c == 'X' ? 8u : 9u;
            if (op > 8u) fault(err, ST_E_CIGAR_OP);
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) mine = v;
            if (W) st32(dst + 4 * (base + rank_in(m)), v << 4 | op);
        }
        span += wave_sum64(mine);
        base += (uint64_t)__popcll(m);
    }
    return span;
}

// The BAM record of the line t[0, n), by the whole wave: every lane returns its length (block_size
// included); W writes it at dst.  *err (the lane's own, ~0u on entry): the smallest SamTextError met; left at ~0u if none.
// F: the f32 values are parsed (parse_f32 needs several times the registers of the rest: the kernels without F only mark
// the rare line that holds a float, *has_float, whose values then are not written; the F kernels redo those lines).
template <bool W, bool F>
__device__ uint64_t st_line(const uint8_t *t, uint64_t n, const SamTextRefs &R, uint8_t *dst, uint32_t *err, bool *has_float) {
    const uint32_t lane = lane_id();
    // the first eleven tabs: lane k keeps tab k
    unsigned long long tabv = n;
    uint32_t found = 0;
    for (uint64_t c0 = 0; c0 < n && found < 11; c0 += 64) {
        const uint64_t k = c0 + lane;
        uint64_t m = __ballot(k < n && t[k] == '\t');
        for (; m && found < 11; m &= m - 1, found++)
            if (lane == found) tabv = c0 + (uint64_t)(__ffsll((unsigned long long)m) - 1);
    }
    if (found < 10) {
        fault(err, ST_E_FIELDS);
        return 0;
    }
    uint64_t fb[11], fe[11]; // the fields' bounds
    fb[0] = 0;
#pragma unroll
    for (int f = 0; f < 10; f++) {
        fe[f] = __shfl(tabv, f, 64);
        fb[f + 1] = fe[f] + 1;
    }
    fe[10] = found == 11 ? (uint64_t)__shfl(tabv, 10, 64) : n;
    // QNAME
    const uint64_t qn = fe[0];
    if (!qn) fault(err, ST_E_QNAME_EMPTY);
    if (qn > 254) fault(err, ST_E_QNAME_LONG);
    const uint32_t l_rn = (uint32_t)min(qn, (uint64_t)254) + 1;
    // FLAG RNAME POS MAPQ
    int64_t flag = 0, pos1 = 0, mapq = 0, pnext1 = 0, tlen = 0;
    if (!parse_dec(t, fb[1], fe[1], false, &flag) || flag > 65535) fault(err, ST_E_FLAG);
    bool ok = true;
    const int32_t ref = ref_lookup(t, fb[2], fe[2], R, &ok);
    if (!ok) fault(err, ST_E_RNAME);
    if (!parse_dec(t, fb[3], fe[3], false, &pos1) || pos1 > 0x7FFFFFFFll) fault(err, ST_E_POS);
    if (!parse_dec(t, fb[4], fe[4], false, &mapq) || mapq > 255) fault(err, ST_E_MAPQ);
    // CIGAR: counted first, since more than 65535 operations go to a CG:B,I tag behind the line's own tags
    const uint64_t cb = fb[5], ce = fe[5];
    const bool no_cigar = ce - cb == 1 && t[cb] == '*';
    uint64_t n_ops = 0, span = 0;
    if (!no_cigar) {
        if (cb == ce || is_digit(t[ce - 1])) fault(err, ST_E_CIGAR_DIGITS);
        for (uint64_t c0 = cb; c0 < ce; c0 += 64) {
            const uint64_t k = c0 + lane;
            n_ops += (uint64_t)__popcll(__ballot(k < ce && !is_digit(t[k])));
        }
    }
    const bool long_cigar = n_ops > 65535;
    const uint32_t n_cig = long_cigar ? 2u : (uint32_t)n_ops;
    uint8_t *const name_dst = dst + 36, *const cig_dst = name_dst + l_rn;
    if (!no_cigar) {
        if (!long_cigar) span = cigar_ops<W>(t, cb, ce, cig_dst, err);
        else if (!W) span = cigar_ops<false>(t, cb, ce, nullptr, err);
    }
    // RNEXT PNEXT TLEN
    int32_t next_ref;
    if (fe[6] - fb[6] == 1 && t[fb[6]] == '=') {
        next_ref = ref;
    } else {
        ok = true;
        next_ref = ref_lookup(t, fb[6], fe[6], R, &ok);
        if (!ok) fault(err, ST_E_RNEXT);
    }
    if (!parse_dec(t, fb[7], fe[7], false, &pnext1) || pnext1 > 0x7FFFFFFFll) fault(err, ST_E_PNEXT);
    if (!parse_dec(t, fb[8], fe[8], true, &tlen) || tlen > 0x7FFFFFFFll || tlen < -0x80000000ll) fault(err, ST_E_TLEN);
    // SEQ: eight letters per lane become four bytes, the high nibble first
    const uint64_t sb = fb[9], qb = fb[10];
    const bool no_seq = fe[9] - sb == 1 && t[sb] == '*';
    const uint64_t l_seq = no_seq ? 0 : fe[9] - sb, packed = (l_seq + 1) / 2;
    uint8_t *const seq_dst = cig_dst + 4ull * n_cig, *const qual_dst = seq_dst + packed;
    if (!no_seq && !l_seq) fault(err, ST_E_SEQ);
    for (uint64_t g = lane; 4 * g < packed; g += 64) {
        uint8_t c[8] = {};
        if (8 * g + 8 <= l_seq) {
            __builtin_memcpy(c, t + sb + 8 * g, 8);
        } else {
            for (uint32_t j = 0; 8 * g + j < l_seq; j++) c[j] = t[sb + 8 * g + j];
        }
        uint32_t word = 0;
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
            uint32_t v = 0;
            if (8 * g + j < l_seq) {
                v = seq_code(c[j]);
                if (v > 15u) {
                    fault(err, ST_E_SEQ);
                    v = 0;
                }
            }
            word |= v << (8 * (j >> 1) + ((j & 1) ? 0 : 4));
        }
        if (W) {
            if (4 * g + 4 <= packed) st32(seq_dst + 4 * g, word);
            else
                for (uint32_t j = 0; 4 * g + j < packed; j++) seq_dst[4 * g + j] = (uint8_t)(word >> (8 * j));
        }
    }
    // QUAL: four bytes per lane, the byte minus 33; `*` gives 0xFF for every base
    const uint64_t ql = fe[10] - qb;
    const bool no_qual = ql == 1 && t[qb] == '*';
    if (!no_qual) {
        if (no_seq) fault(err, ST_E_QUAL_NO_SEQ);
        else if (ql != l_seq) fault(err, ST_E_QUAL_LEN);
    }
    const uint64_t q_take = no_qual ? 0 : min(ql, l_seq);
    for (uint64_t g = lane; 4 * g < l_seq; g += 64) {
        uint32_t word = 0xFFFFFFFFu;
        if (!no_qual) {
            uint8_t c[4] = {33, 33, 33, 33};
            if (4 * g + 4 <= q_take) {
                __builtin_memcpy(c, t + qb + 4 * g, 4);
            } else {
                for (uint32_t j = 0; 4 * g + j < q_take; j++) c[j] = t[qb + 4 * g + j];
            }
            word = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const uint32_t v = (uint32_t)c[j] - 33u;
                if (v > 93u) fault(err, ST_E_QUAL_CHAR);
                word |= (v & 255u) << (8 * j);
            }
        }
        if (W) {
            if (4 * g + 4 <= l_seq) st32(qual_dst + 4 * g, word);
            else
                for (uint32_t j = 0; 4 * g + j < l_seq; j++) qual_dst[4 * g + j] = (uint8_t)(word >> (8 * j));
        }
    }
    // tags, in line order: serial per tag, parallel inside each one.  The walk ends at the first faulty tag.
    uint8_t *const aux = qual_dst + l_seq;
    uint64_t tsize = 0;
    if (found == 11) {
        uint64_t tb = fe[10] + 1;
        for (;;) {
            uint64_t te = n; // the next tab, or the end of the line
            for (uint64_t c0 = tb; c0 < n; c0 += 64) {
                const uint64_t k = c0 + lane;
                const uint64_t m = __ballot(k < n && t[k] == '\t');
                if (m) {
                    te = c0 + (uint64_t)(__ffsll((unsigned long long)m) - 1);
                    break;
                }
            }
            const uint64_t L = te - tb;
            const uint8_t *p = t + tb;
            if (L < 5 || p[2] != ':' || p[4] != ':') {
                fault(err, ST_E_TAG_FORM);
                break;
            }
            const uint8_t ty = p[3];
            const uint64_t vb = tb + 5, vl = L - 5;
            uint8_t *const o = aux + tsize;
            if (W && lane == 0) {
                o[0] = p[0];
                o[1] = p[1];
            }
            if (ty == 'A') {
                if (vl != 1) {
                    fault(err, ST_E_TAG_FORM);
                    break;
                }
                if (W && lane == 0) {
                    o[2] = 'A';
                    o[3] = t[vb];
                }
                tsize += 4;
            } else if (ty == 'i') {
                int64_t v = 0;
                if (!parse_dec(t, vb, te, true, &v) || v < -0x80000000ll || v > 0xFFFFFFFFll) {
                    fault(err, ST_E_NUMBER);
                    break;
                }
                // the smallest type that holds the value
                const uint32_t w = v >= 0 ? (v < 256 ? 1u : v < 65536 ? 2u : 4u) : (v >= -128 ? 1u : v >= -32768 ? 2u : 4u);
                if (W && lane == 0) {
                    o[2] = v >= 0 ? (w == 1 ? 'C' : w == 2 ? 'S' : 'I') : (w == 1 ? 'c' : w == 2 ? 's' : 'i');
                    if (w == 1) o[3] = (uint8_t)v;
                    else if (w == 2) st16(o + 3, (uint32_t)v);
                    else st32(o + 3, (uint32_t)v);
                }
                tsize += 3 + w;
            } else if (ty == 'f') {
                if (vl > ST_FLOAT_TEXT_MAX) {
                    fault(err, ST_E_FLOAT_LONG);
                    break;
                }
                if (F) {
                    // one lane parses (the parser is the costly part of these kernels); the wave takes its answer
                    uint32_t u = 0, good = 0;
                    if (lane == 0) good = parse_f32(t + vb, (uint32_t)vl, &u) ? 1u : 0u;
                    good = (uint32_t)__shfl((int)good, 0, 64);
                    if (!good) {
                        fault(err, ST_E_NUMBER);
                        break;
                    }
                    if (W && lane == 0) {
                        o[2] = 'f';
                        st32(o + 3, u);
                    }
                } else {
                    *has_float = true;
                }
                tsize += 7;
            } else if (ty == 'Z' || ty == 'H') {
                if (ty == 'H') {
                    bool bad = (vl & 1) != 0;
                    for (uint64_t c0 = 0; c0 < vl; c0 += 64) {
                        const uint64_t k = c0 + lane;
                        const uint32_t c = k < vl ? t[vb + k] : '0';
                        if (__ballot(!(is_digit(c) || ((c | 0x20u) - 'a') <= 5u))) bad = true;
                    }
                    if (bad) {
                        fault(err, ST_E_HEX);
                        break;
                    }
                }
                if (W) {
                    for (uint64_t k = lane; k < vl; k += 64) o[3 + k] = t[vb + k];
                    if (lane == 0) {
                        o[2] = ty;
                        o[3 + vl] = 0;
                    }
                }
                tsize += 3 + vl + 1;
            } else if (ty == 'B') {
                if (vl < 1) {
                    fault(err, ST_E_TAG_FORM);
                    break;
                }
                const uint8_t sub = t[vb];
                const uint32_t w = b_width(sub);
                if (!w) {
                    fault(err, ST_E_B_SUB);
                    break;
                }
                if (vl > 1 && t[vb + 1] != ',') {
                    fault(err, ST_E_NUMBER);
                    break;
                }
                if (!F && sub == 'f') *has_float = true;
                // the elements, 64 bytes at a time behind a ballot of the commas: each comma's lane parses what follows it
                uint64_t cnt = 0;
                uint32_t berr = ~0u;
                for (uint64_t c0 = vb + 1; c0 < te; c0 += 64) {
                    const uint64_t k = c0 + lane;
                    const bool comma = k < te && t[k] == ',';
                    const uint64_t m = __ballot(comma);
                    if (comma) {
                        uint64_t e2 = k + 1;
                        while (e2 < te && t[e2] != ',') e2++;
                        uint8_t *const q = o + 8 + (cnt + rank_in(m)) * w;
                        if (sub == 'f') {
                            if (e2 - (k + 1) > ST_FLOAT_TEXT_MAX) berr = min(berr, (uint32_t)ST_E_FLOAT_LONG);
                            else if (F) {
                                uint32_t u = 0;
                                if (!parse_f32(t + k + 1, (uint32_t)(e2 - (k + 1)), &u)) berr = min(berr, (uint32_t)ST_E_NUMBER);
                                if (W) st32(q, u);
                            } else if (e2 == k + 1) berr = min(berr, (uint32_t)ST_E_NUMBER);
                        } else {
                            int64_t v = 0;
                            const int64_t lo = sub == 'c' ? -128 : sub == 's' ? -32768 : sub == 'i' ? -0x80000000ll : 0;
                            const int64_t hi = sub == 'c' ? 127 : sub == 'C' ? 255 : sub == 's' ? 32767 : sub == 'S' ? 65535 : sub == 'i' ? 0x7FFFFFFFll : 0xFFFFFFFFll;
                            if (!parse_dec(t, k + 1, e2, lo < 0, &v) || v < lo || v > hi) berr = min(berr, (uint32_t)ST_E_NUMBER);
                            if (W) {
                                if (w == 1) q[0] = (uint8_t)v;
                                else if (w == 2) st16(q, (uint32_t)v);
                                else st32(q, (uint32_t)v);
                            }
                        }
                    }
                    cnt += (uint64_t)__popcll(m);
                }
                berr = wave_min(berr);
                if (berr != ~0u) {
                    fault(err, berr);
                    break;
                }
                if (W && lane == 0) {
                    o[2] = 'B';
                    o[3] = sub;
                    st32(o + 4, (uint32_t)cnt);
                }
                tsize += 8 + cnt * w;
            } else {
                fault(err, ST_E_TAG_TYPE);
                break;
            }
            if (te >= n) break;
            tb = te + 1;
        }
    }
    if (long_cigar) { // SAM specification 4.2.2: the operations in a CG:B,I tag, <l_seq>S<span>N in the record's CIGAR
        uint8_t *const o = aux + tsize;
        if (W) {
            span = cigar_ops<true>(t, cb, ce, o + 8, err);
            if (lane == 0) {
                o[0] = 'C';
                o[1] = 'G';
                o[2] = 'B';
                o[3] = 'I';
                st32(o + 4, (uint32_t)n_ops);
                st32(cig_dst, (uint32_t)l_seq << 4 | 4u);
                st32(cig_dst + 4, (uint32_t)span << 4 | 3u);
            }
        }
        tsize += 8 + 4 * n_ops;
    }
    const uint64_t total = 36ull + l_rn + 4ull * n_cig + packed + l_seq + tsize;
    if (total > (1ull << 31)) fault(err, ST_E_TOO_LARGE);
    if (W) {
        for (uint64_t k = lane; k < l_rn - 1; k += 64) name_dst[k] = t[k];
        if (lane == 0) {
            name_dst[l_rn - 1] = 0;
            const int64_t pos = pos1 - 1;
            const uint32_t bin = pos < 0 ? 4680u : reg2bin(pos, pos + (int64_t)max(span, (uint64_t)1)) & 0xFFFFu;
            st32(dst, (uint32_t)(total - 4));
            st32(dst + 4, (uint32_t)ref);
            st32(dst + 8, (uint32_t)pos);
            st32(dst + 12, l_rn | (uint32_t)mapq << 8 | bin << 16);
            st32(dst + 16, n_cig | (uint32_t)flag << 16);
            st32(dst + 20, (uint32_t)l_seq);
            st32(dst + 24, (uint32_t)next_ref);
            st32(dst + 28, (uint32_t)(pnext1 - 1));
            st32(dst + 32, (uint32_t)tlen);
        }
    }
    return total;
}

__global__ __launch_bounds__(BT) void k_st_size(const uint8_t *__restrict__ text, const uint64_t *__restrict__ start, uint64_t n, uint64_t first_index,
                                                SamTextRefs R, uint64_t *__restrict__ len, unsigned long long *bad, SamTextFloats fl) {
    const uint64_t i = (uint64_t)blockIdx.x * LINES_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= n) return; // (a whole wave: i is the wave's)
    uint32_t err = ~0u;
    bool has_float = false;
    const uint64_t a = start[i];
    const uint64_t bytes = st_line<false, false>(text + a, start[i + 1] - 1 - a, R, nullptr, &err, &has_float);
    err = wave_min(err);
    if (lane_id() == 0) {
        len[i] = bytes;
        fl.mark[i] = has_float;
        if (has_float) fl.list[atomicAdd(fl.count, 1ull)] = i;
        if (i == n - 1) len[n] = 0;
        // a marked line's faults are k_st_size_floats': this pass walked on past a float it did not parse, so a fault it met
        // behind one may not be the line's leftmost
        if (err != ~0u && !has_float) (void)atomicMin(bad, (unsigned long long)(first_index + i) << ST_ERR_BITS | err);
    }
}

// the lines k_st_size marked, a wave each, with the float parser: their values are validated (their size is known) and every
// fault of the line is found again, in line order
__global__ __launch_bounds__(BT) void k_st_size_floats(const uint8_t *__restrict__ text, const uint64_t *__restrict__ start, uint64_t first_index,
                                                       SamTextRefs R, unsigned long long *bad, SamTextFloats fl) {
    const uint64_t cnt = *fl.count;
    for (uint64_t j = (uint64_t)blockIdx.x * LINES_PER_BLOCK + (threadIdx.x >> 6); j < cnt; j += (uint64_t)gridDim.x * LINES_PER_BLOCK) {
        const uint64_t i = fl.list[j], a = start[i];
        uint32_t err = ~0u;
        bool has_float = false;
        (void)st_line<false, true>(text + a, start[i + 1] - 1 - a, R, nullptr, &err, &has_float);
        err = wave_min(err);
        if (lane_id() == 0 && err != ~0u) (void)atomicMin(bad, (unsigned long long)(first_index + i) << ST_ERR_BITS | err);
    }
}

__global__ void k_st_total(const uint64_t *__restrict__ off, uint64_t n, const unsigned long long *__restrict__ bad, unsigned long long *host) {
    if (threadIdx.x == 0) {
        host[0] = off[n];
        host[1] = *bad;
    }
}

__global__ __launch_bounds__(BT) void k_st_write(const uint8_t *__restrict__ text, const uint64_t *__restrict__ start, uint64_t n, SamTextRefs R,
                                                 const uint64_t *__restrict__ off, uint8_t *__restrict__ out, SamTextFloats fl) {
    const uint64_t i = (uint64_t)blockIdx.x * LINES_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= n || fl.mark[i]) return; // (a marked line is k_st_write_floats')
    uint32_t err = ~0u;
    bool has_float = false;
    const uint64_t a = start[i];
    (void)st_line<true, false>(text + a, start[i + 1] - 1 - a, R, out + off[i], &err, &has_float);
}

__global__ __launch_bounds__(BT) void k_st_write_floats(const uint8_t *__restrict__ text, const uint64_t *__restrict__ start, SamTextRefs R,
                                                        const uint64_t *__restrict__ off, uint8_t *__restrict__ out, SamTextFloats fl) {
    const uint64_t cnt = *fl.count;
    for (uint64_t j = (uint64_t)blockIdx.x * LINES_PER_BLOCK + (threadIdx.x >> 6); j < cnt; j += (uint64_t)gridDim.x * LINES_PER_BLOCK) {
        const uint64_t i = fl.list[j], a = start[i];
        uint32_t err = ~0u;
        bool has_float = false;
        (void)st_line<true, true>(text + a, start[i + 1] - 1 - a, R, out + off[i], &err, &has_float);
    }
}

} // namespace

uint32_t samtext_name_hash(const uint8_t *p, uint64_t n) { return fnv1a(p, n); }
bool samtext_parse_f32_host(const uint8_t *p, uint32_t n, uint32_t *bits) { return n <= ST_FLOAT_TEXT_MAX && parse_f32(p, n, bits); }

hipError_t launch_samtext_count(const uint8_t *text, uint64_t bytes, uint64_t *tile_cnt, hipStream_t s) {
    const uint64_t tiles = samtext_tiles(bytes);
    if (!tiles || tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_st_count, dim3((uint32_t)tiles), dim3(BT), 0, s, text, bytes, tile_cnt, tiles);
    return hipGetLastError();
}

hipError_t launch_samtext_word(const uint64_t *v, uint64_t n, unsigned long long *host, hipStream_t s) {
    hipLaunchKernelGGL(k_st_word, dim3(1), dim3(64), 0, s, v, n, host);
    return hipGetLastError();
}

hipError_t launch_samtext_scatter(const uint8_t *text, uint64_t bytes, const uint64_t *tile_off, uint64_t cap, uint64_t *start, hipStream_t s) {
    const uint64_t tiles = samtext_tiles(bytes);
    if (!tiles || tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_st_scatter, dim3((uint32_t)tiles), dim3(BT), 0, s, text, bytes, tile_off, cap, start);
    return hipGetLastError();
}

hipError_t launch_samtext_size(const uint8_t *text, const uint64_t *start, uint64_t n, uint64_t first_index, const SamTextRefs &refs, uint64_t *len,
                               unsigned long long *bad, const SamTextFloats &fl, hipStream_t s) {
    if (!n) return hipSuccess;
    const uint64_t blocks = (n + LINES_PER_BLOCK - 1) / LINES_PER_BLOCK;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(fl.count, 0, sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_st_size, dim3((uint32_t)blocks), dim3(BT), 0, s, text, start, n, first_index, refs, len, bad, fl);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_st_size_floats, dim3(FLOAT_BLOCKS), dim3(BT), 0, s, text, start, first_index, refs, bad, fl);
    return hipGetLastError();
}

hipError_t launch_samtext_total(const uint64_t *off, uint64_t n, const unsigned long long *bad, unsigned long long *host, hipStream_t s) {
    hipLaunchKernelGGL(k_st_total, dim3(1), dim3(64), 0, s, off, n, bad, host);
    return hipGetLastError();
}

hipError_t launch_samtext_write(const uint8_t *text, const uint64_t *start, uint64_t n, const SamTextRefs &refs, const uint64_t *off, uint8_t *out,
                                const SamTextFloats &fl, hipStream_t s) {
    if (!n) return hipSuccess;
    const uint64_t blocks = (n + LINES_PER_BLOCK - 1) / LINES_PER_BLOCK;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_st_write, dim3((uint32_t)blocks), dim3(BT), 0, s, text, start, n, refs, off, out, fl);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_st_write_floats, dim3(FLOAT_BLOCKS), dim3(BT), 0, s, text, start, refs, off, out, fl);
    return hipGetLastError();
}

} // namespace ngsq
