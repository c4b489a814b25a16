// sam_kernel.hip -- `ngs convert <BAM> <SAM>` on the device: the SAM line of every record of a batch
// of the device ingest.  One wave per record in both passes: the sizing pass walks the record as the write pass does and
// only counts, so the two agree by construction; the offsets between them come from the ingest's exclusive scan.  Inside
// a record the wave spreads what is long across its lanes -- CIGAR operations, SEQ and QUAL bytes, Z/H bytes, B array
// elements -- so that a 100 kb read or a 70 000-operation CIGAR costs its own wave some more steps, not one thread the
// whole batch.  sam.cpp drives them, copies the text to the host and writes it.
#include <hip/hip_runtime.h>

#include "sam_kernels.h"

namespace ngsq {

namespace {

constexpr uint32_t BT = 256; // threads per block: four records
constexpr uint32_t RECS_PER_BLOCK = BT / 64;
constexpr uint32_t FLOAT_BLOCKS = 1024; // grid of the kernels over the records that hold a float (grid-stride)

__device__ __forceinline__ uint32_t ld32u(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ uint32_t ld16u(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

__host__ __device__ inline uint32_t dec_len32(uint32_t v) {
    uint32_t n = 1;
    for (uint32_t t = 10; n < 10 && v >= t; t *= 10) n++;
    return n;
}
__host__ __device__ inline uint32_t dec_len64(uint64_t v) {
    uint32_t n = 1;
    while (v >= 10) {
        v /= 10;
        n++;
    }
    return n;
}
// decimal text of v (every integer of a SAM line fits: |v| < 2^32)
__host__ __device__ inline uint32_t int_len(int64_t v) { return (v < 0 ? 1u : 0u) + dec_len32((uint32_t)(v < 0 ? -v : v)); }
__host__ __device__ inline void put_int(char *p, int64_t v, uint32_t len) {
    uint32_t m = (uint32_t)(v < 0 ? -v : v);
    const uint32_t lo = v < 0 ? 1u : 0u;
    if (lo) p[0] = '-';
    for (uint32_t k = len; k-- > lo;) {
        p[k] = (char)('0' + m % 10);
        m /= 10;
    }
}

// ---- f32 text --------------------------------------------------------------------------------
// 320-bit unsigned integers, little-endian limbs: exact comparisons of d * 10^q with N * 2^E
struct Big {
    uint32_t w[10];
};
__host__ __device__ inline void big_set(Big &a, uint64_t v) {
    for (int k = 0; k < 10; k++) a.w[k] = 0;
    a.w[0] = (uint32_t)v;
    a.w[1] = (uint32_t)(v >> 32);
}
__host__ __device__ inline void big_mul(Big &a, uint32_t m) {
    uint64_t c = 0;
    for (int k = 0; k < 10; k++) {
        c += (uint64_t)a.w[k] * m;
        a.w[k] = (uint32_t)c;
        c >>= 32;
    }
}
__host__ __device__ inline void big_pow5(Big &a, int n) {
    for (; n >= 13; n -= 13) big_mul(a, 1220703125u); // 5^13
    uint32_t m = 1;
    for (; n > 0; n--) m *= 5;
    big_mul(a, m);
}
__host__ __device__ inline void big_shl(Big &a, int s) {
    const int wq = s >> 5, bq = s & 31;
    for (int k = 9; k >= 0; k--) {
        const uint32_t hi = k - wq >= 0 ? a.w[k - wq] : 0u, lo = k - wq - 1 >= 0 ? a.w[k - wq - 1] : 0u;
        a.w[k] = bq ? (hi << bq | lo >> (32 - bq)) : hi;
    }
}
__host__ __device__ inline int big_cmp(const Big &a, const Big &b) {
    for (int k = 9; k >= 0; k--)
        if (a.w[k] != b.w[k]) return a.w[k] < b.w[k] ? -1 : 1;
    return 0;
}
// sign of d * 10^q - n * 2^e (d, n < 2^40: the candidates are near the float, whose magnitude bounds both sides by 2^200)
__host__ __device__ __attribute__((noinline)) int cmp_dec_bin(uint64_t d, int q, uint64_t n, int e) {
    Big a, b;
    big_set(a, d);
    big_set(b, n);
    if (q >= 0) big_pow5(a, q);
    else big_pow5(b, -q);
    if (q > e) big_shl(a, q - e);
    else big_shl(b, e - q);
    return big_cmp(a, b);
}

// The shortest decimal d * 10^q that reads back as the finite non-zero float m * 2^e, and among those the closest to it (a
// tie: the even d).  Reading rounds to the nearest float, a tie to the even mantissa: the interval between the midpoints to
// the two neighbours holds its ends exactly when m is even.  The first q from above whose grid has a point inside the
// interval is the shortest; the point is the grid point nearest the float, or its neighbour on the interval's side.
__host__ __device__ inline void f32_shortest(uint32_t ex, uint32_t fr, uint64_t *d_out, int *q_out) {
    const uint64_t m = ex ? (fr | 0x800000u) : fr;
    const int e = ex ? (int)ex - 150 : -149;
    const uint64_t hi_n = 2 * m + 1;
    const int hi_e = e - 1;
    const bool low_closer = fr == 0 && ex > 1; // a power of two: the neighbour below is half as far
    const uint64_t lo_n = low_closer ? 4 * m - 1 : 2 * m - 1;
    const int lo_e = low_closer ? e - 2 : e - 1;
    const bool incl = (m & 1) == 0;
    const double xd = ldexp((double)m, e); // exact
    const int k = (int)floor(log10(xd));
    for (int q = k + 2; q >= k - 10; q--) {
        uint64_t d0 = (uint64_t)(xd / pow(10.0, (double)q)); // floor(x / 10^q), up to the division's rounding
        while (d0 > 0 && cmp_dec_bin(d0, q, m, e) > 0) d0--;
        while (cmp_dec_bin(d0 + 1, q, m, e) <= 0) d0++;
        const int c = cmp_dec_bin(2 * d0 + 1, q, m, e + 1); // (d0 + 1/2) 10^q against x
        const uint64_t r = c < 0 ? d0 + 1 : c > 0 ? d0 : d0 + (d0 & 1);
        for (int t = 0; t < 3; t++) {
            const uint64_t d = t == 0 ? r : t == 1 ? r + 1 : r - 1;
            if (d == 0 || (t == 2 && r == 0)) continue;
            const int a = cmp_dec_bin(d, q, lo_n, lo_e), b = cmp_dec_bin(d, q, hi_n, hi_e);
            if (incl ? (a >= 0 && b <= 0) : (a > 0 && b < 0)) {
                *d_out = d;
                *q_out = q;
                return;
            }
        }
    }
    *d_out = m; // (not reached: nine significant digits always read back)
    *q_out = 0;
}

// THE float formatter of the SAM text (`f` tags and B:f elements): Rust's Display of an f32 -- the shortest digits that read
// back, the closest of them, positional without an exponent, no trailing ".0"; NaN, inf, -inf, -0.  Returns the length
// (at most 48); writes the text to out unless it is null.
__host__ __device__ __attribute__((noinline)) uint32_t sam_f32(uint32_t u, char *out) {
    const uint32_t neg = u >> 31, ex = (u >> 23) & 255u, fr = u & 0x7FFFFFu;
    if (ex == 255u) {
        const char *t = fr ? "NaN" : neg ? "-inf" : "inf";
        const uint32_t n = fr ? 3 : 3 + neg;
        if (out)
            for (uint32_t k = 0; k < n; k++) out[k] = t[k];
        return n;
    }
    if (ex == 0 && fr == 0) {
        if (out) {
            if (neg) out[0] = '-';
            out[neg] = '0';
        }
        return 1 + neg;
    }
    uint64_t d;
    int q;
    f32_shortest(ex, fr, &d, &q);
    while (d % 10 == 0) { // (the search never stops on one; kept so the text below can rely on it)
        d /= 10;
        q++;
    }
    const int nd = (int)dec_len64(d);
    const int pnt = nd + q; // digits in front of the point
    const uint32_t len = neg + (q >= 0 ? (uint32_t)(nd + q) : pnt > 0 ? (uint32_t)nd + 1 : (uint32_t)(2 - pnt + nd));
    if (!out) return len;
    char *p = out + neg;
    if (neg) out[0] = '-';
    if (q >= 0) {
        for (int j = nd - 1; j >= 0; j--, d /= 10) p[j] = (char)('0' + d % 10);
        for (int j = 0; j < q; j++) p[nd + j] = '0';
    } else if (pnt > 0) {
        for (int j = nd - 1; j >= 0; j--, d /= 10) p[j < pnt ? j : j + 1] = (char)('0' + d % 10);
        p[pnt] = '.';
    } else {
        p[0] = '0';
        p[1] = '.';
        for (int j = 0; j < -pnt; j++) p[2 + j] = '0';
        for (int j = nd - 1; j >= 0; j--, d /= 10) p[2 - pnt + j] = (char)('0' + d % 10);
    }
    return len;
}

// ---- one record's line, by one wave ----------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

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

// value width of a B array subtype, 0: not one
__device__ __forceinline__ uint32_t b_width(uint8_t sub) {
    return sub == 'c' || sub == 'C' ? 1u : sub == 's' || sub == 'S' ? 2u : sub == 'i' || sub == 'I' || sub == 'f' ? 4u : 0u;
}
// an integer of type ty ('c' 'C' 's' 'S' 'i' 'I') at p
__device__ __forceinline__ int64_t int_value(uint8_t ty, const uint8_t *p) {
    switch (ty) {
    case 'c': return (int8_t)p[0];
    case 'C': return p[0];
    case 's': return (int16_t)ld16u(p);
    case 'S': return ld16u(p);
    case 'i': return (int32_t)ld32u(p);
    default: return ld32u(p);
    }
}

// The tag that holds the real CIGAR of a long-CIGAR record (SAM specification 4.2.2; the ingest's rule, bam_device.hip
// aux_find_cg): the first CG:B,I tag of the data, if the tags in front of it are whole; its offset in [p0, end), or -1.
__device__ int64_t find_cg(const uint8_t *p0, const uint8_t *end) {
    const uint8_t *p = p0;
    while (end - p >= 4) {
        const uint8_t t0 = p[0], t1 = p[1], ty = p[2];
        const uint8_t *at = p;
        p += 3;
        uint64_t n = 0;
        if (ty == 'A' || ty == 'c' || ty == 'C') n = 1;
        else if (ty == 's' || ty == 'S') n = 2;
        else if (ty == 'i' || ty == 'I' || ty == 'f') n = 4;
        else if (ty == 'Z' || ty == 'H') {
            while (p < end && *p) p++;
            if (p >= end) return -1;
            n = 1;
        } else if (ty == 'B') {
            if (end - p < 5) return -1;
            const uint8_t sub = p[0];
            const uint32_t cnt = ld32u(p + 1), w = b_width(sub);
            if (!w) return -1;
            n = 5 + (uint64_t)cnt * w;
            if (t0 == 'C' && t1 == 'G' && sub == 'I') {
                if ((uint64_t)(end - p) < n || cnt < 2) return -1;
                return at - p0;
            }
        } else {
            return -1;
        }
        if ((uint64_t)(end - p) < n) return -1;
        p += n;
    }
    return -1;
}

// Copy n bytes from src to dst across the wave (W: write; the caller adds n to its cursor)
template <bool W> __device__ __forceinline__ void wave_copy(char *dst, const uint8_t *src, uint64_t n) {
    if (!W) return;
    for (uint64_t k = lane_id(); k < n; k += 64) dst[k] = (char)src[k];
}
// lane 0 writes a short text
template <bool W> __device__ __forceinline__ void put_text(char *dst, const char *t, uint32_t n) {
    if (W && lane_id() == 0)
        for (uint32_t k = 0; k < n; k++) dst[k] = t[k];
}
template <bool W> __device__ __forceinline__ uint32_t emit_int(char *dst, int64_t v) {
    const uint32_t n = int_len(v);
    if (W && lane_id() == 0) put_int(dst, v, n);
    return n;
}
// a reference name, '*' for -1; *err for an id outside the table
template <bool W> __device__ __forceinline__ uint64_t emit_ref(char *dst, int32_t r, const SamRefs &R, uint32_t *err) {
    if (r == -1 || r < -1 || (uint32_t)r >= R.n_refs) {
        if (r != -1) *err = min(*err, (uint32_t)SAM_E_REF);
        put_text<W>(dst, "*", 1);
        return 1;
    }
    const uint64_t a = R.name_off[r], n = R.name_off[r + 1] - a;
    wave_copy<W>(dst, reinterpret_cast<const uint8_t *>(R.names) + a, n);
    return n;
}

// The SAM line of record i, by the whole wave: every lane returns its length; W writes it at dst.
// *err (the lane's own, ~0u on entry): the smallest SamError met; left at ~0u if none.  F: the f32 values are formatted
// (sam_f32 needs four times the registers of the rest: the kernels without F run at full occupancy and only mark the rare
// record that holds a float, *has_float, whose length and text then are wrong; the F kernels redo those records).
template <bool W, bool F>
__device__ uint64_t sam_line(const ngsq_batch &b, const BatchOrigin &o, const SamRefs &R, uint64_t i, char *dst, uint32_t *err,
                             bool *has_float) {
    const uint32_t lane = lane_id();
    const uint8_t *rec = o.raw + o.rec_off[i];
    const uint32_t bs = ld32u(rec);
    const uint8_t *body = rec + 4, *end = body + bs;
    const int32_t ref = (int32_t)ld32u(body), pos = (int32_t)ld32u(body + 4);
    const uint32_t l_rn = body[8], mapq = body[9], n_raw_ops = ld16u(body + 12), flag = ld16u(body + 14);
    const uint32_t l = ld32u(body + 16);
    const int32_t next_ref = (int32_t)ld32u(body + 20), next_pos = (int32_t)ld32u(body + 24), tlen = (int32_t)ld32u(body + 28);
    const uint8_t *name = body + 32, *seq = name + l_rn + 4ull * n_raw_ops, *qual = seq + (l + 1) / 2, *aux = qual + l;
    uint64_t cur = 0;
    // QNAME FLAG RNAME POS MAPQ
    const uint32_t qn = l_rn ? l_rn - 1 : 0;
    wave_copy<W>(dst, name, qn);
    cur += qn;
    put_text<W>(dst + cur, "\t", 1);
    cur += 1;
    cur += emit_int<W>(dst + cur, flag);
    put_text<W>(dst + cur, "\t", 1);
    cur += 1;
    cur += emit_ref<W>(dst + cur, ref, R, err);
    put_text<W>(dst + cur, "\t", 1);
    cur += 1;
    cur += emit_int<W>(dst + cur, (int64_t)pos + 1);
    put_text<W>(dst + cur, "\t", 1);
    cur += 1;
    cur += emit_int<W>(dst + cur, mapq);
    put_text<W>(dst + cur, "\t", 1);
    cur += 1;
    // CIGAR: the batch's resolved operations (a long CIGAR's come from its CG tag), 64 at a time
    uint64_t k0, n_ops;
    if (b.cigar_off) {
        k0 = b.cigar_off[i];
        n_ops = b.cigar_off[i + 1] - k0;
    } else {
        k0 = i * (uint64_t)b.cigar_stride;
        n_ops = min((uint32_t)b.n_cigar[i], b.cigar_stride);
    }
    if (!n_ops) {
        put_text<W>(dst + cur, "*", 1);
        cur += 1;
    }
    for (uint64_t c0 = 0; c0 < n_ops; c0 += 64) {
        const uint64_t k = c0 + lane;
        uint32_t c = 0, len = 0;
        if (k < n_ops) {
            c = b.cigar[k0 + k];
            if ((c & 15u) > 8u) *err = min(*err, (uint32_t)SAM_E_CIGAR_OP);
            len = dec_len32(c >> 4) + 1;
        }
        const uint32_t incl = wave_incl(len);
        if (W && k < n_ops) {
            char *p = dst + cur + (incl - len);
            put_int(p, c >> 4, len - 1);
            p[len - 1] = "MIDNSHP=X???????"[c & 15u];
        }
        cur += __shfl(incl, 63, 64);
    }
    put_text<W>(dst + cur, "\t", 1);
    cur += 1;
    // RNEXT PNEXT TLEN
    if (next_ref == ref && ref >= 0) {
        put_text<W>(dst + cur, "=", 1);
        cur += 1;
    } else {
        cur += emit_ref<W>(dst + cur, next_ref, R, err);
    }
    put_text<W>(dst + cur, "\t", 1);
    cur += 1;
    cur += emit_int<W>(dst + cur, (int64_t)next_pos + 1);
    put_text<W>(dst + cur, "\t", 1);
    cur += 1;
    cur += emit_int<W>(dst + cur, tlen);
    put_text<W>(dst + cur, "\t", 1);
    cur += 1;
    // SEQ and QUAL: a byte per lane, neighbouring lanes on neighbouring bytes
    if (!l) {
        put_text<W>(dst + cur, "*\t*", 3);
        cur += 3;
    } else {
        if (W)
            for (uint64_t k = lane; k < l; k += 64)
                dst[cur + k] = "=ACMGRSVTWYHKDBN"[(seq[k >> 1] >> ((k & 1) ? 0 : 4)) & 15u];
        cur += l;
        put_text<W>(dst + cur, "\t", 1);
        cur += 1;
        if (qual[0] == 0xFF) { // htslib's test for absent qualities
            put_text<W>(dst + cur, "*", 1);
            cur += 1;
        } else {
            for (uint64_t k = lane; k < l; k += 64) {
                const uint32_t q = qual[k];
                if (q > 93u) *err = min(*err, (uint32_t)SAM_E_QUAL);
                if (W) dst[cur + k] = (char)(q + 33);
            }
            cur += l;
        }
    }
    // tags, in file order; a long CIGAR's CG tag is not one of them
    int64_t cg_at = -1;
    if (n_raw_ops == 2 && l && aux <= end) {
        const uint32_t op0 = ld32u(name + l_rn), op1 = ld32u(name + l_rn + 4);
        if (op0 == (l << 4 | 4u) && (op1 & 15u) == 3u) cg_at = find_cg(aux, end);
    }
    const uint8_t *p = aux;
    while (p < end) {
        if (end - p < 3) {
            *err = min(*err, (uint32_t)SAM_E_OVERRUN);
            break;
        }
        const uint8_t t0 = p[0], t1 = p[1], ty = p[2];
        const bool skip = p - aux == cg_at;
        const uint8_t *v = p + 3;
        const uint64_t left = (uint64_t)(end - v);
        const uint64_t at = cur + 1; // behind the tab
        if (!skip && W && lane == 0) {
            dst[cur] = '\t';
            dst[at] = (char)t0;
            dst[at + 1] = (char)t1;
            dst[at + 2] = ':';
            dst[at + 4] = ':';
        }
        uint64_t n = 6; // "\tTG:T:"
        const uint8_t *next;
        if (ty == 'A' || ty == 'c' || ty == 'C' || ty == 's' || ty == 'S' || ty == 'i' || ty == 'I' || ty == 'f') {
            const uint32_t w = ty == 'A' || ty == 'c' || ty == 'C' ? 1u : ty == 's' || ty == 'S' ? 2u : 4u;
            if (left < w) {
                *err = min(*err, (uint32_t)SAM_E_OVERRUN);
                break;
            }
            next = v + w;
            if (!skip) {
                if (ty == 'A') {
                    if (W && lane == 0) {
                        dst[at + 3] = 'A';
                        dst[at + 5] = (char)v[0];
                    }
                    n += 1;
                } else if (ty == 'f') {
                    if (F) {
                        const uint32_t u = ld32u(v);
                        if (W && lane == 0) {
                            dst[at + 3] = 'f';
                            (void)sam_f32(u, dst + at + 5);
                        }
                        n += sam_f32(u, nullptr);
                    } else {
                        *has_float = true;
                    }
                } else {
                    if (W && lane == 0) dst[at + 3] = 'i';
                    n += emit_int<W>(dst + at + 5, int_value(ty, v));
                }
            }
        } else if (ty == 'Z' || ty == 'H') {
            uint64_t len = ~0ull; // bytes in front of the NUL, looked for 64 at a time
            for (uint64_t c0 = 0; c0 < left; c0 += 64) {
                const uint64_t k = c0 + lane;
                const uint64_t hit = __ballot(k < left && v[k] == 0);
                if (hit) {
                    len = c0 + (uint64_t)(__ffsll((unsigned long long)hit) - 1);
                    break;
                }
            }
            if (len == ~0ull) {
                *err = min(*err, (uint32_t)SAM_E_STR_NUL);
                break;
            }
            next = v + len + 1;
            if (!skip) {
                if (W && lane == 0) dst[at + 3] = (char)ty;
                wave_copy<W>(dst + at + 5, v, len);
                n += len;
            }
        } else if (ty == 'B') {
            if (left < 5) {
                *err = min(*err, (uint32_t)SAM_E_OVERRUN);
                break;
            }
            const uint8_t sub = v[0];
            const uint32_t w = b_width(sub);
            if (!w) {
                *err = min(*err, (uint32_t)SAM_E_B_SUB);
                break;
            }
            const uint64_t cnt = ld32u(v + 1);
            if (cnt * w > left - 5) {
                *err = min(*err, (uint32_t)SAM_E_OVERRUN);
                break;
            }
            next = v + 5 + cnt * w;
            if (!F && sub == 'f') *has_float = true;
            if (!skip && (F || sub != 'f')) {
                if (W && lane == 0) {
                    dst[at + 3] = 'B';
                    dst[at + 5] = (char)sub;
                }
                n += 1;
                const uint8_t *e0 = v + 5;
                for (uint64_t c0 = 0; c0 < cnt; c0 += 64) { // ",value" per element, 64 elements at a time
                    const uint64_t k = c0 + lane;
                    uint32_t len = 0, u = 0;
                    int64_t iv = 0;
                    if (k < cnt) {
                        if (F && sub == 'f') {
                            u = ld32u(e0 + 4 * k);
                            len = 1 + sam_f32(u, nullptr);
                        } else {
                            iv = int_value(sub, e0 + k * w);
                            len = 1 + int_len(iv);
                        }
                    }
                    const uint32_t incl = wave_incl(len);
                    if (W && k < cnt) {
                        char *q = dst + cur + n + (incl - len);
                        q[0] = ',';
                        if (F && sub == 'f') (void)sam_f32(u, q + 1);
                        else put_int(q + 1, iv, len - 1);
                    }
                    n += __shfl(incl, 63, 64);
                }
            }
        } else {
            *err = min(*err, (uint32_t)SAM_E_TAG_TYPE);
            break;
        }
        if (!skip) cur += n;
        p = next;
    }
    put_text<W>(dst + cur, "\n", 1);
    return cur + 1;
}

__global__ __launch_bounds__(BT) void k_sam_size(ngsq_batch b, BatchOrigin o, SamRefs R, uint64_t *__restrict__ len,
                                                 unsigned long long *bad, SamFloats fl, const uint8_t *__restrict__ keep) {
    const uint64_t i = (uint64_t)blockIdx.x * RECS_PER_BLOCK + (threadIdx.x >> 6);
    const uint64_t n = b.n_records;
    if (i >= n) return; // (a whole wave: i is the wave's)
    if (keep && !keep[i]) { // a dropped record: no length, no error, no float mark (k_sam_write looks at keep again)
        if (lane_id() == 0) {
            len[i] = 0;
            fl.mark[i] = 0;
            if (i == n - 1) len[n] = 0;
        }
        return;
    }
    uint32_t err = ~0u;
    bool has_float = false;
    const uint64_t bytes = sam_line<false, false>(b, o, R, i, nullptr, &err, &has_float);
    err = wave_min(err);
    if (lane_id() == 0) {
        len[i] = bytes;
        fl.mark[i] = has_float;
        if (has_float) fl.list[atomicAdd(fl.count, 1ull)] = i;
        if (i == n - 1) len[n] = 0;
        if (err != ~0u) (void)atomicMin(bad, (unsigned long long)(b.first_record_index + i) << SAM_ERR_BITS | err);
    }
}

// the records k_sam_size marked, a wave each, with the float formatter
__global__ __launch_bounds__(BT) void k_sam_size_floats(ngsq_batch b, BatchOrigin o, SamRefs R, uint64_t *__restrict__ len,
                                                        unsigned long long *bad, SamFloats fl) {
    const uint64_t cnt = *fl.count;
    for (uint64_t j = (uint64_t)blockIdx.x * RECS_PER_BLOCK + (threadIdx.x >> 6); j < cnt; j += (uint64_t)gridDim.x * RECS_PER_BLOCK) {
        const uint64_t i = fl.list[j];
        uint32_t err = ~0u;
        bool has_float = false;
        const uint64_t bytes = sam_line<false, true>(b, o, R, i, nullptr, &err, &has_float);
        err = wave_min(err);
        if (lane_id() == 0) {
            len[i] = bytes;
            if (err != ~0u) (void)atomicMin(bad, (unsigned long long)(b.first_record_index + i) << SAM_ERR_BITS | err);
        }
    }
}

__global__ void k_sam_total(const uint64_t *__restrict__ off, uint64_t n, const unsigned long long *__restrict__ bad,
                            unsigned long long *host) {
    if (threadIdx.x == 0) {
        host[0] = off[n];
        host[1] = *bad;
    }
}

__global__ __launch_bounds__(BT) void k_sam_write(ngsq_batch b, BatchOrigin o, SamRefs R, const uint64_t *__restrict__ off,
                                                  char *__restrict__ text, SamFloats fl, const uint8_t *__restrict__ keep) {
    const uint64_t i = (uint64_t)blockIdx.x * RECS_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= b.n_records || fl.mark[i]) return; // (a marked record is k_sam_write_floats')
    if (keep && !keep[i]) return;               // (a dropped record is nobody's)
    uint32_t err = ~0u;
    bool has_float = false;
    (void)sam_line<true, false>(b, o, R, i, text + off[i], &err, &has_float);
}

__global__ __launch_bounds__(BT) void k_sam_write_floats(ngsq_batch b, BatchOrigin o, SamRefs R, const uint64_t *__restrict__ off,
                                                         char *__restrict__ text, SamFloats fl) {
    const uint64_t cnt = *fl.count;
    for (uint64_t j = (uint64_t)blockIdx.x * RECS_PER_BLOCK + (threadIdx.x >> 6); j < cnt; j += (uint64_t)gridDim.x * RECS_PER_BLOCK) {
        const uint64_t i = fl.list[j];
        uint32_t err = ~0u;
        bool has_float = false;
        (void)sam_line<true, true>(b, o, R, i, text + off[i], &err, &has_float);
    }
}

} // namespace

hipError_t launch_sam_size(const ngsq_batch &b, const BatchOrigin &o, const SamRefs &refs, uint64_t *len, unsigned long long *bad,
                           const SamFloats &fl, hipStream_t s, const uint8_t *keep) {
    if (!b.n_records) return hipSuccess;
    const uint64_t blocks = (b.n_records + RECS_PER_BLOCK - 1) / RECS_PER_BLOCK;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(fl.count, 0, sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sam_size, dim3((uint32_t)blocks), dim3(BT), 0, s, b, o, refs, len, bad, fl, keep);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_sam_size_floats, dim3(FLOAT_BLOCKS), dim3(BT), 0, s, b, o, refs, len, bad, fl);
    return hipGetLastError();
}

hipError_t launch_sam_total(const uint64_t *off, uint64_t n, const unsigned long long *bad, unsigned long long *host, hipStream_t s) {
    hipLaunchKernelGGL(k_sam_total, dim3(1), dim3(64), 0, s, off, n, bad, host);
    return hipGetLastError();
}

hipError_t launch_sam_write(const ngsq_batch &b, const BatchOrigin &o, const SamRefs &refs, const uint64_t *off, char *text,
                            const SamFloats &fl, hipStream_t s, const uint8_t *keep) {
    if (!b.n_records) return hipSuccess;
    const uint64_t blocks = (b.n_records + RECS_PER_BLOCK - 1) / RECS_PER_BLOCK;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sam_write, dim3((uint32_t)blocks), dim3(BT), 0, s, b, o, refs, off, text, fl, keep);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sam_write_floats, dim3(FLOAT_BLOCKS), dim3(BT), 0, s, b, o, refs, off, text, fl);
    return hipGetLastError();
}

} // namespace ngsq
