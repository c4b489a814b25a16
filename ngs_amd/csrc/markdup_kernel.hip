// markdup_kernel.hip -- `ngs markdup` on the device.  The ends pass is a wave per resident record: its
// lanes share the CIGAR's operations for the unclipped 5' end and the QUAL bytes, in aligned 16-byte words, for the score.  The
// key pass is a thread per record and hashes the names of the pair candidates; the mate search behind it is collate_kernel.hip's.
// The mark works on entries (a pair, or a candidate): keys and values a thread per entry, and behind the sort a thread per rank
// finds the run heads, raises its run's best value and compares its own with it, so that no step is quadratic in a run.  The
// apply pass stores one byte per record.  markdup.cpp drives them.
#include <hip/hip_runtime.h>

#include "fastq_format.h" // fq_ld16u, fq_ld32u, CLASS_*
#include "markdup_kernels.h"
#include "name_key.h"

namespace ngsq {

namespace {

constexpr uint32_t BT = 256;
constexpr uint32_t WAVES = BT / 64;

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

// acc + the bytes of w that are >= 15: a byte is >= 15 iff its top bit is set or its low seven bits plus 113 carry into it
__device__ __forceinline__ uint32_t add_scores(uint32_t w, uint32_t acc) {
    const uint32_t top = (((w & 0x7F7F7F7Fu) + 0x71717171u) | w) & 0x80808080u;
    return __builtin_amdgcn_sad_u8(w & ((top >> 7) * 0xFFu), 0u, acc);
}
__device__ __forceinline__ uint32_t score_of(uint32_t b) { return b >= 15u ? b : 0u; }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (uint32_t m = 32; m; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
    for (uint32_t m = 32; m; m >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, m);
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    for (uint32_t m = 32; m; m >>= 1) v = min(v, (uint32_t)__shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    for (uint32_t m = 32; m; m >>= 1) v = max(v, (uint32_t)__shfl_xor(v, m));
    return v;
}

__global__ __launch_bounds__(BT) void k_markdup_ends(const uint64_t *__restrict__ addr, uint64_t n, uint8_t *__restrict__ cls, uint64_t *__restrict__ end,
                                                     uint32_t *__restrict__ score, unsigned long long *work) {
    const uint64_t i = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= n) return; // (a whole wave: i is the wave's)
    const uint32_t lane = lane_id();
    const uint8_t *body = body_at(addr, i);
    const int32_t ref = (int32_t)fq_ld32u(body), pos = (int32_t)fq_ld32u(body + 4);
    const uint32_t l_rn = body[8], n_ops = fq_ld16u(body + 12), flag = fq_ld16u(body + 14), l = fq_ld32u(body + 16);
    const uint8_t *cig = body + 32 + l_rn;
    const uint8_t *qual = cig + 4ull * n_ops + ((uint64_t)l + 1) / 2;
    // ---- the score: the bytes in front of the first aligned word and behind the last one by lanes, the words 16 bytes a lane
    uint32_t acc = 0;
    if (l && qual[0] != 0xFFu) {
        const uint32_t head = min((uint32_t)(-(uintptr_t)qual & 15u), l);
        const uint64_t words = ((uint64_t)l - head) >> 4;
        const uint64_t tail_at = head + 16 * words;
        const uint32_t tail = (uint32_t)(l - tail_at); // < 16
        if (lane < head) acc = score_of(qual[lane]);
        if (lane >= 16u && lane - 16u < tail) acc = score_of(qual[tail_at + lane - 16u]);
        const uint4 *q16 = reinterpret_cast<const uint4 *>(qual + head);
        for (uint64_t w = lane; w < words; w += 64) {
            const uint4 v = q16[w];
            acc = add_scores(v.x, acc);
            acc = add_scores(v.y, acc);
            acc = add_scores(v.z, acc);
            acc = add_scores(v.w, acc);
        }
        acc = wave_sum(acc);
    }
    // ---- the end of a candidate: the lanes share the operations, twice (the span and the clip run's edges, then the run)
    uint64_t e = MARKDUP_NO_END;
    uint32_t c = CLASS_OTHER;
    bool bad = false;
    if (!(flag & 0x904u) && ref >= 0 && pos >= 0) {
        const bool rev = flag & 0x10u;
        int64_t u = pos;
        if (n_ops) {
            uint64_t span = 0;
            uint32_t first = n_ops, last_end = 0; // the first operation that is no clip; one behind the last that is none
            for (uint32_t k = lane; k < n_ops; k += 64) {
                const uint32_t op = fq_ld32u(cig + 4ull * k), code = op & 15u;
                if (code != 4u && code != 5u) {
                    first = min(first, k);
                    last_end = k + 1;
                }
                if (0x18Du >> code & 1u) span += op >> 4; // M, D, N, = and X
            }
            const uint32_t from = rev ? wave_max(last_end) : 0u, to = rev ? n_ops : wave_min(first);
            uint64_t clip = 0;
            for (uint32_t k = from + lane; k < to; k += 64) clip += fq_ld32u(cig + 4ull * k) >> 4;
            clip = wave_sum(clip);
            u = rev ? (int64_t)pos + (int64_t)wave_sum(span) - 1 + (int64_t)clip : (int64_t)pos - (int64_t)clip;
        }
        bad = u < -MARKDUP_END_BIAS || u >= ((int64_t)1 << 31) - MARKDUP_END_BIAS;
        if (!bad) e = (uint64_t)(uint32_t)ref << 33 | (uint64_t)(u + MARKDUP_END_BIAS) << 1 | (rev ? 1u : 0u);
        if ((flag & 0x9u) == 0x1u) c = (flag & 0xC0u) == 0x40u ? CLASS_ONE : (flag & 0xC0u) == 0x80u ? CLASS_TWO : CLASS_OTHER;
    }
    if (lane == 0) {
        cls[i] = (uint8_t)c;
        end[i] = e;
        score[i] = acc;
        if (bad) (void)atomicMin(&work[CW_BAD], (unsigned long long)i);
    }
}

__global__ __launch_bounds__(BT) void k_markdup_key(const uint64_t *__restrict__ addr, const uint8_t *__restrict__ cls, const uint64_t *__restrict__ end,
                                                    uint64_t n, uint64_t mask, uint64_t *__restrict__ key, unsigned long long *work) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    const bool in = i < n;
    bool cand = false, cleared = false;
    if (in) {
        const uint8_t *body = body_at(addr, i);
        key[i] = cls[i] == CLASS_OTHER ? COLLATE_KEY_OTHER : name_hash(body + 32, name_bytes(body)) & mask;
        cand = end[i] != MARKDUP_NO_END;
        cleared = body[15] & 0x4u;
    }
    const uint32_t n_cand = __popcll(__ballot(cand)), n_cleared = __popcll(__ballot(cleared));
    if (lane_id() == 0) {
        if (n_cand) atomicAdd(&work[MW_CANDIDATES], (unsigned long long)n_cand);
        if (n_cleared) atomicAdd(&work[MW_CLEARED], (unsigned long long)n_cleared);
    }
}

__device__ __forceinline__ bool of_kind(const uint64_t *end, const uint32_t *mate, const uint8_t *dup, uint64_t i, uint32_t kind) {
    if (kind == MK_LEAD) return mate[i] != COLLATE_NONE && mate[i] > i;
    return kind == MK_CANDIDATE ? end[i] != MARKDUP_NO_END : dup[i] == 0;
}

__global__ __launch_bounds__(BT) void k_markdup_list_flag(const uint64_t *__restrict__ end, const uint32_t *__restrict__ mate, const uint8_t *__restrict__ dup,
                                                          uint64_t n, uint32_t kind, uint64_t *__restrict__ flag) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (i == 0) flag[n] = 0;
    if (i < n) flag[i] = of_kind(end, mate, dup, i, kind) ? 1 : 0;
}

__global__ __launch_bounds__(BT) void k_markdup_list_fill(const uint64_t *__restrict__ end, const uint32_t *__restrict__ mate, const uint8_t *__restrict__ dup,
                                                          uint64_t n, uint32_t kind, const uint64_t *__restrict__ flag, uint32_t *__restrict__ list) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (i < n && of_kind(end, mate, dup, i, kind)) list[flag[i]] = (uint32_t)i;
}

// the low word of a value: larger for the smaller index, and never all ones (i + 1 >= 1), so that ~0 stays a pair member's
__device__ __forceinline__ uint64_t value_of(uint32_t score, uint32_t i) { return (uint64_t)score << 32 | (uint32_t)~(i + 1u); }

__global__ __launch_bounds__(BT) void k_markdup_entry_keys(const uint32_t *__restrict__ list, uint64_t m, const uint32_t *__restrict__ mate,
                                                           const uint64_t *__restrict__ end, const uint32_t *__restrict__ score, uint64_t *__restrict__ hi,
                                                           uint64_t *__restrict__ lo, uint64_t *__restrict__ val) {
    const uint64_t e = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (e >= m) return;
    const uint32_t i = list[e], j = mate[i];
    if (hi) {
        const uint64_t a = end[i], b = end[j];
        hi[e] = max(a, b);
        lo[e] = min(a, b);
        val[e] = value_of(score[i] + score[j], i);
    } else {
        lo[e] = end[i];
        val[e] = j != COLLATE_NONE ? ~0ull : value_of(score[i], i);
    }
}

__global__ __launch_bounds__(BT) void k_markdup_gather(const uint64_t *__restrict__ src, const uint32_t *__restrict__ perm, uint64_t m, uint64_t *__restrict__ dst) {
    const uint64_t q = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (q < m) dst[q] = src[perm[q]];
}

__global__ __launch_bounds__(BT) void k_markdup_compose(const uint32_t *__restrict__ first, const uint32_t *__restrict__ second, uint64_t m, uint32_t *__restrict__ out) {
    const uint64_t r = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (r < m) out[r] = first[second[r]];
}

__global__ __launch_bounds__(BT) void k_markdup_heads(const uint32_t *__restrict__ order, const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint64_t m,
                                                      uint64_t *__restrict__ flag) {
    const uint64_t r = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (r == 0) flag[m] = 0;
    if (r >= m) return;
    bool head = r == 0;
    if (!head) {
        const uint32_t a = order[r], b = order[r - 1];
        head = lo[a] != lo[b] || (hi && hi[a] != hi[b]);
    }
    flag[r] = head ? 1 : 0;
}

__global__ __launch_bounds__(BT) void k_markdup_best(const uint32_t *__restrict__ order, const uint64_t *__restrict__ run, const uint64_t *__restrict__ val, uint64_t m,
                                                     unsigned long long *best) {
    const uint64_t r = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (r < m) (void)atomicMax(&best[run[r + 1] - 1], (unsigned long long)val[order[r]]);
}

__global__ __launch_bounds__(BT) void k_markdup_mark(const uint32_t *__restrict__ order, const uint64_t *__restrict__ run, const uint64_t *__restrict__ val,
                                                     const unsigned long long *__restrict__ best, const uint32_t *__restrict__ list, const uint32_t *__restrict__ mate,
                                                     uint64_t m, bool pairs, uint8_t *__restrict__ dup, unsigned long long *work) {
    const uint64_t r = (uint64_t)blockIdx.x * BT + threadIdx.x;
    bool marked = false;
    if (r < m) {
        const uint32_t e = order[r], i = list[e], j = mate[i];
        if (val[e] != best[run[r + 1] - 1] && (pairs || j == COLLATE_NONE)) {
            marked = true;
            dup[i] = 1;
            if (pairs) dup[j] = 1;
        }
    }
    const uint32_t c = __popcll(__ballot(marked));
    if (c && lane_id() == 0) atomicAdd(&work[pairs ? MW_DUP_PAIRS : MW_DUP_FRAGMENTS], (unsigned long long)c);
}

__global__ __launch_bounds__(BT) void k_markdup_apply(const uint64_t *__restrict__ addr, const uint8_t *__restrict__ dup, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (i >= n) return;
    uint8_t *p = reinterpret_cast<uint8_t *>((uintptr_t)addr[i]) + 19;
    *p = (uint8_t)((*p & ~0x4u) | (dup[i] ? 0x4u : 0u));
}

__global__ void k_markdup_words(const unsigned long long *__restrict__ work, unsigned long long *host) {
    if (threadIdx.x < MARKDUP_WORK_WORDS) host[threadIdx.x] = work[threadIdx.x];
}

uint32_t blocks_of(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }
bool countable(uint64_t n) { return n && n <= 0xFFFFFFFFull; }

} // namespace

hipError_t launch_markdup_ends(const uint64_t *addr, uint64_t n, uint8_t *cls, uint64_t *end, uint32_t *score, unsigned long long *work, hipStream_t s) {
    if (!countable(n)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_markdup_ends, dim3(blocks_of(n, WAVES)), dim3(BT), 0, s, addr, n, cls, end, score, work);
    return hipGetLastError();
}

hipError_t launch_markdup_key(const uint64_t *addr, const uint8_t *cls, const uint64_t *end, uint64_t n, uint32_t hash_bits, uint64_t *key,
                              unsigned long long *work, hipStream_t s) {
    if (!countable(n) || hash_bits > 63u) return hipErrorInvalidValue;
    const uint64_t mask = hash_bits ? ((uint64_t)1 << hash_bits) - 1 : ~0ull >> 1;
    hipLaunchKernelGGL(k_markdup_key, dim3(blocks_of(n, BT)), dim3(BT), 0, s, addr, cls, end, n, mask, key, work);
    return hipGetLastError();
}

hipError_t launch_markdup_list_flag(const uint64_t *end, const uint32_t *mate, const uint8_t *dup, uint64_t n, uint32_t kind, uint64_t *flag, hipStream_t s) {
    if (!countable(n) || kind > MK_SURVIVOR) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_markdup_list_flag, dim3(blocks_of(n, BT)), dim3(BT), 0, s, end, mate, dup, n, kind, flag);
    return hipGetLastError();
}

hipError_t launch_markdup_list_fill(const uint64_t *end, const uint32_t *mate, const uint8_t *dup, uint64_t n, uint32_t kind, const uint64_t *flag,
                                    uint32_t *list, hipStream_t s) {
    if (!countable(n) || kind > MK_SURVIVOR) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_markdup_list_fill, dim3(blocks_of(n, BT)), dim3(BT), 0, s, end, mate, dup, n, kind, flag, list);
    return hipGetLastError();
}

hipError_t launch_markdup_entry_keys(const uint32_t *list, uint64_t m, const uint32_t *mate, const uint64_t *end, const uint32_t *score, uint64_t *hi,
                                     uint64_t *lo, uint64_t *val, hipStream_t s) {
    if (!countable(m)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_markdup_entry_keys, dim3(blocks_of(m, BT)), dim3(BT), 0, s, list, m, mate, end, score, hi, lo, val);
    return hipGetLastError();
}

hipError_t launch_markdup_gather(const uint64_t *src, const uint32_t *perm, uint64_t m, uint64_t *dst, hipStream_t s) {
    if (!countable(m)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_markdup_gather, dim3(blocks_of(m, BT)), dim3(BT), 0, s, src, perm, m, dst);
    return hipGetLastError();
}

hipError_t launch_markdup_compose(const uint32_t *first, const uint32_t *second, uint64_t m, uint32_t *out, hipStream_t s) {
    if (!countable(m)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_markdup_compose, dim3(blocks_of(m, BT)), dim3(BT), 0, s, first, second, m, out);
    return hipGetLastError();
}

hipError_t launch_markdup_heads(const uint32_t *order, const uint64_t *hi, const uint64_t *lo, uint64_t m, uint64_t *flag, hipStream_t s) {
    if (!countable(m)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_markdup_heads, dim3(blocks_of(m, BT)), dim3(BT), 0, s, order, hi, lo, m, flag);
    return hipGetLastError();
}

hipError_t launch_markdup_best(const uint32_t *order, const uint64_t *run, const uint64_t *val, uint64_t m, unsigned long long *best, hipStream_t s) {
    if (!countable(m)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_markdup_best, dim3(blocks_of(m, BT)), dim3(BT), 0, s, order, run, val, m, best);
    return hipGetLastError();
}

hipError_t launch_markdup_mark(const uint32_t *order, const uint64_t *run, const uint64_t *val, const unsigned long long *best, const uint32_t *list,
                               const uint32_t *mate, uint64_t m, bool pairs, uint8_t *dup, unsigned long long *work, hipStream_t s) {
    if (!countable(m)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_markdup_mark, dim3(blocks_of(m, BT)), dim3(BT), 0, s, order, run, val, best, list, mate, m, pairs, dup, work);
    return hipGetLastError();
}

hipError_t launch_markdup_apply(const uint64_t *addr, const uint8_t *dup, uint64_t n, hipStream_t s) {
    if (!countable(n)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_markdup_apply, dim3(blocks_of(n, BT)), dim3(BT), 0, s, addr, dup, n);
    return hipGetLastError();
}

hipError_t launch_markdup_words(const unsigned long long *work, unsigned long long *host, hipStream_t s) {
    hipLaunchKernelGGL(k_markdup_words, dim3(1), dim3(64), 0, s, work, host);
    return hipGetLastError();
}

} // namespace ngsq
