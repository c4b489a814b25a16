// collate_kernel.hip -- `ngs fastq --collate` on the device.  The walk's kernels see a batch of the device
// ingest: a thread per record decides what is kept (fastq_route's rules), a wave per kept record checks its scores.  The match's
// kernels see the resident records through their addresses: a thread per record hashes its name into a sort key, and after the
// sort a thread per rank searches the run of its key for records of its own name, comparing bytes, so that a collision of the
// hash costs time and never a wrong pair.  The lists and the pieces' size pass are a thread per entry, the write pass is a wave
// per record through fastq_format.h's formatter.  collate.cpp drives them.
#include <hip/hip_runtime.h>

#include "collate_kernels.h"
#include "fastq_format.h"
#include "name_key.h"

namespace ngsq {

namespace {

constexpr uint32_t BT = 256;
constexpr uint32_t WAVES = BT / 64;

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ uint32_t class_of(uint32_t flag) { return (flag & 0xC0u) == 0x40u ? CLASS_ONE : (flag & 0xC0u) == 0x80u ? CLASS_TWO : CLASS_OTHER; }

__global__ __launch_bounds__(BT) void k_collate_flag(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ rec_off, uint64_t n, FastqRules R,
                                                     uint64_t *__restrict__ cnt, uint64_t *__restrict__ bytes, unsigned long long *work) {
    __shared__ unsigned int tally[COLLATE_WORK_WORDS];
    if (threadIdx.x < COLLATE_WORK_WORDS) tally[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    const bool in = i < n;
    FastqFate fate = FATE_EXCLUDED;
    uint32_t cls = CLASS_OTHER, out = 0;
    if (in) {
        const uint8_t *p = raw + rec_off[i];
        fate = fastq_route(fq_ld16u(p + 18), fq_ld32u(p + 20), R, &cls, &out); // (R.two_files is 0: nothing is dropped here)
        const bool kept = fate == FATE_WRITTEN;
        cnt[i] = kept ? 1 : 0;
        bytes[i] = kept ? 4ull + fq_ld32u(p) : 0;
        if (i == 0) cnt[n] = bytes[n] = 0;
    }
    const bool kept = in && fate == FATE_WRITTEN;
    const uint32_t c_excl = __popcll(__ballot(in && fate == FATE_EXCLUDED)), c_noseq = __popcll(__ballot(in && fate == FATE_NO_SEQUENCE)),
                   c_one = __popcll(__ballot(kept && cls == CLASS_ONE)), c_two = __popcll(__ballot(kept && cls == CLASS_TWO)),
                   c_other = __popcll(__ballot(kept && cls == CLASS_OTHER));
    if (lane_id() == 0) {
        if (c_excl) atomicAdd(&tally[CW_EXCLUDED], c_excl);
        if (c_noseq) atomicAdd(&tally[CW_NO_SEQUENCE], c_noseq);
        if (c_one) atomicAdd(&tally[CW_ONE], c_one);
        if (c_two) atomicAdd(&tally[CW_TWO], c_two);
        if (c_other) atomicAdd(&tally[CW_OTHER], c_other);
    }
    __syncthreads();
    if (threadIdx.x >= CW_EXCLUDED && threadIdx.x <= CW_OTHER && tally[threadIdx.x]) atomicAdd(&work[threadIdx.x], (unsigned long long)tally[threadIdx.x]);
}

__global__ __launch_bounds__(BT) void k_collate_qual(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ rec_off, uint64_t n,
                                                     const uint64_t *__restrict__ cnt, uint64_t first_index, unsigned long long *work) {
    const uint64_t r = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (r >= n || cnt[r + 1] == cnt[r]) return; // (a whole wave: r is the wave's)
    const uint8_t *body = raw + rec_off[r] + 4;
    const uint32_t l_rn = body[8], n_ops = fq_ld16u(body + 12), l = fq_ld32u(body + 16);
    const uint8_t *qual = body + 32 + l_rn + 4ull * n_ops + ((uint64_t)l + 1) / 2;
    if (qual[0] == 0xFF) return; // no QUAL: nothing to check
    bool bad = false;
    for (uint64_t k = lane_id(); k < l; k += 64) bad |= qual[k] > 93u;
    if (__any(bad) && lane_id() == 0) (void)atomicMin(&work[CW_BAD], (unsigned long long)(first_index + r) << FASTQ_ERR_BITS | FASTQ_E_QUAL);
}

__global__ __launch_bounds__(BT) void k_collate_key(const uint64_t *__restrict__ addr, uint64_t n, uint64_t mask, uint64_t *__restrict__ key,
                                                    uint8_t *__restrict__ cls) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (i >= n) return;
    const uint8_t *body = body_at(addr, i);
    const uint32_t c = class_of(fq_ld16u(body + 14));
    cls[i] = (uint8_t)c;
    key[i] = c == CLASS_OTHER ? COLLATE_KEY_OTHER : name_hash(body + 32, name_bytes(body)) & mask;
}

__global__ __launch_bounds__(BT) void k_collate_run_limit(const uint64_t *__restrict__ skey, uint64_t n, unsigned long long *work) {
    const uint64_t r = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (r + COLLATE_MAX_RUN >= n) return;
    const uint64_t k = skey[r];
    if (k != COLLATE_KEY_OTHER && k == skey[r + COLLATE_MAX_RUN]) work[CW_LONG_RUN] = 1ull;
}

__global__ __launch_bounds__(BT) void k_collate_match(const uint64_t *__restrict__ skey, const uint32_t *__restrict__ perm, const uint64_t *__restrict__ addr,
                                                      const uint8_t *__restrict__ cls, uint64_t n, uint32_t *__restrict__ mate, unsigned long long *work) {
    const uint64_t r = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (r >= n) return;
    const uint32_t i = perm[r];
    const uint32_t c = cls[i];
    if (c == CLASS_OTHER) {
        mate[i] = COLLATE_NONE;
        return;
    }
    const uint64_t key = skey[r];
    const uint8_t *body = body_at(addr, i);
    const uint32_t qn = name_bytes(body);
    uint32_t ones = c == CLASS_ONE ? 1u : 0u, twos = c == CLASS_TWO ? 1u : 0u, partner = COLLATE_NONE;
    bool collided = false;
    auto visit = [&](uint64_t q) {
        const uint32_t j = perm[q];
        const uint8_t *bj = body_at(addr, j);
        if (name_bytes(bj) == qn && same_name(body + 32, bj + 32, qn)) {
            const uint32_t cj = cls[j];
            ones += cj == CLASS_ONE ? 1u : 0u;
            twos += cj == CLASS_TWO ? 1u : 0u;
            if (cj != c) partner = j;
        } else {
            collided = true;
        }
    };
    // (a run holds at most COLLATE_MAX_RUN records: the driver has refused a longer one)
    for (uint64_t q = r; q > 0 && skey[q - 1] == key; q--) visit(q - 1);
    for (uint64_t q = r + 1; q < n && skey[q] == key; q++) visit(q);
    mate[i] = ones == 1u && twos == 1u ? partner : COLLATE_NONE;
    if (ones > 1u || twos > 1u) atomicAdd(&work[CW_AMBIGUOUS], 1ull);
    if (collided) atomicAdd(&work[CW_COLLISIONS], 1ull);
}

__device__ __forceinline__ bool of_kind(uint32_t c, uint32_t m, uint64_t i, uint32_t kind) {
    if (kind == CK_OTHER) return c == CLASS_OTHER;
    if (c == CLASS_OTHER) return false;
    return kind == CK_LEAD ? m != COLLATE_NONE && m > i : m == COLLATE_NONE;
}

__global__ __launch_bounds__(BT) void k_collate_list_flag(const uint8_t *__restrict__ cls, const uint32_t *__restrict__ mate, uint64_t n, uint32_t kind,
                                                          uint64_t *__restrict__ flag) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (i == 0) flag[n] = 0;
    if (i < n) flag[i] = of_kind(cls[i], mate[i], i, kind) ? 1 : 0;
}

__global__ __launch_bounds__(BT) void k_collate_list_fill(const uint8_t *__restrict__ cls, const uint32_t *__restrict__ mate, uint64_t n, uint32_t kind,
                                                          const uint64_t *__restrict__ flag, uint32_t *__restrict__ list) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (i < n && of_kind(cls[i], mate[i], i, kind)) list[flag[i]] = (uint32_t)i;
}

__device__ __forceinline__ uint64_t text_bytes_of(const CollatePiece &p, uint32_t i, const FastqRules &R) {
    const uint8_t *body = body_at(p.addr, i);
    return fastq_record_bytes(body[8], fq_ld32u(body + 16), p.cls[i], R);
}
// the read one and the read two of the pair that record i leads
__device__ __forceinline__ void pair_of(const CollatePiece &p, uint32_t i, uint32_t *one, uint32_t *two) {
    const uint32_t j = p.mate[i];
    const bool first = p.cls[i] == CLASS_ONE;
    *one = first ? i : j;
    *two = first ? j : i;
}

__global__ __launch_bounds__(BT) void k_collate_size(CollatePiece p, FastqRules R, uint64_t *__restrict__ len_a, uint64_t *__restrict__ len_b) {
    const uint64_t e = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (e == 0) {
        len_a[p.m] = 0;
        if (len_b) len_b[p.m] = 0;
    }
    if (e >= p.m) return;
    const uint32_t i = p.list[e];
    if (p.mode == CM_RECORD) {
        len_a[e] = text_bytes_of(p, i, R);
        return;
    }
    uint32_t one, two;
    pair_of(p, i, &one, &two);
    const uint64_t a = text_bytes_of(p, one, R), b = text_bytes_of(p, two, R);
    if (p.mode == CM_SPLIT) {
        len_a[e] = a;
        len_b[e] = b;
    } else {
        len_a[e] = a + b;
    }
}

__global__ __launch_bounds__(BT) void k_collate_write(CollatePiece p, FastqRules R, const uint64_t *__restrict__ off_a, const uint64_t *__restrict__ off_b,
                                                      char *__restrict__ text_a, char *__restrict__ text_b) {
    const uint64_t w = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    const bool pairs = p.mode != CM_RECORD;
    const uint64_t e = pairs ? w >> 1 : w;
    if (e >= p.m) return; // (a whole wave: e is the wave's)
    uint32_t i = p.list[e];
    char *dst = text_a + off_a[e];
    if (pairs) {
        uint32_t one, two;
        pair_of(p, i, &one, &two);
        if (w & 1u) {
            i = two;
            dst = p.mode == CM_SPLIT ? text_b + off_b[e] : dst + text_bytes_of(p, one, R);
        } else {
            i = one;
        }
    }
    const uint8_t *body = body_at(p.addr, i);
    (void)fastq_format_record(body, p.cls[i], R, dst, lane_id()); // (the walk has checked the scores)
}

__global__ void k_collate_words(const unsigned long long *__restrict__ work, unsigned long long *host) {
    if (threadIdx.x < COLLATE_WORK_WORDS) host[threadIdx.x] = work[threadIdx.x];
}

uint32_t blocks_of(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

} // namespace

hipError_t launch_collate_flag(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, const FastqRules &r, uint64_t *cnt, uint64_t *bytes,
                               unsigned long long *work, hipStream_t s) {
    if (!n || n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_collate_flag, dim3(blocks_of(n, BT)), dim3(BT), 0, s, raw, rec_off, n, r, cnt, bytes, work);
    return hipGetLastError();
}

hipError_t launch_collate_qual(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, const uint64_t *cnt, uint64_t first_index,
                               unsigned long long *work, hipStream_t s) {
    if (!n || n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_collate_qual, dim3(blocks_of(n, WAVES)), dim3(BT), 0, s, raw, rec_off, n, cnt, first_index, work);
    return hipGetLastError();
}

hipError_t launch_collate_key(const uint64_t *addr, uint64_t n, uint32_t hash_bits, uint64_t *key, uint8_t *cls, hipStream_t s) {
    if (!n || n > 0xFFFFFFFFull || hash_bits > 63u) return hipErrorInvalidValue;
    const uint64_t mask = hash_bits ? ((uint64_t)1 << hash_bits) - 1 : ~0ull >> 1;
    hipLaunchKernelGGL(k_collate_key, dim3(blocks_of(n, BT)), dim3(BT), 0, s, addr, n, mask, key, cls);
    return hipGetLastError();
}

hipError_t launch_collate_run_limit(const uint64_t *skey, uint64_t n, unsigned long long *work, hipStream_t s) {
    if (n <= COLLATE_MAX_RUN) return hipSuccess;
    if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_collate_run_limit, dim3(blocks_of(n - COLLATE_MAX_RUN, BT)), dim3(BT), 0, s, skey, n, work);
    return hipGetLastError();
}

hipError_t launch_collate_match(const uint64_t *skey, const uint32_t *perm, const uint64_t *addr, const uint8_t *cls, uint64_t n, uint32_t *mate,
                                unsigned long long *work, hipStream_t s) {
    if (!n || n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_collate_match, dim3(blocks_of(n, BT)), dim3(BT), 0, s, skey, perm, addr, cls, n, mate, work);
    return hipGetLastError();
}

hipError_t launch_collate_list_flag(const uint8_t *cls, const uint32_t *mate, uint64_t n, uint32_t kind, uint64_t *flag, hipStream_t s) {
    if (!n || n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_collate_list_flag, dim3(blocks_of(n, BT)), dim3(BT), 0, s, cls, mate, n, kind, flag);
    return hipGetLastError();
}

hipError_t launch_collate_list_fill(const uint8_t *cls, const uint32_t *mate, uint64_t n, uint32_t kind, const uint64_t *flag, uint32_t *list,
                                    hipStream_t s) {
    if (!n || n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_collate_list_fill, dim3(blocks_of(n, BT)), dim3(BT), 0, s, cls, mate, n, kind, flag, list);
    return hipGetLastError();
}

hipError_t launch_collate_size(const CollatePiece &p, const FastqRules &r, uint64_t *len_a, uint64_t *len_b, hipStream_t s) {
    if (!p.m || p.m > 0xFFFFFFFFull || (p.mode == CM_SPLIT && !len_b)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_collate_size, dim3(blocks_of(p.m, BT)), dim3(BT), 0, s, p, r, len_a, p.mode == CM_SPLIT ? len_b : nullptr);
    return hipGetLastError();
}

hipError_t launch_collate_write(const CollatePiece &p, const FastqRules &r, const uint64_t *off_a, const uint64_t *off_b, char *text_a, char *text_b,
                                hipStream_t s) {
    if (!p.m || p.m > 0xFFFFFFFFull || (p.mode == CM_SPLIT && (!off_b || !text_b))) return hipErrorInvalidValue;
    const uint64_t waves = p.mode == CM_RECORD ? p.m : 2 * p.m;
    hipLaunchKernelGGL(k_collate_write, dim3(blocks_of(waves, WAVES)), dim3(BT), 0, s, p, r, off_a, off_b, text_a, text_b);
    return hipGetLastError();
}

hipError_t launch_collate_words(const unsigned long long *work, unsigned long long *host, hipStream_t s) {
    hipLaunchKernelGGL(k_collate_words, dim3(1), dim3(64), 0, s, work, host);
    return hipGetLastError();
}

} // namespace ngsq
