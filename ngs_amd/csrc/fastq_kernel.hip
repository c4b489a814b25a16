// fastq_kernel.hip -- `ngs fastq` on the device: the four FASTQ lines of every kept record of a batch of
// the device ingest.  A record's length is closed-form (name + 2 l_seq + 6, 2 more with a suffix), so the size/classify pass
// is a thread per record that reads three fields; the offsets between the passes come from the ingest's exclusive scan, one
// per output.  The write pass is a wave per record: a lane takes one packed SEQ byte -- two letters -- and two scores per turn,
// a 100 kb read costs its own wave more turns.  Both passes route a record through fastq_route, so they agree by
// construction.  fastq.cpp drives them.
#include <hip/hip_runtime.h>

#include "fastq_kernels.h"

namespace ngsq {

namespace {

constexpr uint32_t BT = 256; // threads per block: 256 records of the size pass, four of the write pass
constexpr uint32_t RECS_PER_BLOCK = BT / 64;

__device__ __forceinline__ uint32_t ld32u(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ uint32_t ld16u(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

// "=ACMGRSVTWYHKDBN"[c] out of two registers
__device__ __forceinline__ char base_letter(uint32_t c) {
    const uint64_t t = c & 8u ? 0x4E42444B48595754ull : 0x565352474D43413Dull;
    return (char)(t >> ((c & 7u) * 8u));
}
// the complement of a 4-bit code: its four bits reversed
__device__ __forceinline__ uint32_t complement(uint32_t c) { return __brev(c) >> 28; }

enum FastqClass : uint32_t { CLASS_ONE = 0, CLASS_TWO, CLASS_OTHER };
enum FastqFate : uint32_t { FATE_EXCLUDED = 0, FATE_NO_SEQUENCE, FATE_DROPPED, FATE_WRITTEN };

// THE routing rule of include/ngsq_fastq.h: what becomes of a record with this flag and l_seq, its class, its output
__device__ __forceinline__ FastqFate fastq_route(uint32_t flag, uint32_t l_seq, const FastqRules &r, uint32_t *cls, uint32_t *out) {
    *cls = (flag & 0xC0u) == 0x40u ? CLASS_ONE : (flag & 0xC0u) == 0x80u ? CLASS_TWO : CLASS_OTHER;
    *out = r.two_files ? *cls : 0u;
    if ((flag & r.exclude) != 0 || (flag & r.require) != r.require) return FATE_EXCLUDED;
    if (!l_seq) return FATE_NO_SEQUENCE;
    if (r.two_files && *cls == CLASS_OTHER && !r.has_other) return FATE_DROPPED;
    return FATE_WRITTEN;
}

__global__ __launch_bounds__(BT) void k_fastq_size(ngsq_batch b, BatchOrigin o, FastqRules R, FastqOffsets len, unsigned long long *work) {
    __shared__ unsigned int tally[FASTQ_WORK_WORDS];
    if (threadIdx.x < FASTQ_WORK_WORDS) tally[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t n = b.n_records, i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    const bool in = i < n;
    FastqFate fate = FATE_EXCLUDED;
    uint32_t cls = CLASS_OTHER, out = 0;
    uint64_t bytes = 0;
    if (in) {
        const uint8_t *body = o.raw + o.rec_off[i] + 4;
        const uint32_t l_rn = body[8], flag = ld16u(body + 14), l = ld32u(body + 16);
        fate = fastq_route(flag, l, R, &cls, &out);
        const uint32_t sfx = R.name_suffix && cls != CLASS_OTHER ? 2u : 0u;
        bytes = (uint64_t)(l_rn ? l_rn - 1 : 0) + 2ull * l + 6ull + sfx;
#pragma unroll
        for (uint32_t k = 0; k < FASTQ_OUTPUTS; k++)
            if (len.v[k]) {
                len.v[k][i] = fate == FATE_WRITTEN && out == k ? bytes : 0;
                if (i == n - 1) len.v[k][n] = 0;
            }
    }
    // the batch's counts: a ballot per wave, the block's sums in LDS, one atomic per count and block
    const bool kept = in && (fate == FATE_WRITTEN || fate == FATE_DROPPED);
    const uint32_t c_excl = __popcll(__ballot(in && fate == FATE_EXCLUDED)), c_noseq = __popcll(__ballot(in && fate == FATE_NO_SEQUENCE)),
                   c_one = __popcll(__ballot(kept && cls == CLASS_ONE)), c_two = __popcll(__ballot(kept && cls == CLASS_TWO)),
                   c_other = __popcll(__ballot(kept && cls == CLASS_OTHER)), c_drop = __popcll(__ballot(in && fate == FATE_DROPPED));
    if (lane_id() == 0) {
        if (c_excl) atomicAdd(&tally[FW_EXCLUDED], c_excl);
        if (c_noseq) atomicAdd(&tally[FW_NO_SEQUENCE], c_noseq);
        if (c_one) atomicAdd(&tally[FW_ONE], c_one);
        if (c_two) atomicAdd(&tally[FW_TWO], c_two);
        if (c_other) atomicAdd(&tally[FW_OTHER], c_other);
        if (c_drop) atomicAdd(&tally[FW_DROPPED], c_drop);
    }
    __syncthreads();
    if (threadIdx.x > FW_BAD && threadIdx.x < FASTQ_WORK_WORDS && tally[threadIdx.x]) atomicAdd(&work[threadIdx.x], (unsigned long long)tally[threadIdx.x]);
}

__global__ void k_fastq_total(FastqOffsets off, uint64_t n, const unsigned long long *__restrict__ work, unsigned long long *host) {
    if (threadIdx.x < FASTQ_OUTPUTS) host[FH_BYTES + threadIdx.x] = off.v[threadIdx.x] ? off.v[threadIdx.x][n] : 0ull;
    if (threadIdx.x < FASTQ_WORK_WORDS) host[FH_WORK + threadIdx.x] = work[threadIdx.x];
}

__global__ void k_fastq_bad(const unsigned long long *__restrict__ work, unsigned long long *host) {
    if (threadIdx.x == 0) host[FH_WORK + FW_BAD] = work[FW_BAD];
}

__global__ __launch_bounds__(BT) void k_fastq_write(ngsq_batch b, BatchOrigin o, FastqRules R, FastqOffsets off, FastqText text,
                                                    unsigned long long *work) {
    const uint64_t i = (uint64_t)blockIdx.x * RECS_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= b.n_records) return; // (a whole wave: i is the wave's)
    const uint32_t lane = lane_id();
    const uint8_t *body = o.raw + o.rec_off[i] + 4;
    const uint32_t l_rn = body[8], n_ops = ld16u(body + 12), flag = ld16u(body + 14), l = ld32u(body + 16);
    uint32_t cls, out;
    if (fastq_route(flag, l, R, &cls, &out) != FATE_WRITTEN) return;
    const uint8_t *name = body + 32, *seq = name + l_rn + 4ull * n_ops, *qual = seq + ((uint64_t)l + 1) / 2;
    const uint32_t qn = l_rn ? l_rn - 1 : 0, sfx = R.name_suffix && cls != CLASS_OTHER ? 2u : 0u;
    // "@<name>[/1|/2]\n", then where the SEQ and the QUAL line begin
    char *dst = text.v[out] + off.v[out][i];
    for (uint32_t k = lane; k < qn; k += 64) dst[1 + k] = (char)name[k];
    char *const sq = dst + 1 + qn + sfx + 1, *const ql = sq + (uint64_t)l + 3;
    if (lane == 0) {
        dst[0] = '@';
        if (sfx) {
            dst[1 + qn] = '/';
            dst[2 + qn] = (char)('1' + cls);
        }
        sq[-1] = '\n';
        sq[l] = '\n';
        sq[(uint64_t)l + 1] = '+';
        sq[(uint64_t)l + 2] = '\n';
        ql[l] = '\n';
    }
    const bool rev = (flag & 0x10u) != 0, odd = (l & 1u) != 0;
    const bool no_qual = qual[0] == 0xFF; // htslib's test for absent qualities
    const uint64_t nb = ((uint64_t)l + 1) / 2;
    const char dq = (char)(R.default_quality + 33);
    bool bad = false;
    // turn j of a lane: the letters and scores of text positions 2 j and 2 j + 1
    for (uint64_t j = lane; j < nb; j += 64) {
        const uint64_t k0 = 2 * j;
        const bool two = k0 + 1 < l;
        uint32_t c0, c1;
        if (!rev) {
            const uint32_t x = seq[j];
            c0 = x >> 4;
            c1 = x & 15u;
        } else if (!odd) { // the pair is one packed byte from the end: nibbles swapped, each bit-reversed = the byte bit-reversed
            const uint32_t x = __brev((uint32_t)seq[nb - 1 - j]) >> 24;
            c0 = x >> 4;
            c1 = x & 15u;
        } else { // an odd length shifts the reversed read by half a byte: the high nibble of one byte, the low one of the byte in front
            c0 = complement((uint32_t)seq[nb - 1 - j] >> 4);
            c1 = two ? complement((uint32_t)seq[nb - 2 - j] & 15u) : 0u;
        }
        sq[k0] = base_letter(c0);
        if (two) sq[k0 + 1] = base_letter(c1);
        if (no_qual) {
            ql[k0] = dq;
            if (two) ql[k0 + 1] = dq;
        } else {
            const uint64_t a = rev ? (uint64_t)l - 1 - k0 : k0;
            const uint32_t q0 = qual[a], q1 = two ? qual[rev ? a - 1 : a + 1] : 0u;
            bad |= q0 > 93u || q1 > 93u;
            ql[k0] = (char)(q0 + 33);
            if (two) ql[k0 + 1] = (char)(q1 + 33);
        }
    }
    if (__any(bad) && lane == 0) (void)atomicMin(&work[FW_BAD], (unsigned long long)(b.first_record_index + i) << FASTQ_ERR_BITS | FASTQ_E_QUAL);
}

} // namespace

hipError_t launch_fastq_size(const ngsq_batch &b, const BatchOrigin &o, const FastqRules &r, const FastqOffsets &len, unsigned long long *work,
                             hipStream_t s) {
    if (!b.n_records) return hipSuccess;
    const uint64_t blocks = (b.n_records + BT - 1) / BT;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fastq_size, dim3((uint32_t)blocks), dim3(BT), 0, s, b, o, r, len, work);
    return hipGetLastError();
}

hipError_t launch_fastq_total(const FastqOffsets &off, uint64_t n, const unsigned long long *work, unsigned long long *host, hipStream_t s) {
    hipLaunchKernelGGL(k_fastq_total, dim3(1), dim3(64), 0, s, off, n, work, host);
    return hipGetLastError();
}

hipError_t launch_fastq_write(const ngsq_batch &b, const BatchOrigin &o, const FastqRules &r, const FastqOffsets &off, const FastqText &text,
                              unsigned long long *work, unsigned long long *host, hipStream_t s) {
    if (!b.n_records) return hipSuccess;
    const uint64_t blocks = (b.n_records + RECS_PER_BLOCK - 1) / RECS_PER_BLOCK;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fastq_write, dim3((uint32_t)blocks), dim3(BT), 0, s, b, o, r, off, text, work);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fastq_bad, dim3(1), dim3(64), 0, s, work, host);
    return hipGetLastError();
}

} // namespace ngsq
