// fastq_format.h -- the routing rule and the record formatter of `ngs fastq` as __device__ functions, for the kernels of
// `ngs fastq --collate` (collate_kernel.hip), which format resident records in pair order.  They are
// fastq_kernel.hip's fastq_route and the body of its k_fastq_write, statement for statement.  k_fastq_write itself does not
// call them: compiled through this function it takes 43 VGPRs where section 26.3 records 40 (no scratch and eight waves per
// SIMD either way), and the rule of that section is that the kernel keeps its figures, so it keeps its own body.  Whoever
// changes a line here changes it there; tests/test_fastq_collate_gpu.py holds both to tests/fastq_model.py's text.  Only a
// .hip file includes this.
#pragma once

#include <hip/hip_runtime.h>

#include "fastq_kernels.h"

namespace ngsq {

__device__ __forceinline__ uint32_t fq_ld32u(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ uint32_t fq_ld16u(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

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

// the bytes of a record's four lines: name + 2 l_seq + 6, 2 more with a suffix
__device__ __forceinline__ uint64_t fastq_record_bytes(uint32_t l_rn, uint32_t l_seq, uint32_t cls, const FastqRules &R) {
    const uint32_t sfx = R.name_suffix && cls != CLASS_OTHER ? 2u : 0u;
    return (uint64_t)(l_rn ? l_rn - 1 : 0) + 2ull * l_seq + 6ull + sfx;
}

// THE record formatter, a wave per record: the four lines of the record whose body (the bytes behind block_size) is at `body`,
// of class cls, at dst.  A lane takes one packed SEQ byte -- two letters -- and two scores per turn.  True in the lanes that
// met a present score above 93.
__device__ __forceinline__ bool fastq_format_record(const uint8_t *body, uint32_t cls, const FastqRules &R, char *dst, uint32_t lane) {
    const uint32_t l_rn = body[8], n_ops = fq_ld16u(body + 12), flag = fq_ld16u(body + 14), l = fq_ld32u(body + 16);
    const uint8_t *name = body + 32, *seq = name + l_rn + 4ull * n_ops, *qual = seq + ((uint64_t)l + 1) / 2;
    const uint32_t qn = l_rn ? l_rn - 1 : 0, sfx = R.name_suffix && cls != CLASS_OTHER ? 2u : 0u;
    // "@<name>[/1|/2]\n", then where the SEQ and the QUAL line begin
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
    return bad;
}

} // namespace ngsq
