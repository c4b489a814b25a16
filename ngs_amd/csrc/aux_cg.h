// aux_cg.h -- the long-CIGAR tag on the device (SAM specification 4.2.2): where a record's CG:B,I tag keeps its operations.
// k_rec_fixed (bam_device.hip) and k_bai_sorted (bai_kernel.hip) resolve the placeholder <l_seq>S<span>N through it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ngsq {

// bam_reader.h aux_find_cg, on the device (only the rare lane whose CIGAR is the long-CIGAR placeholder walks its tags):
// offset from p of the CG:B,I tag's operations and their number, or 0
__device__ inline uint64_t aux_find_cg(const uint8_t *p0, const uint8_t *end, uint32_t *n_ops) {
    const uint8_t *p = p0;
    while (end - p >= 4) {
        const uint8_t t0 = p[0], t1 = p[1], ty = p[2];
        p += 3;
        uint64_t n = 0;
        if (ty == 'A' || ty == 'c' || ty == 'C') n = 1;
        else if (ty == 's' || ty == 'S') n = 2;
        else if (ty == 'i' || ty == 'I' || ty == 'f') n = 4;
        else if (ty == 'Z' || ty == 'H') {
            while (p < end && *p) p++;
            if (p >= end) return 0;
            n = 1;
        } else if (ty == 'B') {
            if (end - p < 5) return 0;
            const uint8_t sub = p[0];
            const uint32_t cnt = (uint32_t)p[1] | (uint32_t)p[2] << 8 | (uint32_t)p[3] << 16 | (uint32_t)p[4] << 24;
            const uint32_t w = sub == 'c' || sub == 'C' ? 1 : sub == 's' || sub == 'S' ? 2 : sub == 'i' || sub == 'I' || sub == 'f' ? 4 : 0;
            if (!w) return 0;
            n = 5 + (uint64_t)cnt * w;
            if (t0 == 'C' && t1 == 'G' && sub == 'I') {
                if ((uint64_t)(end - p) < n) return 0;
                *n_ops = cnt;
                return (uint64_t)(p + 5 - p0);
            }
        } else {
            return 0;
        }
        if ((uint64_t)(end - p) < n) return 0;
        p += n;
    }
    return 0;
}

} // namespace ngsq
