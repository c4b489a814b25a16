// name_key.h -- the read name of a resident record as the mate search sees it: where the record's body
// lies, how many bytes its name has, the 64-bit hash that becomes the sort key, and the exact comparison made inside a run of
// equal keys.  Shared by the kernels of `ngs fastq --collate` (collate_kernel.hip) and `ngs markdup` (markdup_kernel.hip), so that
// both pair mates by one rule.  Only a .hip file includes this.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ngsq {

__device__ __forceinline__ const uint8_t *body_at(const uint64_t *addr, uint64_t i) { return reinterpret_cast<const uint8_t *>((uintptr_t)addr[i]) + 4; }
__device__ __forceinline__ uint32_t name_bytes(const uint8_t *body) { return body[8] ? body[8] - 1u : 0u; }

// a 64-bit hash of the name's bytes and their number: eight bytes a step, the rest by bytes; nothing behind the name is read
__device__ __forceinline__ uint64_t name_hash(const uint8_t *name, uint32_t qn) {
    constexpr uint64_t M = 0x9E3779B97F4A7C15ull;
    uint64_t h = 0x243F6A8885A308D3ull ^ qn;
    uint32_t k = 0;
    for (; k + 8 <= qn; k += 8) {
        uint64_t w;
        __builtin_memcpy(&w, name + k, 8);
        h = (h ^ w) * M;
        h ^= h >> 29;
    }
    uint64_t w = 0;
    for (uint32_t q = 0; k + q < qn; q++) w |= (uint64_t)name[k + q] << (8u * q);
    h = (h ^ w) * M;
    h ^= h >> 32;
    h *= 0xD6E8FEB86659FD93ull;
    h ^= h >> 32;
    return h;
}

__device__ __forceinline__ bool same_name(const uint8_t *a, const uint8_t *b, uint32_t qn) {
    for (uint32_t k = 0; k < qn; k++)
        if (a[k] != b[k]) return false;
    return true;
}

} // namespace ngsq
