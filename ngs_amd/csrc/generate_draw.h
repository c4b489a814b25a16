// generate_draw.h -- the draws of `ngs generate`, one definition for the kernels and the host:
// every random value is a pure function of (seed, pair index, purpose, attempt or base index).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NGSQ_GEN_HD __host__ __device__ __forceinline__
#else
#define NGSQ_GEN_HD inline
#endif

namespace ngsq {

// what a draw is for; the index beside it is the attempt (SEQUENCE, START, INNER), the base of the read (HIT_*, BASE_*) or 0
enum GenPurpose : uint32_t { GEN_PROVIDER = 0, GEN_SEQUENCE, GEN_START, GEN_INNER, GEN_HIT_ONE, GEN_BASE_ONE, GEN_HIT_TWO, GEN_BASE_TWO };

constexpr uint64_t GEN_GOLDEN = 0x9E3779B97F4A7C15ull;

// the splitmix64 finaliser
NGSQ_GEN_HD uint64_t gen_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// the pair's key: shared by all its draws
NGSQ_GEN_HD uint64_t gen_pair_key(uint64_t seed, uint64_t pair) { return gen_mix(seed ^ gen_mix(pair + GEN_GOLDEN)); }
NGSQ_GEN_HD uint64_t gen_draw(uint64_t key, uint32_t purpose, uint32_t index) {
    return gen_mix(key + GEN_GOLDEN * ((((uint64_t)purpose << 32) | index) + 1));
}
// an integer in [0, n): the high half of u * n
NGSQ_GEN_HD uint64_t gen_below(uint64_t u, uint64_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(u, n);
#else
    return (uint64_t)(((unsigned __int128)u * n) >> 64);
#endif
}

} // namespace ngsq
