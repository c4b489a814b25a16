// bgzf_crc.h -- the gzip CRC32 of one BGZF block by one wavefront: what k_bgzf_crc (bgzf_inflate.hip) compares with a block's
// trailer and k_deflate_crc (bgzf_deflate.hip) stores into one.  Device code: include from a .hip file, inside no namespace.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ngsq {

// x^(8 S 2^j) mod P for every slice length S <= CRC_MAX_SLICE and combination step j < 6, on the current device (computed once
// per device and process; bgzf_inflate.hip)
hipError_t bgzf_crc_pow_table(const uint32_t **tab);

namespace {

// ---- CRC32 (gzip): GF(2) helpers in the reflected representation -----------------------------
constexpr uint32_t CRC_POLY = 0xEDB88320u;
// Slicing tables: t[k][b] = register after byte b followed by k zero bytes.  Sixteen bytes are then folded with sixteen
// INDEPENDENT lookups (one LDS round trip) where the byte-wise table needs sixteen dependent ones: k_bgzf_crc was bound
// by exactly that latency (0.98 ms per 520 MB; 16 KiB of tables per workgroup instead of 1 KiB).
constexpr uint32_t CRC_SLICES = 16;
struct CrcTable {
    uint32_t t[CRC_SLICES][256];
    constexpr CrcTable() : t() {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
            t[0][i] = c;
        }
        for (uint32_t k = 1; k < CRC_SLICES; k++)
            for (uint32_t i = 0; i < 256; i++) t[k][i] = (t[k - 1][i] >> 8) ^ t[0][t[k - 1][i] & 0xFFu];
    }
};
// (copied to LDS by the kernels: crc_load_tables)
__constant__ CrcTable c_crc;
__device__ __forceinline__ uint32_t ld32u(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__host__ __device__ inline uint32_t crc_mul(uint32_t a, uint32_t b) { // a * b mod P
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
__host__ __device__ inline uint32_t crc_xpow8(uint32_t n_bytes) { // x^(8 n) mod P
    uint32_t r = 1u << 31, sq = 0x00800000u;      // x^0, x^8
    for (uint32_t e = n_bytes; e; e >>= 1) {
        if (e & 1u) r = crc_mul(r, sq);
        sq = crc_mul(sq, sq);
    }
    return r;
}

constexpr uint32_t CRC_WAVES = 8; // BGZF blocks per workgroup: the tables are loaded once for all of them
constexpr uint32_t CRC_MAX_SLICE = 1024; // bytes of one of the 64 slices of a block (ISIZE <= 65536)

// the slicing tables into s_tab[CRC_SLICES * 256], by the whole workgroup (of n_threads); the caller's barrier follows
__device__ __forceinline__ void crc_load_tables(uint32_t *s_tab, uint32_t n_threads) {
    for (uint32_t k = threadIdx.x; k < CRC_SLICES * 256; k += n_threads) s_tab[k] = c_crc.t[k >> 8][k & 0xFFu];
}

// CRC32 of p[0, isize) by one wavefront; the value (every lane's).  The block is cut into 64
// equal slices, right-aligned (the CRC register is linear in the message once the initial value is
// accounted for, and leading zero bytes leave a zero register at zero): the lane that holds byte 0
// starts from 0xFFFFFFFF, the others from 0, and the slices are combined pairwise in six steps,
// register(A || B) = register(A) * x^(8 |B|) + register(B), with |B| the same for every pair of a step.
// isize is wave-uniform and at most 64 * CRC_MAX_SLICE.
__device__ __forceinline__ uint32_t crc_wave_block(const uint8_t *p, uint32_t isize, uint32_t lane, const uint32_t *s_tab,
                                                   const uint32_t *__restrict__ pow_tab) {
    const uint32_t S = (isize + 63u) / 64u, pad = 64u * S - isize;
    // real bytes of this lane's slice
    const uint32_t v0 = lane * S, v1 = v0 + S;
    const uint32_t a = v0 > pad ? v0 - pad : 0u, b = v1 > pad ? v1 - pad : 0u;
    uint32_t c = (a == 0 && b > 0) ? 0xFFFFFFFFu : 0u;
    // 64 bytes per step into registers: every lane walks its own slice, so with narrower loads a cache line
    // would be fetched again for each of them (the 64 lanes' lines of a step do not fit the vector cache)
    uint32_t i = a;
    for (; i + 64 <= b; i += 64) {
        uint32_t w[16];
        __builtin_memcpy(w, p + i, 64);
#pragma unroll
        for (int k = 0; k < 16; k += 4) {
            const uint32_t x0 = c ^ w[k], x1 = w[k + 1], x2 = w[k + 2], x3 = w[k + 3];
            c = s_tab[15 * 256 + (x0 & 0xFFu)] ^ s_tab[14 * 256 + ((x0 >> 8) & 0xFFu)] ^ s_tab[13 * 256 + ((x0 >> 16) & 0xFFu)] ^
                s_tab[12 * 256 + (x0 >> 24)] ^ s_tab[11 * 256 + (x1 & 0xFFu)] ^ s_tab[10 * 256 + ((x1 >> 8) & 0xFFu)] ^
                s_tab[9 * 256 + ((x1 >> 16) & 0xFFu)] ^ s_tab[8 * 256 + (x1 >> 24)] ^ s_tab[7 * 256 + (x2 & 0xFFu)] ^
                s_tab[6 * 256 + ((x2 >> 8) & 0xFFu)] ^ s_tab[5 * 256 + ((x2 >> 16) & 0xFFu)] ^ s_tab[4 * 256 + (x2 >> 24)] ^
                s_tab[3 * 256 + (x3 & 0xFFu)] ^ s_tab[2 * 256 + ((x3 >> 8) & 0xFFu)] ^ s_tab[1 * 256 + ((x3 >> 16) & 0xFFu)] ^
                s_tab[x3 >> 24];
        }
    }
    for (; i + 4 <= b; i += 4) {
        const uint32_t x = c ^ ld32u(p + i);
        c = s_tab[3 * 256 + (x & 0xFFu)] ^ s_tab[2 * 256 + ((x >> 8) & 0xFFu)] ^ s_tab[1 * 256 + ((x >> 16) & 0xFFu)] ^ s_tab[x >> 24];
    }
    for (; i < b; i++) c = s_tab[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
    // pairwise combination: after step j the lanes whose low j+1 bits are ones hold 2^(j+1) slices.  The multiplier of step
    // j, x^(8 S 2^j), comes from a table (a slice has at most 1024 bytes): computed here -- a dozen GF(2) multiplications of 32
    // scalar steps each, per block -- it was half of this kernel's scalar instructions, on the unit the decoders are short of.
    const uint32_t *const pw = pow_tab + __builtin_amdgcn_readfirstlane(S) * 6u;
    for (uint32_t j = 0; j < 6; j++) {
        const uint32_t left = (uint32_t)__shfl_up((int)c, 1u << j, 64);
        if ((lane & ((2u << j) - 1u)) == (2u << j) - 1u) c = crc_mul(left, pw[j]) ^ c;
    }
    return ~__builtin_amdgcn_readlane(c, 63);
}

} // namespace
} // namespace ngsq
