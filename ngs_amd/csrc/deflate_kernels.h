// deflate_kernels.h -- the device DEFLATE encoder: a device buffer becomes complete BGZF blocks, written
// compacted in input order.  Launcher only; bgzf_deflate.hip has the kernels, bgzf_deflate.cpp the public entry.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "ingest_consumer.h" // ScanScratch, DevArray

namespace ngsq {

constexpr uint32_t DEFLATE_BLOCK_INPUT = 65280;  // input bytes of a block (htslib's): a stored block always fits BSIZE
constexpr uint32_t DEFLATE_MEMBER_EXTRA = 18 + 8; // gzip header with the BC field, CRC32 and ISIZE
constexpr uint32_t DEFLATE_STORED_EXTRA = 5;      // BFINAL/BTYPE byte, LEN, NLEN
// The input buffer must be readable for DEFLATE_IN_SLACK bytes past its last byte: the match compare reads eight bytes at a
// time and clips the length afterwards.  What it reads there never reaches the output.
constexpr uint32_t DEFLATE_IN_SLACK = 16;
constexpr uint32_t DEFLATE_STAGE_STRIDE = 65536;  // bytes of a block's staged payload (a dynamic payload is shorter than the stored form)
enum DeflateEffort : uint32_t { DEFLATE_EFFORT_NORMAL = 0, DEFLATE_EFFORT_HIGH = 1 }; // (NGSQ_BGZF_EFFORT_*, include/ngsq_bgzf.h)
constexpr uint32_t DEFLATE_CHAIN_K = 8; // candidates a position walks along its hash chain at high effort
enum DeflateHost : uint32_t { DH_BYTES = 0, DH_STORED, DH_TOKENS, DH_MATCHES, DEFLATE_HOST_WORDS };

extern const uint8_t BGZF_EOF_BLOCK[28]; // the EOF block of the specification (bgzf_deflate.cpp)

inline uint64_t deflate_blocks(uint64_t n) { return (n + DEFLATE_BLOCK_INPUT - 1) / DEFLATE_BLOCK_INPUT; }
// most bytes the blocks of n input bytes take (every block stored)
inline uint64_t deflate_bound(uint64_t n) { return n + deflate_blocks(n) * (DEFLATE_MEMBER_EXTRA + DEFLATE_STORED_EXTRA); }

// the device arrays a caller keeps between launches on one stream
struct DeflateScratch {
    DevArray<uint8_t> stage;       // [blocks * DEFLATE_STAGE_STRIDE] payloads before they are packed
    DevArray<uint16_t> dist;       // [grid * 65536] match distances of the block a workgroup is working on
    DevArray<uint16_t> link;       // [grid * 65536] high effort only: a position's link to the previous one of its hash
    DevArray<uint64_t> off;        // [blocks + 1] member sizes, then their offsets
    DevArray<uint32_t> crc, flags; // [blocks]
    DevArray<unsigned long long> work; // ticket, stored blocks, tokens, matches
    ScanScratch scan;
};

// in[0, n) (device, DEFLATE_IN_SLACK readable bytes behind it) -> out (device, room for deflate_bound(n) bytes): one BGZF block
// per DEFLATE_BLOCK_INPUT bytes, no EOF block.  host (pinned, device address): DEFLATE_HOST_WORDS words, written by the last
// kernel; host[DH_BYTES] = bytes written to out.  ev (optional, four timing events): recorded in front of the encoder, the CRC,
// the pack and behind it.  effort: a DeflateEffort; DEFLATE_EFFORT_HIGH searches harder for matches and never writes a larger
// block.  The output bytes depend on the input bytes and the effort alone.
hipError_t launch_bgzf_deflate(const uint8_t *in, uint64_t n, uint8_t *out, DeflateScratch &sc, unsigned long long *host, uint32_t effort,
                               hipStream_t s, hipEvent_t *ev = nullptr);

} // namespace ngsq
