// sort_kernels.h -- `ngs convert --sort coordinate` on the device: the keys of resident BAM records, a
// stable LSD radix sort of (key, index) pairs with 8-bit digits, and the gather of the records into sorted pieces.  Launchers
// only; sort_kernel.hip has the kernels, sort.cpp the sort's public entry, samsort.cpp and bamsort.cpp the drivers (SAM text and
// BAM in), sort_resident.h the phases they share.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "ingest_consumer.h" // ScanScratch, DevArray

namespace ngsq {

constexpr uint32_t SORT_DIGITS = 8;      // 8-bit digits of a 64-bit key, lowest first
constexpr uint32_t SORT_BINS = 256;
constexpr uint32_t SORT_BT = 512;        // threads of a ranking workgroup: eight waves
constexpr uint32_t SORT_ROUNDS = 8;      // keys a lane ranks: a wave takes 64 consecutive keys per round
constexpr uint32_t SORT_TILE = SORT_BT * SORT_ROUNDS; // keys one workgroup ranks at a time
constexpr uint32_t SORT_GATHER_SLACK = 16; // readable bytes behind a record slab: the gather reads whole eight-byte words

inline uint64_t sort_tiles(uint64_t n) { return (n + SORT_TILE - 1) / SORT_TILE; }
// entries of a pass's (digit, tile) table, digit-major, and one more for the scan's total
inline uint64_t sort_table_entries(uint64_t n) { return sort_tiles(n) * SORT_BINS + 1; }

// hist[d * 256 + b] = keys whose digit d is b (hist is zeroed here)
hipError_t launch_sort_histogram(const uint64_t *keys, uint64_t n, unsigned long long *hist, hipStream_t s);
// table[b * tiles + t] = keys of tile t whose digit `digit` is b, table[256 * tiles] = 0 (then scanned in place by the caller)
hipError_t launch_sort_count(const uint64_t *keys, uint64_t n, uint32_t digit, uint64_t *table, hipStream_t s);
// after the scan of table: (keys_in[i], idx_in[i]) goes to the slot its digit and its place among the keys of that digit give
// it, equal digits in input order.  idx_in == nullptr: the index of a pair is its position (the first pass that runs).
hipError_t launch_sort_scatter(const uint64_t *keys_in, const uint32_t *idx_in, uint64_t n, uint32_t digit, const uint64_t *table, uint64_t *keys_out,
                               uint32_t *idx_out, hipStream_t s);
// idx[i] = i (no pass ran: the input was in order already)
hipError_t launch_sort_iota(uint32_t *idx, uint64_t n, hipStream_t s);

// The records a chunk's write pass has left at base + off[i], i < n (off[n] = their bytes): record first + i gets its
// address, its length and its key (unplaced records last).
hipError_t launch_sort_keys(const uint8_t *base, const uint64_t *off, uint64_t n, uint64_t first, uint64_t *addr, uint32_t *len, uint64_t *key,
                            hipStream_t s);
// BAM input.  The records of a batch of the device ingest are consecutive in its view `raw`, record i at
// rec_off[i], i < n, n >= 1: host[0] (pinned, device address) = the view offset of the first one's first byte, host[1] = the
// offset behind the last one's last byte.
hipError_t launch_sort_span(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, unsigned long long *host, hipStream_t s);
// raw[begin, begin + bytes), that range, copied to dst, whose address has the residue modulo 16 of raw + begin (else
// hipErrorInvalidValue): aligned 16-byte words between up to 15 bytes at either end.  Record first + i gets what launch_sort_keys
// gives it: its address in dst, its length 4 + block_size and its key.
hipError_t launch_sort_keep(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, uint64_t begin, uint64_t bytes, uint8_t *dst, uint64_t first,
                            uint64_t *addr, uint32_t *len, uint64_t *key, hipStream_t s);
// slen[i] = len[perm[i]], slen[n] = 0 (then scanned in place by the caller into the sorted offsets)
hipError_t launch_sort_lengths(const uint32_t *len, const uint32_t *perm, uint64_t n, uint64_t *slen, hipStream_t s);
// after the scan: host[j] (pinned, device address), j <= pieces, = the first record with a byte at or behind byte
// (first_piece + j) * piece_bytes of the whole sorted stream (n: none); soff counts from `before` bytes into that stream
hipError_t launch_sort_bisect(const uint64_t *soff, uint64_t n, uint64_t piece_bytes, uint64_t first_piece, uint64_t before, uint64_t pieces,
                              unsigned long long *host, hipStream_t s);
// The bytes [lo, hi) of the sorted stream to out[0, hi - lo): records [a, b) of the sorted order, each clipped to the range.
// A wave per record; eight-byte stores behind an alignment prologue, the source read as whole words and shifted.
hipError_t launch_sort_gather(const uint64_t *addr, const uint32_t *perm, const uint64_t *soff, uint64_t a, uint64_t b, uint64_t lo, uint64_t hi,
                              uint8_t *out, hipStream_t s);

// Device bytes per resident record beside its own: address 8, length 4, key 8, the sort's second key array and its two index
// arrays 16, the sorted offset 8, and its share of the pass table (half a byte).
constexpr uint64_t SORT_BYTES_PER_RECORD = 48;

// ---- a BAM sorted in rounds (bamsort.cpp drives these)

// Device bytes per record of the survey: key 8, length 4, the sort's second key array 8 and its two index arrays 8, and its
// share of the pass table (256 entries of 8 bytes per tile of SORT_TILE keys), rounded up.  The sorted offsets take no array of
// their own: behind the sort they lie in the half of the key ping-pong that does not hold the sorted keys.
constexpr uint64_t SORT_SURVEY_BYTES_PER_RECORD = 8 + 4 + 8 + 4 + 4 + (SORT_BINS * 8 + SORT_TILE - 1) / SORT_TILE;
constexpr uint32_t SORT_SURVEY_MARK = 0x80000000u; // the top bit of a survey length (a record is shorter than 2^25 bytes): bai_kernel.hip sets it
// a place in the sorted order: rank order is the order of (key, input ordinal) pairs, the sort being stable
struct SortBound {
    uint64_t key, ord;
};
enum { SP_END = 0, SP_END_OFF, SP_KEY, SP_ORD, SP_FIRST_LEN, SP_WORDS };
// The records of a batch of the device ingest, record i at raw + rec_off[i]: the record of input ordinal first + i gets its
// length 4 + block_size and launch_sort_keys' key.  No record byte and no address is kept.
hipError_t launch_sort_survey(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, uint64_t first, uint32_t *len, uint64_t *key, hipStream_t s);
// launch_sort_lengths for survey lengths: slen drops SORT_SURVEY_MARK, *marked (device) = the smallest i whose length has it, ~0: none
hipError_t launch_sort_survey_lengths(const uint32_t *len, const uint32_t *perm, uint64_t n, uint64_t *slen, unsigned long long *marked, hipStream_t s);
// A round that begins at sorted rank start < n: host[SP_END] (pinned, device address) = the largest end whose records take
// soff[end] - soff[start] + per_record * (end - start) <= budget, [SP_END_OFF] = soff[end], [SP_KEY], [SP_ORD] = the sorted key
// and the input ordinal at rank end (~0 both: end == n), [SP_FIRST_LEN] = the length of the record at rank start.
hipError_t launch_sort_plan(const uint64_t *soff, const uint64_t *skey, const uint32_t *perm, uint64_t n, uint64_t start, uint64_t budget,
                            uint64_t per_record, unsigned long long *host, hipStream_t s);
// cnt[i] = 1 and bytes[i] = its length where lo <= (key, first + i) < hi for record i of the batch, else 0 both; cnt[n] = bytes[n] = 0
// (then scanned in place by the caller)
hipError_t launch_sort_round_flag(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, uint64_t first, SortBound lo, SortBound hi, uint64_t *cnt,
                                  uint64_t *bytes, hipStream_t s);
// after the two scans: every kept record whole to dst + off[i], compacted; record first + cnt[i] gets its address there, its
// length and its key.  A wave per record; nothing outside a record or its place is read or written.
hipError_t launch_sort_take(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, const uint64_t *cnt, const uint64_t *off, uint8_t *dst,
                            uint64_t first, uint64_t *addr, uint32_t *len, uint64_t *key, hipStream_t s);

// the device arrays of a sort, beside the caller's keys: the ping-pong's other half, the pass table, the histograms
struct SortScratch {
    DevArray<uint64_t> keys_b, table;
    DevArray<uint32_t> idx[2];
    DevArray<unsigned long long> hist;
    ScanScratch scan;
    uint32_t passes_run = 0, passes_skipped = 0;
};
// The sort of keys[0, n) (device; overwritten: they are one half of the ping-pong), n from 1 to 2^32 - 1: *perm, one of
// sc.idx, holds the input index of the i-th key in ascending order, equal keys in input order.  Waits for the stream once, for the histograms
// that say which passes run (sort.cpp).
hipError_t sort_pairs_u64(uint64_t *keys, uint64_t n, SortScratch &sc, hipStream_t s, const uint32_t **perm);

} // namespace ngsq
