// markdup_kernels.h -- `ngs markdup` on the device: the class, the packed unclipped 5' end and the score
// of every resident record, the name keys of the pair candidates (the mate search itself is collate_kernels.h's), the entry
// lists, the keys and values of the pairs and of the fragments, the runs of equal keys and their survivors, and the flag byte.
// Launchers only; markdup_kernel.hip has the kernels, markdup.cpp the driver.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "collate_kernels.h"

namespace ngsq {

constexpr uint64_t MARKDUP_NO_END = ~0ull;  // end[i] of a record that is no candidate (a packed end has ref < 2^31 in front)
constexpr int64_t MARKDUP_END_BIAS = (int64_t)1 << 30; // u + 2^30 lies in [0, 2^31)
// Device bytes per resident record beside its own: address 8, length 4, key 8, the sort's second key array and its two index
// arrays 16, its share of the pass table (half a byte), the stream offset 8 (the run flags before it), class 1, duplicate 1,
// end 8, score 4, mate 4, its list entry 4, and of the entries: the high word 4 (a pair has two records), the low word 8, the
// value 8, the first permutation and the composed one 2 each, the run's best 8; rounded up.
constexpr uint64_t MARKDUP_BYTES_PER_RECORD = 104;

// the device words of a run: collate's (the bad word, set to ~0 by the driver, and the match's three), then this command's
enum MarkdupWork : uint32_t { MW_CANDIDATES = COLLATE_WORK_WORDS, MW_CLEARED, MW_DUP_PAIRS, MW_DUP_FRAGMENTS, MARKDUP_WORK_WORDS };

enum MarkdupKind : uint32_t {
    MK_LEAD = 0,  // a pair's earlier record: mate[i] > i
    MK_CANDIDATE, // every candidate: end[i] != MARKDUP_NO_END
    MK_SURVIVOR   // every record that is no duplicate: dup[i] == 0
};

// A wave per resident record i < n at addr[i].  cls[i] = CLASS_ONE / CLASS_TWO for a pair candidate, CLASS_OTHER for every
// other record; end[i] = the packed end of a candidate, MARKDUP_NO_END otherwise; score[i] = the sum of the QUAL bytes >= 15
// modulo 2^32 (0 with QUAL missing).  A candidate whose u lies outside [-2^30, 2^31 - 2^30) lowers work[CW_BAD] (atomicMin) to i.
hipError_t launch_markdup_ends(const uint64_t *addr, uint64_t n, uint8_t *cls, uint64_t *end, uint32_t *score, unsigned long long *work, hipStream_t s);
// A thread per record: key[i] = launch_collate_key's hash for a pair candidate, COLLATE_KEY_OTHER otherwise; the candidates and
// the records that came in with 0x400 are added to work[MW_CANDIDATES] and work[MW_CLEARED].
hipError_t launch_markdup_key(const uint64_t *addr, const uint8_t *cls, const uint64_t *end, uint64_t n, uint32_t hash_bits, uint64_t *key,
                              unsigned long long *work, hipStream_t s);
// flag[i] = 1 where record i is of `kind`, flag[n] = 0; after the scan: list[flag[i]] = i for every record of the kind
hipError_t launch_markdup_list_flag(const uint64_t *end, const uint32_t *mate, const uint8_t *dup, uint64_t n, uint32_t kind, uint64_t *flag, hipStream_t s);
hipError_t launch_markdup_list_fill(const uint64_t *end, const uint32_t *mate, const uint8_t *dup, uint64_t n, uint32_t kind, const uint64_t *flag,
                                    uint32_t *list, hipStream_t s);
// Entry e < m of the pair list, i = list[e], j = mate[i]: hi[e], lo[e] = the larger and the smaller of the two ends,
// val[e] = (score[i] + score[j]) mod 2^32 << 32 | ~(i + 1).
// hi == nullptr: entry e of the candidate list: lo[e] = end[i], val[e] = ~0 for a pair member, else score[i] << 32 | ~(i + 1).
hipError_t launch_markdup_entry_keys(const uint32_t *list, uint64_t m, const uint32_t *mate, const uint64_t *end, const uint32_t *score, uint64_t *hi,
                                     uint64_t *lo, uint64_t *val, hipStream_t s);
// dst[q] = src[perm[q]], q < m
hipError_t launch_markdup_gather(const uint64_t *src, const uint32_t *perm, uint64_t m, uint64_t *dst, hipStream_t s);
// out[r] = first[second[r]], r < m
hipError_t launch_markdup_compose(const uint32_t *first, const uint32_t *second, uint64_t m, uint32_t *out, hipStream_t s);
// order[r]: the entry at rank r.  flag[r] = 1 where r == 0 or a key word of entry order[r] differs from that of order[r - 1]
// (hi may be null), flag[m] = 0 (then scanned in place by the caller: the run of rank r is flag[r + 1] - 1).
hipError_t launch_markdup_heads(const uint32_t *order, const uint64_t *hi, const uint64_t *lo, uint64_t m, uint64_t *flag, hipStream_t s);
// best[run of r] = max(val[order[r]]) (atomicMax; best is zeroed by the caller)
hipError_t launch_markdup_best(const uint32_t *order, const uint64_t *run, const uint64_t *val, uint64_t m, unsigned long long *best, hipStream_t s);
// Entry order[r] whose value is not its run's best.  pairs: dup[i] = dup[mate[i]] = 1 and work[MW_DUP_PAIRS] counts it; else, if
// record i is no pair member, dup[i] = 1 and work[MW_DUP_FRAGMENTS] counts it.
hipError_t launch_markdup_mark(const uint32_t *order, const uint64_t *run, const uint64_t *val, const unsigned long long *best, const uint32_t *list,
                               const uint32_t *mate, uint64_t m, bool pairs, uint8_t *dup, unsigned long long *work, hipStream_t s);
// byte 19 of record i (the high byte of its flag): bit 0x400 cleared, then set where dup[i]; one byte store per record
hipError_t launch_markdup_apply(const uint64_t *addr, const uint8_t *dup, uint64_t n, hipStream_t s);
// host (pinned, device address) receives the work words
hipError_t launch_markdup_words(const unsigned long long *work, unsigned long long *host, hipStream_t s);

} // namespace ngsq
