// collate_kernels.h -- `ngs fastq --collate` on the device: which records of an ingest batch are kept, the
// name keys of the resident records, the exact mate search inside the runs of equal keys, the three index lists in file order,
// and the size and write passes of a piece of a list.  Launchers only; collate_kernel.hip has the kernels, collate.cpp the
// driver.  The record formatter is fastq_format.h's, shared with `ngs fastq`.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "fastq_kernels.h"

namespace ngsq {

constexpr uint32_t COLLATE_OUTPUTS = 4;             // read ones, read twos, others, singletons
constexpr uint32_t COLLATE_NONE = 0xFFFFFFFFu;      // mate[i]: record i has no mate (at most 2^32 - 1 records are resident)
constexpr uint64_t COLLATE_KEY_OTHER = ~0ull;       // the key of an other: behind every hash (a hash has its top bit clear)
constexpr uint64_t COLLATE_MAX_RUN = 1024;          // NGSQ_COLLATE_MAX_RUN
// Device bytes per resident record beside its own: address 8, length 4, key 8, the sort's second key array and its two index
// arrays 16, its share of the pass table (half a byte), class 1, mate 4, the list scan 8, its list entry 4, rounded up.
constexpr uint64_t COLLATE_BYTES_PER_RECORD = 56;

// the device words of a run: the bad word (set to ~0 by the driver), the counts of the walk, the counts of the match
enum CollateWork : uint32_t { CW_BAD = 0, CW_EXCLUDED, CW_NO_SEQUENCE, CW_ONE, CW_TWO, CW_OTHER, CW_AMBIGUOUS, CW_COLLISIONS, CW_LONG_RUN, COLLATE_WORK_WORDS };

enum CollateKind : uint32_t { CK_LEAD = 0, CK_SINGLE, CK_OTHER }; // the three lists
// how the entries of a list become text
enum CollateMode : uint32_t {
    CM_SPLIT = 0,   // an entry leads a pair: its read one to text a, its read two to text b
    CM_INTERLEAVED, // an entry leads a pair: its read one, then its read two, to text a
    CM_RECORD       // an entry is a record: to text a
};

// Flag pass, a thread per record of the batch: cnt[i] = 1 and bytes[i] = 4 + block_size where record i is kept (the two flag
// tests and l_seq >= 1), else 0 both; cnt[n] = bytes[n] = 0 (then scanned in place by the caller); the batch's counts are added
// to work[CW_EXCLUDED .. CW_OTHER].
hipError_t launch_collate_flag(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, const FastqRules &r, uint64_t *cnt, uint64_t *bytes,
                               unsigned long long *work, hipStream_t s);
// after the scan of cnt, a wave per record of the batch: a kept record with a present score above 93 lowers work[CW_BAD]
// (atomicMin) to ((first_index + i) << FASTQ_ERR_BITS | FASTQ_E_QUAL)
hipError_t launch_collate_qual(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, const uint64_t *cnt, uint64_t first_index,
                               unsigned long long *work, hipStream_t s);
// Resident record i < n at addr[i]: cls[i] = its class; key[i] = the hash of its name's bytes, its top bit clear, and with
// hash_bits in 1 .. 63 only that many low bits, for a read one or two; COLLATE_KEY_OTHER for an other.
hipError_t launch_collate_key(const uint64_t *addr, uint64_t n, uint32_t hash_bits, uint64_t *key, uint8_t *cls, hipStream_t s);
// skey: the sorted keys.  work[CW_LONG_RUN] = 1 if skey[r] == skey[r + COLLATE_MAX_RUN] != COLLATE_KEY_OTHER for some rank r.
hipError_t launch_collate_run_limit(const uint64_t *skey, uint64_t n, unsigned long long *work, hipStream_t s);
// A thread per sorted rank: the record perm[r] walks the run of its key both ways and compares names, length then bytes.
// mate[i] = the other record of its name where the name has exactly one read one and one read two, else COLLATE_NONE (others
// too); work[CW_AMBIGUOUS] counts the ones and twos whose name has more than one one or more than one two, work[CW_COLLISIONS]
// those that met another name in their run.
hipError_t launch_collate_match(const uint64_t *skey, const uint32_t *perm, const uint64_t *addr, const uint8_t *cls, uint64_t n, uint32_t *mate,
                                unsigned long long *work, hipStream_t s);
// flag[i] = 1 where record i is of `kind` (CK_LEAD: mate[i] > i; CK_SINGLE: a one or two without mate; CK_OTHER), flag[n] = 0
hipError_t launch_collate_list_flag(const uint8_t *cls, const uint32_t *mate, uint64_t n, uint32_t kind, uint64_t *flag, hipStream_t s);
// after the scan: list[flag[i]] = i for every record of the kind (the same test)
hipError_t launch_collate_list_fill(const uint8_t *cls, const uint32_t *mate, uint64_t n, uint32_t kind, const uint64_t *flag, uint32_t *list,
                                    hipStream_t s);

// a piece of a list: entries list[0, m), as text of mode `mode`
struct CollatePiece {
    const uint32_t *list;
    uint64_t m;
    const uint64_t *addr;
    const uint8_t *cls;
    const uint32_t *mate;
    uint32_t mode;
};
// Size pass, a thread per entry: len_a[e] (and len_b[e] with CM_SPLIT) = the text bytes of entry e in text a (b);
// len_a[m] = len_b[m] = 0 (then scanned in place by the caller).  Closed-form from the records' fixed 32 bytes.
hipError_t launch_collate_size(const CollatePiece &p, const FastqRules &r, uint64_t *len_a, uint64_t *len_b, hipStream_t s);
// Write pass, a wave per record (two per entry of a pair): the four lines at text_a + off_a[e] or text_b + off_b[e]; with
// CM_INTERLEAVED the read two lies behind the read one.
hipError_t launch_collate_write(const CollatePiece &p, const FastqRules &r, const uint64_t *off_a, const uint64_t *off_b, char *text_a, char *text_b,
                                hipStream_t s);
// host (pinned, device address) receives the work words
hipError_t launch_collate_words(const unsigned long long *work, unsigned long long *host, hipStream_t s);

} // namespace ngsq
