// derive_kernels.h -- `ngs derive instrument` on the device: the distinct instrument ids and flowcell
// ids of the read names of a batch of the device ingest, as two exact sets of byte strings.  Launchers only;
// derive_kernel.hip has the kernels, derive.cpp the driver and the predictor.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "ingest_kernels.h"

namespace ngsq {

// One slot of a set's open-addressing table.  key: 0 = empty, else the string's hash (never 0), claimed by atomicCAS.
// epoch: 0 until the claimant has filled the slot, then the number of the launch that did.  A launch trusts a slot whose
// epoch is neither 0 nor its own: it was filled before a kernel boundary, so plain loads of it and of its bytes are safe.
struct DeriveSlot {
    unsigned long long key;
    uint32_t off, len; // the string: arena[off, off + len)
    uint32_t epoch;
    uint32_t pad;
};

// One appended string.  Every string a lane could not find in the table is listed: the winner of a slot's claim and the
// candidates, which had no slot to claim or could not verify the one they met.  The host de-duplicates the list exactly.
struct DeriveEntry {
    uint32_t off, len;
    uint32_t set; // 0 instrument, 1 flowcell; | DERIVE_CANDIDATE
};
constexpr uint32_t DERIVE_CANDIDATE = 0x80000000u;

// device words of one scan (set by derive.cpp before the first batch: bad = ~0, the others 0)
struct DeriveState {
    unsigned long long bad;        // smallest file index of a record whose name has neither 5 nor 7 segments, ~0: none
    unsigned long long skipped;    // records whose name is "*"
    unsigned long long arena_used; // bytes asked of the arena (beyond arena_cap: overflow)
    unsigned long long n_entries;  // entries asked of the list (beyond entries_cap: overflow)
    unsigned long long overflow;   // 1: a string was dropped, the scan's result is void
};

struct DeriveSets {
    DeriveSlot *table[2]; // [slots] each
    uint32_t slots;       // a power of two
    uint8_t *arena;
    uint32_t arena_cap;
    DeriveEntry *entries;
    uint32_t entries_cap;
    DeriveState *state;
};

// what the host reads per batch (pinned, device address): [bad | overflow | length of the bad name | - | its bytes (256)]
constexpr uint32_t DERIVE_HOST_WORDS = 4 + 32;

// The names of the batch's records (record i of the batch is record base + i of the file) into the two sets; epoch: the
// launch's number, 1 for the first and never reused.  Behind it one wave copies the state's bad index and overflow word to
// `host` and, when the smallest bad index is a record of this batch, that record's name.
hipError_t launch_derive_names(const ngsq_batch &b, const BatchOrigin &o, uint64_t base, uint32_t epoch, const DeriveSets &sets,
                               unsigned long long *host, hipStream_t s);

} // namespace ngsq
