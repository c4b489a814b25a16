// sam_kernels.h -- `ngs convert <BAM> <SAM>` on the device: the SAM text of every record of a batch of
// the device ingest.  Launchers only; sam_kernel.hip has the kernels, sam.cpp the driver, the copies and the writer thread.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "ingest_kernels.h"

namespace ngsq {

// the @SQ names on the device: the name of sequence r is names[name_off[r] .. name_off[r + 1])
struct SamRefs {
    const char *names;
    const uint64_t *name_off;
    uint32_t n_refs;
};

// Why a record has no SAM line.  The codes follow the fields' order on the line: a record with two
// faults reports the one further left.
enum SamError : uint32_t {
    SAM_OK = 0,
    SAM_E_REF,      // a reference sequence id outside [-1, n_refs)
    SAM_E_CIGAR_OP, // a CIGAR operation code above 8
    SAM_E_QUAL,     // a quality score above 93
    SAM_E_TAG_TYPE, // a tag value type outside AcCsSiIfZHB
    SAM_E_STR_NUL,  // a Z or H value without its NUL inside the record
    SAM_E_B_SUB,    // a B array subtype outside cCsSiIf
    SAM_E_OVERRUN,  // a tag (a B array's count included) that runs past the record's end
};
constexpr uint32_t SAM_ERR_BITS = 8; // bad word: record index in the file << SAM_ERR_BITS | SamError, ~0: none

// The records of a batch that hold an f32 value (an `f` tag or a B:f array): the full-occupancy kernels mark them and leave
// them to kernels with the float formatter.
struct SamFloats {
    uint8_t *mark;               // [n] 1: the record holds a float
    uint64_t *list;              // [n] the marked records, in no order
    unsigned long long *count;   // entries of list (zeroed by launch_sam_size)
};

// Sizing pass: len[i] = bytes of record i's line (newline included), len[n] = 0; the smallest (index << 8 | code) of a
// record that cannot be written goes to *bad (atomicMin); fl receives the records that hold a float.  One wave per record.
// keep (optional, device, [n]; `ngs view`): a record with keep[i] == 0 is dropped -- length 0, no
// error, no float mark, nothing written by the write pass.  nullptr: every record has its line.
hipError_t launch_sam_size(const ngsq_batch &b, const BatchOrigin &o, const SamRefs &refs, uint64_t *len, unsigned long long *bad,
                           const SamFloats &fl, hipStream_t s, const uint8_t *keep = nullptr);
// after the exclusive scan of len: host (pinned, device address) receives [off[n], *bad]
hipError_t launch_sam_total(const uint64_t *off, uint64_t n, const unsigned long long *bad, unsigned long long *host, hipStream_t s);
// Write pass: record i's line at text + off[i].  One wave per record; SEQ and QUAL a byte per lane.
hipError_t launch_sam_write(const ngsq_batch &b, const BatchOrigin &o, const SamRefs &refs, const uint64_t *off, char *text,
                            const SamFloats &fl, hipStream_t s, const uint8_t *keep = nullptr);

} // namespace ngsq
