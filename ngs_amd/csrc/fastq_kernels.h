// fastq_kernels.h -- `ngs fastq` on the device: the FASTQ text of every kept record of a batch of the
// device ingest, one device buffer per output.  Launchers only; fastq_kernel.hip has the kernels, fastq.cpp the driver, the
// encoders and the writer threads.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "ingest_kernels.h"

namespace ngsq {

constexpr uint32_t FASTQ_OUTPUTS = 3; // read ones, read twos, others (NGSQ_FASTQ_ONE / _TWO / _OTHER)

// the rules of a run (include/ngsq_fastq.h), as the kernels read them
struct FastqRules {
    uint32_t require, exclude;  // flag bits
    uint32_t default_quality;   // the score of a record without QUAL
    uint32_t name_suffix;       // 1: "/1" and "/2" behind the names of read ones and read twos
    uint32_t two_files;         // 0: every kept record goes to output 0
    uint32_t has_other;         // two-file mode: 1: others go to output 2, 0: they are dropped
};

// Why a kept record has no FASTQ text
enum FastqError : uint32_t { FASTQ_OK = 0, FASTQ_E_QUAL }; // a quality score above 93
constexpr uint32_t FASTQ_ERR_BITS = 8; // bad word: record index in the file << FASTQ_ERR_BITS | FastqError, ~0: none

// the device words of a run: the bad word (set to ~0 by the driver), then the counts, which add up over the batches
enum FastqWork : uint32_t { FW_BAD = 0, FW_EXCLUDED, FW_NO_SEQUENCE, FW_ONE, FW_TWO, FW_OTHER, FW_DROPPED, FASTQ_WORK_WORDS };
// what the host reads of a batch (pinned, device address): the three totals, then the work words
enum FastqHost : uint32_t { FH_BYTES = 0, FH_WORK = FASTQ_OUTPUTS, FASTQ_HOST_WORDS = FASTQ_OUTPUTS + FASTQ_WORK_WORDS };

// the three outputs' per-record arrays (sizes, then offsets after the scan), n + 1 entries each; null: an output the run has not
struct FastqOffsets {
    uint64_t *v[FASTQ_OUTPUTS];
};
struct FastqText {
    char *v[FASTQ_OUTPUTS];
};

// Size/classify pass, a thread per record: len.v[k][i] = bytes of record i's four lines if it is kept and goes to output k,
// else 0; len.v[k][n] = 0; the counts of the batch are added to work.  Reads flag, l_seq and l_read_name only.
hipError_t launch_fastq_size(const ngsq_batch &b, const BatchOrigin &o, const FastqRules &r, const FastqOffsets &len, unsigned long long *work,
                             hipStream_t s);
// after the exclusive scans of len: host receives [off.v[k][n] (0 for a null output) | the work words]
hipError_t launch_fastq_total(const FastqOffsets &off, uint64_t n, const unsigned long long *work, unsigned long long *host, hipStream_t s);
// Write pass, a wave per record: the four lines of kept record i at text.v[k] + off.v[k][i], k its output.  A lane takes a packed
// SEQ byte and two scores at a time.  A present score above 93 lowers work[FW_BAD] (atomicMin) to (index << 8 | FASTQ_E_QUAL).
// host (pinned, device address): receives work[FW_BAD] at host[FH_WORK + FW_BAD] behind the pass.
hipError_t launch_fastq_write(const ngsq_batch &b, const BatchOrigin &o, const FastqRules &r, const FastqOffsets &off, const FastqText &text,
                              unsigned long long *work, unsigned long long *host, hipStream_t s);

} // namespace ngsq
