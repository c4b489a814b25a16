// bai_kernels.h -- `ngs index` on the device: the BAI of a coordinate-sorted BAM built from the
// batches of the device ingest.  Launchers only; bai_kernel.hip has the kernels, bai.cpp the driver and the file writer.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "ingest_kernels.h"

namespace ngsq {

// What one record passes on to the next one, across blocks and batches.
struct BaiCarry {
    int32_t ref, pos;
    uint32_t bin, w1;    // bin; last 16 kb window it overlaps
    uint32_t placed;     // ref >= 0 and pos >= 0
    uint32_t has;        // a record has been seen
    uint64_t endv;       // virtual position behind the record (for the first record: behind the header)
};

// one run of records of the same (sequence, bin), in file order: exactly one chunk
struct BaiRun {
    uint64_t start; // chunk start: the position behind the record in front of its first record
    uint64_t rec;   // index of its first record in the file
    int32_t ref;    // -1: the unplaced records at the end of the file
    uint32_t bin;
};

// device words of one index build (zeroed / set by bai.cpp before the first batch)
struct BaiState {
    BaiCarry carry[2];          // batch k reads carry[k & 1] and writes carry[(k + 1) & 1]
    unsigned long long bad_order; // smallest index of a record that breaks the coordinate order, ~0: none
    unsigned long long bad_limit; // smallest index of a record the BAI cannot hold (sequence id, or beyond the windows kept), ~0: none
};

// per-sequence linear index: windows [lin_base[r], lin_base[r] + lin_cap[r]) of `lin`, ~0 = no record overlaps the window
struct BaiLinear {
    unsigned long long *lin;
    const uint64_t *lin_base;
    const uint32_t *lin_cap;
    unsigned long long *unmapped; // [n_refs] placed records with flag 0x4
    uint32_t n_refs;
};

// One pass over a batch: reference span, bin and the order check of every record, the linear windows it is the first to
// overlap, its unmapped flag; run_flag[i] = 1 where a run starts (and run_flag[n] = 0), tmp_runs[i] its entry.
hipError_t launch_bai_records(const ngsq_batch &b, const BatchOrigin &o, BaiState *state, uint32_t parity, const BaiLinear &lin,
                              uint64_t *run_flag, BaiRun *tmp_runs, hipStream_t s);
// after the exclusive scan of run_flag: the batch's runs behind the `base` runs already listed; host_count (pinned, device
// address) receives base + the batch's runs
hipError_t launch_bai_gather(const uint64_t *run_off, const BaiRun *tmp_runs, uint64_t n, BaiRun *runs, uint64_t base,
                             unsigned long long *host_count, hipStream_t s);
// End of the file: every sequence's empty windows take the value in front of them (0 before its first record);
// n_intv[r] = last window a record overlaps + 1.  host (pinned, device address): [state words | unmapped[n_refs] | n_intv[n_refs]]
// with the state words = bad_order, bad_limit, the final carry's endv.
hipError_t launch_bai_finish(const BaiLinear &lin, const BaiState *state, uint32_t parity, unsigned long long *host, hipStream_t s);
constexpr uint32_t BAI_HOST_STATE_WORDS = 4;

// ---- the index of a sorted BAM while it is written (sort_resident.h drives these)

// A tile of the sorted order of resident records: record first + i, i < n, is the one at addr[perm[first + i]] (a whole BAM
// record, block_size first, at any byte alignment) and begins at byte soff[first + i] of the sorted stream (soff[records] = its end).
struct BaiSorted {
    const uint64_t *addr;
    const uint32_t *perm;
    const uint64_t *soff;
    uint64_t first, n;
    uint64_t rec0, pos0; // what lies in front of soff[0]: records and bytes of the sorted stream (a file sorted in rounds; else 0)
};
// launch_bai_records for such a tile.  The positions it leaves (run starts, windows, the carry's endv) are stream offsets plus
// one, so that k_bai_finish's 0 keeps meaning "no record in front"; BaiRun::rec is the index in the sorted order.
hipError_t launch_bai_sorted(const BaiSorted &t, BaiState *state, uint32_t parity, const BaiLinear &lin, uint64_t *run_flag, BaiRun *tmp_runs,
                             hipStream_t s);
// A batch of the device ingest, record i at raw + rec_off[i], before anything is resident (a BAM sorted in rounds, DESIGN.md
// section 22.3): len[first + i] gets `mark` where launch_bai_sorted would refuse the record as one the BAI cannot hold.
hipError_t launch_bai_survey(const uint8_t *raw, const uint64_t *rec_off, uint64_t n, uint64_t first, const BaiLinear &lin, uint32_t mark,
                             uint32_t *len, hipStream_t s);
// The file's BGZF blocks that hold records: piece j of piece_bytes stream bytes is blocks [j * blocks_per_piece, ...) of coff,
// DEFLATE_BLOCK_INPUT stream bytes each, coff their file offsets; the stream has `total` bytes and the EOF block lies at eof_coff.
struct BaiBlocks {
    const uint64_t *coff;
    uint64_t piece_bytes, blocks_per_piece, total, eof_coff;
};
// table[i] = base + off[i], i < n_blocks: the encoder's member offsets of a job whose first block lies at file offset base
hipError_t launch_bai_blocks(const uint64_t *off, uint64_t n_blocks, uint64_t base, uint64_t *table, hipStream_t s);
// every run's start and every window (after launch_bai_finish) from a stream offset plus one to a virtual position; 0 stays 0
hipError_t launch_bai_translate(const BaiBlocks &b, BaiRun *runs, uint64_t n_runs, unsigned long long *lin, uint64_t n_win, hipStream_t s);

} // namespace ngsq
