// depth_kernels.h -- `ngs depth` on the device: records into a difference array, the array into runs of
// equal depth, the runs into bedGraph lines.  Launchers only; depth_kernel.hip has the kernels, depth.cpp the driver.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/ngsq.h"

namespace ngsq {

constexpr uint32_t DEPTH_BT = 256;                           // threads of a block
constexpr uint32_t DEPTH_ITEMS = 4;                          // positions of a thread: one 16-byte load
constexpr uint32_t DEPTH_GRANULE = DEPTH_BT * DEPTH_ITEMS;   // positions of a block: tiles are multiples of it
constexpr uint64_t DEPTH_TILE_DEFAULT = (uint64_t)1 << 22;   // positions of a tile (16 MiB of differences)
constexpr uint64_t DEPTH_TILE_MAX = (uint64_t)1 << 31;       // (no sequence is longer)
constexpr uint32_t DEPTH_STAGE_BYTES = 16384;                // LDS a block of the write pass stages its lines in

// What one record passes on to the next one's order check, across batches.
struct DepthCarry {
    int32_t ref, pos;
    uint32_t placed; // ref >= 0 and pos >= 0
    uint32_t has;    // a record has been seen on this walk
};

// device words of one call (depth.cpp sets them up: zero, with bad_order, lo_ref and hi_ref at their empty values)
struct DepthState {
    DepthCarry carry[2];          // batch k reads carry[k & 1] and writes carry[(k + 1) & 1]
    unsigned long long bad_order; // smallest index of a record that breaks the coordinate order, ~0: none
    unsigned long long counted;   // records that count
    int32_t lo_ref, hi_ref;       // the batch's smallest and largest sequence id of a placed record (INT32_MAX, -1: none)
    // the run path, from tile to tile of one sequence or region
    int32_t depth;                // the depth behind the last tile's last position
    uint32_t open;                // 1: a run is held back, its end lies in a later tile
    uint32_t open_start;
    int32_t open_depth;
    uint32_t n_runs;              // runs of the tile at hand, the one held back included
    uint32_t lines;               // lines of the tile at hand
};

// the words the host reads (pinned, device address): after launch_depth_order [bad_order, lo_ref, hi_ref], after
// launch_depth_total [text bytes, lines]
constexpr uint32_t DEPTH_HOST_WORDS = 4;

// Order check of a batch against the record in front of each record (the carry for the first), the batch's first and last
// sequence, and the three words to the host.  The batch's lo_ref / hi_ref start from their empty values.
hipError_t launch_depth_order(const ngsq_batch &b, DepthState *state, uint32_t parity, unsigned long long *host, hipStream_t s);

// the window of one sequence the difference array stands for: positions [lo, lo + len) of sequence ref, diff[len + 1]
struct DepthWindow {
    int32_t ref;
    uint32_t lo, len;
    int32_t *diff;
};
// Every record of the batch that counts (sequence w.ref, pos >= 0, no excluded flag, mapq >= min_mapq, keep[i] != 0 when keep is
// given) adds 1 to state->counted and, clipped to the window, +1 at its first position and -1 behind its last.
hipError_t launch_depth_add(const ngsq_batch &b, const uint8_t *keep, const DepthWindow &w, uint32_t exclude_flags, uint32_t min_mapq,
                            DepthState *state, hipStream_t s);

// Every record of the batch that passes k_depth_add's test for sequence `ref` (pos >= 0, no excluded flag, mapq >= min_mapq,
// keep[i] != 0 when keep is given) adds 1 to state->counted: a sequence that has no difference array (`ngs depth --by`: no
// interval, length 0).  hipErrorInvalidValue, and no launch, for a null pointer or an empty batch.
hipError_t launch_depth_count(const ngsq_batch &b, const uint8_t *keep, int32_t ref, uint32_t exclude_flags, uint32_t min_mapq, DepthState *state,
                              hipStream_t s);

// the arrays of the run path, sized for the largest tile: bsum / bcnt [tile / DEPTH_GRANULE], rstart / rdepth [tile + 1], off [tile + 2]
struct DepthTileArrays {
    int32_t *bsum;
    uint32_t *bcnt;
    uint32_t *rstart;
    int32_t *rdepth;
    uint64_t *off;
};
// One tile: positions [t0, t0 + n) of the window, n <= the tile size, t0 a multiple of DEPTH_GRANULE.  A position starts a run
// when its difference is not 0, and the window's first position always does.  launch_depth_runs leaves the tile's run starts
// (as coordinates of the sequence) and depths behind the run held back from the tile in front, state->n_runs their number.
hipError_t launch_depth_runs(const DepthWindow &w, uint64_t t0, uint32_t n, const DepthTileArrays &a, DepthState *state, hipStream_t s);
// The byte size of every line of the tile into a.off[0, entries), 0 behind the lines; entries: more than the tile can have lines
// (at most its n positions + 2).  A run's end is the next run's start; the tile's last run is held back unless the tile is the
// window's last (final), where it ends at w.lo + w.len.
hipError_t launch_depth_size(uint64_t entries, bool final, uint32_t final_end, uint32_t name_len, const DepthTileArrays &a, DepthState *state, hipStream_t s);
// behind the exclusive scan of a.off: the two words to the host, and the run held back (or none) into the state
hipError_t launch_depth_total(bool final, const DepthTileArrays &a, DepthState *state, unsigned long long *host, hipStream_t s);
// the tile's lines into text (the host has read `lines`); name: the sequence's name on the device
hipError_t launch_depth_write(char *text, uint32_t lines, bool final, uint32_t final_end, const char *name, uint32_t name_len, const DepthTileArrays &a,
                              hipStream_t s);
// "name\tstart\tend\t0\n" into text: a sequence or region no record was seen of
hipError_t launch_depth_zero_line(char *text, const char *name, uint32_t name_len, uint32_t start, uint32_t end, hipStream_t s);

// decimal digits of v
inline uint32_t depth_digits(uint32_t v) {
    uint32_t n = 1;
    while (v >= 10) v /= 10, n++;
    return n;
}

} // namespace ngsq
