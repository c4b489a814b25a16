// depth_windows_kernels.h -- `ngs depth --by <N|BED>` on the device: the difference array of §23 into
// 64-bit prefix sums of the depth, tile by tile; the sums of windows or BED intervals as differences of two prefix values; the
// lines "<name>\t<start>\t<end>\t<mean>\n".  Launchers only; depth_windows_kernel.hip has the kernels, depth_windows.cpp the
// driver.  Every launcher returns hipErrorInvalidValue, and launches nothing, when a pointer it was given is null, a count its
// kernel needs is zero, or the grid is out of range.  Behind them the thresholds variant (section 25): beside P, the count of
// positions at or above each of K depths, looked up the same way, and K more columns a line.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/ngsq_depth.h"
#include "depth_kernels.h"

namespace ngsq {

// device words of one call beside DepthState: the reduce pass's carry from tile to tile of one window (the driver zeroes the
// first three at the window's start), and the sum of all line sums
struct DepthWState {
    int32_t depth;                // the depth behind the last tile's last position
    uint32_t pad;
    unsigned long long P;         // the sum of the depths of the window's positions in front of the next tile
    unsigned long long bound;     // P at the last window boundary in front of the next tile (at the window's start: 0)
    unsigned long long depth_sum; // sum of the sums of all lines sized so far, modulo 2^64
};
constexpr size_t DEPTHW_CARRY_BYTES = 24; // depth, pad, P, bound

// the words the host reads after launch_depthw_total (pinned, device address): [the pass's text bytes, depth_sum so far]
constexpr uint32_t DEPTHW_HOST_WORDS = 2;

// the arrays of the reduce pass, sized for the largest tile: bdepth / bsum / bP [tile / DEPTH_GRANULE], P [tile + 1]
struct DepthWTileArrays {
    int32_t *bdepth;   // a block's sum of differences, then the depth entering it
    long long *bsum;   // a block's sum of depths for an entering depth of 0
    uint64_t *bP;      // P entering a block
    uint64_t *P;       // P[j]: the sum of the depths of the window's positions in front of position t0 + j, j = 0 .. n
};
// One tile: positions [t0, t0 + n) of the window (t0 a multiple of DEPTH_GRANULE, n <= the tile size): a.P[0 .. n] from the
// carry in ws, which moves on to the tile's end.
hipError_t launch_depthw_prefix(const DepthWindow &w, uint64_t t0, uint32_t n, const DepthWTileArrays &a, DepthWState *ws, hipStream_t s);

// --by N: the `count` windows whose end lies in the tile (origin: the coordinate of the tile's first position, n its positions).
// Window kb + j is [(kb + j) N, (kb + j + 1) N) clipped to hi; sum[j] = P(its end) - P(the boundary in front), which for j = 0 is
// ws->bound; ws->bound becomes P at the last window's end.
hipError_t launch_depthw_window_sums(const uint64_t *P, uint64_t origin, uint32_t n, uint32_t window, uint64_t kb, uint32_t count, uint32_t hi,
                                     uint64_t *sum, DepthWState *ws, hipStream_t s);

// --by BED: the `count` intervals of the sequence at hand against the tile [t0, t0 + n) of its positions: acc[i] += P[end - t0]
// for an end in (t0, t0 + n], acc[i] -= P[start - t0] for a start in [t0, t0 + n), wrapping.
hipError_t launch_depthw_interval_acc(const ngsq_depth_interval *iv, uint64_t count, const uint64_t *P, uint64_t t0, uint32_t n, uint64_t *acc,
                                      hipStream_t s);

// Where the lines of a format pass come from: `count` lines of one sequence.
struct DepthLineSource {
    uint64_t count;
    uint32_t zero;                  // 1: every sum is 0 (sum is not looked at)
    uint32_t window;                // >= 1: line k is window kb + k, [(kb + k) window, (kb + k + 1) window) clipped to [lo, hi)
    uint64_t kb;
    uint32_t lo, hi;
    const ngsq_depth_interval *iv;  // window == 0: line k is iv[k]
    const uint64_t *sum;            // sum[k]
};
// Lines [k0, k0 + m) of the source: the byte size of each into off[0, m), off[m] = 0; their sums are added to ws->depth_sum.
hipError_t launch_depthw_size(const DepthLineSource &src, uint64_t k0, uint32_t m, uint32_t name_len, uint64_t *off, DepthWState *ws, hipStream_t s);
// behind the exclusive scan of off[0, m]: the two words to the host
hipError_t launch_depthw_total(const uint64_t *off, uint32_t m, const DepthWState *ws, unsigned long long *host, hipStream_t s);
// the lines into text, off[m] bytes; name: the sequence's name on the device
hipError_t launch_depthw_write(char *text, const DepthLineSource &src, uint64_t k0, uint32_t m, const char *name, uint32_t name_len, const uint64_t *off,
                               hipStream_t s);

// ---- `ngs depth --by ... --thresholds` -----------------------------------------------------------------
// C_k(x): the number of the window's positions in front of x whose depth is at least T_k.  The count of an interval is
// C_k(e) - C_k(s), as its sum is P(e) - P(s).  A count is below 2^31 (no window is longer), so 32 bits hold it; partial sums wrap.

// K in 1 .. NGSQ_DEPTH_MAX_THRESHOLDS depths, strictly ascending, each in 1 .. 2^31 - 1
struct DepthThresholds {
    uint32_t k;
    uint32_t t[NGSQ_DEPTH_MAX_THRESHOLDS];
};

// device words of a thresholds call beside DepthWState: per threshold the reduce pass's carry from tile to tile of one window (the
// driver zeroes DEPTHT_CARRY_BYTES at the window's start), and the sum of the counts of all lines sized so far
struct DepthTState {
    uint32_t C[NGSQ_DEPTH_MAX_THRESHOLDS];      // C_k behind the last tile's last position
    uint32_t boundC[NGSQ_DEPTH_MAX_THRESHOLDS]; // C_k at the last window boundary in front of the next tile (the twin of bound)
    unsigned long long covered[NGSQ_DEPTH_MAX_THRESHOLDS];
};
constexpr size_t DEPTHT_CARRY_BYTES = 2 * NGSQ_DEPTH_MAX_THRESHOLDS * sizeof(uint32_t); // C, boundC

// the words the host reads after launch_deptht_total: the two of launch_depthw_total, then covered[0 .. K)
constexpr uint32_t DEPTHT_HOST_WORDS = DEPTHW_HOST_WORDS + NGSQ_DEPTH_MAX_THRESHOLDS;

// The count arrays of the reduce pass, K rows each.  Position j of the tile lies in block j / DEPTH_GRANULE.  cin[k][j] is the
// number of positions of j's block up to and including j that reach T_k: at most DEPTH_GRANULE = 1024, 16 bits.  C_k in front
// of tile position x is
//     x == 0:  bC[k][0]                                                 (what the tiles in front carried here)
//     x >= 1:  bC[k][(x - 1) / DEPTH_GRANULE] + cin[k][x - 1]
// for x = 0 .. n.  The block looked at is that of position x - 1, which exists for every x in 1 .. n: a lookup at the tile's end
// or exactly on a block boundary reads the last entry of the block in front, never a block the tile does not have.
struct DepthTTileArrays {
    uint16_t *cin;     // [K][stride]; stride a multiple of DEPTH_GRANULE, at least the tile's positions rounded up to it
    uint32_t *bcnt;    // [K][bstride]: a block's positions that reach T_k
    uint32_t *bC;      // [K][bstride]: C_k entering a block
    uint64_t stride;
    uint32_t bstride;  // at least the tile's blocks
};
// launch_depthw_prefix and, in the same pass over the tile, t.cin and t.bcnt; then t.bC from the carry in ts, which moves on.
hipError_t launch_deptht_prefix(const DepthWindow &w, uint64_t t0, uint32_t n, const DepthWTileArrays &a, const DepthTTileArrays &t,
                                const DepthThresholds &thr, DepthWState *ws, DepthTState *ts, hipStream_t s);

// --by N, beside launch_depthw_window_sums (same windows, same arguments): cnt[k * cstride + j] = C_k(end of window kb + j) -
// C_k(the boundary in front), which for j = 0 is ts->boundC[k]; ts->boundC[k] becomes C_k at the last window's end.
hipError_t launch_deptht_window_counts(const DepthTTileArrays &t, uint32_t K, uint64_t origin, uint32_t n, uint32_t window, uint64_t kb, uint32_t count,
                                       uint32_t hi, uint32_t *cnt, uint64_t cstride, DepthTState *ts, hipStream_t s);

// --by BED, beside launch_depthw_interval_acc: acc[k * cstride + i] += C_k(end - t0) for an end in (t0, t0 + n], -= C_k(start - t0)
// for a start in [t0, t0 + n), wrapping.
hipError_t launch_deptht_interval_acc(const ngsq_depth_interval *iv, uint64_t count, const DepthTTileArrays &t, uint32_t K, uint64_t t0, uint32_t n,
                                      uint32_t *acc, uint64_t cstride, hipStream_t s);

// A line source with K counts a line: line k's count for threshold j is cnt[j * cstride + k]; base.zero: K zeros (cnt is not looked at).
struct DepthTLineSource {
    DepthLineSource base;
    uint32_t K;
    const uint32_t *cnt;
    uint64_t cstride;
};
// launch_depthw_size / _total / _write with the K columns "\t<n_k>" behind the mean; the lines' counts are added to ts->covered,
// and launch_deptht_total hands the host DEPTHW_HOST_WORDS + K words.
hipError_t launch_deptht_size(const DepthTLineSource &src, uint64_t k0, uint32_t m, uint32_t name_len, uint64_t *off, DepthWState *ws, DepthTState *ts,
                              hipStream_t s);
hipError_t launch_deptht_total(const uint64_t *off, uint32_t m, uint32_t K, const DepthWState *ws, const DepthTState *ts, unsigned long long *host,
                               hipStream_t s);
hipError_t launch_deptht_write(char *text, const DepthTLineSource &src, uint64_t k0, uint32_t m, const char *name, uint32_t name_len, const uint64_t *off,
                               hipStream_t s);

} // namespace ngsq
