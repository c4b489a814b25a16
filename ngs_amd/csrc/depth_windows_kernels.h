// depth_windows_kernels.h -- `ngs depth --by <N|BED>` on the device: the difference array of §23 into
// 64-bit prefix sums of the depth, tile by tile; the sums of windows or BED intervals as differences of two prefix values; the
// lines "<name>\t<start>\t<end>\t<mean>\n".  Launchers only; depth_windows_kernel.hip has the kernels, depth_windows.cpp the
// driver.  Every launcher returns hipErrorInvalidValue, and launches nothing, when a pointer it was given is null, a count its
// kernel needs is zero, or the grid is out of range.
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

} // namespace ngsq
