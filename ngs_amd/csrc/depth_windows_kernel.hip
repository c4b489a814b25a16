// depth_windows_kernel.hip -- `ngs depth --by <N|BED>` on the device.
//   k_depthw_sums          a tile of the difference array, DEPTH_GRANULE positions per block: the block's sum of differences
//                          and its sum of depths as if the depth entering it were 0
//   k_depthw_offsets       one block: the depth and P entering every block, from the carry of the tile in front
//   k_depthw_prefix        the tile again: P[j], the sum of the depths of the window's positions in front of j, for j = 0 .. n
//   k_depthw_window_sums   one thread per window that ends in the tile: P(end) - P(the boundary in front)
//   k_depthw_interval_acc  one thread per BED interval of the sequence: its end's P added, its start's P taken off
//   k_depthw_size          one thread per line: its bytes; the lines' sums into depth_sum, one atomic a wave
//   k_depthw_write         one thread per line: the text, staged per block in LDS and stored as aligned words
// A range of positions is summed up as (sum of differences, sum of depths for an entering depth of 0, positions); two ranges
// join without looking at the positions again, so blocks meet only at kernel boundaries.  All arithmetic is in integers, the
// sums 64 bits wide and wrapping.  All stores are vector stores of plain C++.
// Behind them the kernels of --thresholds, which a call without thresholds never launches:
//   k_deptht_prefix        k_depthw_prefix and, from the same read, per threshold the block-relative counts and the block's total
//   k_deptht_offsets       one block: C_k entering every block, from the carry of the tile in front
//   k_deptht_window_counts, k_deptht_bound, k_deptht_interval_acc     the twins of the three sum kernels: K lookups where they take one
//   k_deptht_size, k_deptht_total, k_deptht_write                     the format pass with K more columns a line
#include <hip/hip_runtime.h>

#include <algorithm>

#include "depth_windows_kernels.h"

namespace ngsq {

namespace {

constexpr uint32_t BT = DEPTH_BT;

// a range of positions: the sum of its differences, the sum of its depths for an entering depth of 0, its positions
struct Agg {
    int32_t d;
    long long s;
    uint32_t n;
};
__device__ inline Agg join(const Agg &l, const Agg &r) { return Agg{l.d + r.d, l.s + r.s + (long long)r.n * l.d, l.n + r.n}; }

// What the block's threads in front of this one add up to, and the whole block.  Two barriers; may be called again.
__device__ inline Agg block_exclusive(const Agg own, Agg *total) {
    __shared__ int32_t wd[BT / 64];
    __shared__ long long ws[BT / 64];
    __shared__ uint32_t wn[BT / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    Agg in = own;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const Agg l{__shfl_up(in.d, d), __shfl_up(in.s, d), __shfl_up(in.n, d)};
        if (lane >= d) in = join(l, in);
    }
    if (lane == 63) wd[wave] = in.d, ws[wave] = in.s, wn[wave] = in.n;
    Agg ex{__shfl_up(in.d, 1), __shfl_up(in.s, 1), __shfl_up(in.n, 1)};
    if (lane == 0) ex = Agg{0, 0, 0};
    __syncthreads();
    Agg before{0, 0, 0}, all{0, 0, 0};
    for (uint32_t k = 0; k < BT / 64; k++) {
        const Agg w{wd[k], ws[k], wn[k]};
        if (k < wave) before = join(before, w);
        all = join(all, w);
    }
    *total = all;
    __syncthreads();
    return join(before, ex);
}

// a thread's four differences of the tile (0 beyond its n positions), how many of them are positions, and what they add up to
struct Items {
    int32_t v[DEPTH_ITEMS];
    Agg agg;
};
__device__ inline Items load_items(const int32_t *__restrict__ diff, uint64_t t0, uint32_t n, uint32_t p) {
    Items it;
    int4 q = make_int4(0, 0, 0, 0);
    if (p < n) q = *reinterpret_cast<const int4 *>(diff + t0 + p); // (16-byte aligned: t0 and p are multiples of 4; the array is padded to the granule)
    it.v[0] = q.x, it.v[1] = q.y, it.v[2] = q.z, it.v[3] = q.w;
    it.agg = Agg{0, 0, 0};
    for (uint32_t j = 0; j < DEPTH_ITEMS; j++) {
        if (p + j >= n) it.v[j] = 0;
        else {
            it.agg.d += it.v[j];
            it.agg.s += it.agg.d;
            it.agg.n++;
        }
    }
    return it;
}

__global__ __launch_bounds__(BT) void k_depthw_sums(const int32_t *__restrict__ diff, uint64_t t0, uint32_t n, int32_t *__restrict__ bdepth,
                                                    long long *__restrict__ bsum) {
    const Items it = load_items(diff, t0, n, blockIdx.x * DEPTH_GRANULE + threadIdx.x * DEPTH_ITEMS);
    Agg total;
    (void)block_exclusive(it.agg, &total);
    if (threadIdx.x == 0) bdepth[blockIdx.x] = total.d, bsum[blockIdx.x] = total.s;
}

__global__ __launch_bounds__(BT) void k_depthw_offsets(uint32_t n_blocks, uint32_t n, int32_t *__restrict__ bdepth, const long long *__restrict__ bsum,
                                                       uint64_t *__restrict__ bP, DepthWState *ws) {
    const int32_t depth0 = ws->depth;
    const uint64_t P0 = ws->P;
    Agg run{0, 0, 0};
    for (uint32_t base = 0; base < n_blocks; base += BT) {
        const uint32_t i = base + threadIdx.x;
        Agg own{0, 0, 0}, total;
        if (i < n_blocks) own = Agg{bdepth[i], bsum[i], min(DEPTH_GRANULE, n - i * DEPTH_GRANULE)}; // (the last block is partial)
        const Agg e = join(run, block_exclusive(own, &total));
        if (i < n_blocks) {
            bdepth[i] = depth0 + e.d;
            bP[i] = P0 + (uint64_t)e.s + (uint64_t)((long long)e.n * depth0);
        }
        run = join(run, total);
    }
    __syncthreads(); // (every thread has read the carry)
    if (threadIdx.x == 0) {
        ws->depth = depth0 + run.d;
        ws->P = P0 + (uint64_t)run.s + (uint64_t)((long long)run.n * depth0);
    }
}

// a thread's P[p .. p + 4] into the tile's P[0 .. n], p < n
__device__ inline void store_prefix(uint64_t *__restrict__ P, uint32_t p, uint32_t n, const uint64_t *out) {
    if (p + DEPTH_ITEMS <= n) { // (32-byte aligned: p is a multiple of 4)
        *reinterpret_cast<ulonglong2 *>(P + p) = make_ulonglong2(out[0], out[1]);
        *reinterpret_cast<ulonglong2 *>(P + p + 2) = make_ulonglong2(out[2], out[3]);
        if (p + DEPTH_ITEMS == n) P[n] = out[DEPTH_ITEMS];
    } else {
        for (uint32_t j = 0; p + j <= n; j++) P[p + j] = out[j]; // (the tile's last thread: P[n] as well)
    }
}

__global__ __launch_bounds__(BT) void k_depthw_prefix(const int32_t *__restrict__ diff, uint64_t t0, uint32_t n, const int32_t *__restrict__ bdepth,
                                                      const uint64_t *__restrict__ bP, uint64_t *__restrict__ P) {
    const uint32_t p = blockIdx.x * DEPTH_GRANULE + threadIdx.x * DEPTH_ITEMS;
    const Items it = load_items(diff, t0, n, p);
    Agg total;
    const Agg e = block_exclusive(it.agg, &total);
    if (p >= n) return;
    const int32_t din = bdepth[blockIdx.x];
    int32_t depth = din + e.d;
    uint64_t at = bP[blockIdx.x] + (uint64_t)e.s + (uint64_t)((long long)e.n * din); // P[p]
    uint64_t out[DEPTH_ITEMS + 1];
    for (uint32_t j = 0; j < DEPTH_ITEMS; j++) {
        out[j] = at;
        depth += it.v[j];
        at += (uint64_t)(long long)depth;
    }
    out[DEPTH_ITEMS] = at;
    store_prefix(P, p, n, out);
}

__global__ __launch_bounds__(BT) void k_depthw_window_sums(const uint64_t *__restrict__ P, uint64_t origin, uint32_t window, uint64_t kb, uint32_t count,
                                                           uint32_t hi, uint64_t *__restrict__ sum, const DepthWState *ws) {
    const uint32_t j = blockIdx.x * BT + threadIdx.x;
    if (j >= count) return;
    const uint64_t end = min((kb + j + 1) * (uint64_t)window, (uint64_t)hi);
    const uint64_t front = j ? P[(kb + j) * (uint64_t)window - origin] : ws->bound;
    sum[j] = P[end - origin] - front;
}

__global__ void k_depthw_bound(const uint64_t *P, uint64_t origin, uint32_t window, uint64_t kb, uint32_t count, uint32_t hi, DepthWState *ws) {
    ws->bound = P[min((kb + count) * (uint64_t)window, (uint64_t)hi) - origin];
}

__global__ __launch_bounds__(BT) void k_depthw_interval_acc(const ngsq_depth_interval *__restrict__ iv, uint64_t count, const uint64_t *__restrict__ P,
                                                            uint64_t t0, uint32_t n, uint64_t *__restrict__ acc) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (i >= count) return;
    const uint64_t s = iv[i].start, e = iv[i].end;
    const bool has_e = e > t0 && e <= t0 + n, has_s = s >= t0 && s < t0 + n;
    if (!has_e && !has_s) return;
    uint64_t a = acc[i];
    if (has_e) a += P[e - t0];
    if (has_s) a -= P[s - t0];
    acc[i] = a;
}

// line k of a source
struct Line {
    uint32_t start, end;
    uint64_t sum;
};
__device__ inline Line line_of(const DepthLineSource &s, uint64_t k) {
    Line l;
    if (s.window) {
        l.start = (uint32_t)max((s.kb + k) * (uint64_t)s.window, (uint64_t)s.lo);
        l.end = (uint32_t)min((s.kb + k + 1) * (uint64_t)s.window, (uint64_t)s.hi);
    } else {
        l.start = s.iv[k].start;
        l.end = s.iv[k].end;
    }
    l.sum = s.zero ? 0 : s.sum[k];
    return l;
}

// The mean with two decimals, rounded half up, in integers: sum / len = w.f
__device__ inline void mean_of(const Line &l, uint64_t *w, uint32_t *f) {
    const uint64_t len = l.end - l.start, r = l.sum % len;
    *w = l.sum / len;
    *f = (uint32_t)((100u * r + len / 2u) / len);
    if (*f == 100u) *w += 1, *f = 0;
}

__device__ inline uint32_t digits64(uint64_t v) {
    uint32_t n = 1;
    while (v >= 10u) v /= 10u, n++;
    return n;
}

__global__ __launch_bounds__(BT) void k_depthw_size(DepthLineSource src, uint64_t k0, uint32_t m, uint32_t name_len, uint64_t *__restrict__ off,
                                                    DepthWState *ws) {
    const uint32_t k = blockIdx.x * BT + threadIdx.x; // (the grid covers m + 1 entries)
    uint64_t bytes = 0, sum = 0;
    if (k < m) {
        const Line l = line_of(src, k0 + k);
        uint64_t w;
        uint32_t f;
        mean_of(l, &w, &f);
        bytes = name_len + 3u + digits64(l.start) + digits64(l.end) + digits64(w) + 4u; // three tabs; ".ff\n"
        sum = l.sum;
    }
    if (k <= m) off[k] = bytes;
    for (uint32_t d = 32; d; d >>= 1) sum += __shfl_xor(sum, d);
    if ((threadIdx.x & 63u) == 0 && sum) (void)atomicAdd(&ws->depth_sum, (unsigned long long)sum);
}

__global__ void k_depthw_total(const uint64_t *off, uint32_t m, const DepthWState *ws, unsigned long long *host) {
    host[0] = off[m];
    host[1] = ws->depth_sum;
}

// v in decimal, its last digit at p[-1]; returns where its first digit lies
__device__ inline char *put_back(char *p, uint64_t v) {
    do {
        *--p = (char)('0' + (uint32_t)(v % 10u));
        v /= 10u;
    } while (v);
    return p;
}

// "name\tstart\tend\tw.ff\n" at dst, `bytes` long
__device__ inline void put_line(char *dst, uint32_t bytes, const char *__restrict__ name, uint32_t name_len, const Line &l) {
    uint64_t w;
    uint32_t f;
    mean_of(l, &w, &f);
    for (uint32_t j = 0; j < name_len; j++) dst[j] = name[j];
    char *p = dst + bytes;
    *--p = '\n';
    *--p = (char)('0' + f % 10u);
    *--p = (char)('0' + f / 10u);
    *--p = '.';
    p = put_back(p, w);
    *--p = '\t';
    p = put_back(p, l.end);
    *--p = '\t';
    p = put_back(p, l.start);
    *--p = '\t';
}

// The staged piece [g0, g1) of the text, in `stage` from byte `phase` on, behind the block's barrier: aligned words, bytes at its two ends.
__device__ inline void store_piece(const uint32_t *stage, uintptr_t g0, uintptr_t g1, uint32_t phase) {
    const uintptr_t gbase = g0 - phase;
    const uint32_t n_words = (uint32_t)((g1 - gbase + 3u) / 4u);
    for (uint32_t wd = threadIdx.x; wd < n_words; wd += BT) {
        const uintptr_t a = gbase + (uintptr_t)wd * 4u;
        if (a >= g0 && a + 4u <= g1) {
            *reinterpret_cast<uint32_t *>(a) = stage[wd];
        } else {
            const char *from = reinterpret_cast<const char *>(stage) + wd * 4u;
            for (uint32_t j = 0; j < 4; j++)
                if (a + j >= g0 && a + j < g1) *reinterpret_cast<char *>(a + j) = from[j];
        }
    }
}

// k_depth_write's scheme: the lines of a block are one contiguous piece of the text, written into LDS at the piece's own phase
// against a 4-byte boundary and stored as aligned words (bytes at its two ends); a piece that does not fit is stored byte by byte.
__global__ __launch_bounds__(BT) void k_depthw_write(char *__restrict__ text, DepthLineSource src, uint64_t k0, uint32_t m, const char *__restrict__ name,
                                                     uint32_t name_len, const uint64_t *__restrict__ off) {
    __shared__ uint32_t stage[DEPTH_STAGE_BYTES / 4];
    const uint32_t a0 = blockIdx.x * BT, a1 = min(a0 + BT, m), k = a0 + threadIdx.x;
    const uint64_t b0 = off[a0], b1 = off[a1];
    const uintptr_t g0 = reinterpret_cast<uintptr_t>(text) + b0, g1 = reinterpret_cast<uintptr_t>(text) + b1;
    const uint32_t phase = (uint32_t)(g0 & 3u);
    const bool staged = b1 - b0 + phase <= DEPTH_STAGE_BYTES; // (the same in every thread)
    if (k < a1) {
        const uint64_t at = off[k];
        const uint32_t bytes = (uint32_t)(off[k + 1] - at);
        char *dst = staged ? reinterpret_cast<char *>(stage) + phase + (uint32_t)(at - b0) : text + at;
        put_line(dst, bytes, name, name_len, line_of(src, k0 + k));
    }
    if (!staged) return;
    __syncthreads();
    store_piece(stage, g0, g1, phase);
}

inline bool grid_of(uint64_t n, uint32_t per_block, uint32_t *blocks) {
    const uint64_t g = (n + per_block - 1) / per_block;
    *blocks = (uint32_t)g;
    return g >= 1 && g <= 0x7FFFFFFFull;
}

// a source the kernels can take lines [k0, k0 + m) of
inline bool source_ok(const DepthLineSource &src, uint64_t k0, uint32_t m) {
    if (!m || k0 + m > src.count) return false;
    if (src.window ? src.lo >= src.hi : !src.iv) return false;
    return src.zero || src.sum;
}

} // namespace

hipError_t launch_depthw_prefix(const DepthWindow &w, uint64_t t0, uint32_t n, const DepthWTileArrays &a, DepthWState *ws, hipStream_t s) {
    uint32_t blocks;
    if (!w.diff || !a.bdepth || !a.bsum || !a.bP || !a.P || !ws) return hipErrorInvalidValue;
    if (t0 % DEPTH_GRANULE || t0 + n > w.len || !grid_of(n, DEPTH_GRANULE, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_depthw_sums, dim3(blocks), dim3(BT), 0, s, w.diff, t0, n, a.bdepth, a.bsum);
    hipLaunchKernelGGL(k_depthw_offsets, dim3(1), dim3(BT), 0, s, blocks, n, a.bdepth, a.bsum, a.bP, ws);
    hipLaunchKernelGGL(k_depthw_prefix, dim3(blocks), dim3(BT), 0, s, w.diff, t0, n, a.bdepth, a.bP, a.P);
    return hipGetLastError();
}

hipError_t launch_depthw_window_sums(const uint64_t *P, uint64_t origin, uint32_t n, uint32_t window, uint64_t kb, uint32_t count, uint32_t hi,
                                     uint64_t *sum, DepthWState *ws, hipStream_t s) {
    uint32_t blocks;
    if (!P || !sum || !ws || !window || !n || !grid_of(count, BT, &blocks)) return hipErrorInvalidValue;
    // every boundary the kernels look up lies in the tile: the first window's end behind its first position, the last one's at or in front of its end
    const uint64_t first_end = std::min<uint64_t>((kb + 1) * window, hi), last_end = std::min<uint64_t>((kb + count) * window, hi);
    if (first_end <= origin || last_end > origin + n || (kb + count - 1) * window >= hi) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_depthw_window_sums, dim3(blocks), dim3(BT), 0, s, P, origin, window, kb, count, hi, sum, ws);
    hipLaunchKernelGGL(k_depthw_bound, dim3(1), dim3(1), 0, s, P, origin, window, kb, count, hi, ws);
    return hipGetLastError();
}

hipError_t launch_depthw_interval_acc(const ngsq_depth_interval *iv, uint64_t count, const uint64_t *P, uint64_t t0, uint32_t n, uint64_t *acc,
                                      hipStream_t s) {
    uint32_t blocks;
    if (!iv || !P || !acc || !n || !grid_of(count, BT, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_depthw_interval_acc, dim3(blocks), dim3(BT), 0, s, iv, count, P, t0, n, acc);
    return hipGetLastError();
}

hipError_t launch_depthw_size(const DepthLineSource &src, uint64_t k0, uint32_t m, uint32_t name_len, uint64_t *off, DepthWState *ws, hipStream_t s) {
    uint32_t blocks;
    if (!off || !ws || !source_ok(src, k0, m) || !grid_of((uint64_t)m + 1, BT, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_depthw_size, dim3(blocks), dim3(BT), 0, s, src, k0, m, name_len, off, ws);
    return hipGetLastError();
}

hipError_t launch_depthw_total(const uint64_t *off, uint32_t m, const DepthWState *ws, unsigned long long *host, hipStream_t s) {
    if (!off || !ws || !host || !m) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_depthw_total, dim3(1), dim3(1), 0, s, off, m, ws, host);
    return hipGetLastError();
}

hipError_t launch_depthw_write(char *text, const DepthLineSource &src, uint64_t k0, uint32_t m, const char *name, uint32_t name_len, const uint64_t *off,
                               hipStream_t s) {
    uint32_t blocks;
    if (!text || !off || (!name && name_len) || !source_ok(src, k0, m) || !grid_of(m, BT, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_depthw_write, dim3(blocks), dim3(BT), 0, s, text, src, k0, m, name, name_len, off);
    return hipGetLastError();
}

// ---- `ngs depth --by ... --thresholds` -----------------------------------------------------------------
namespace {

constexpr uint32_t MAXT = NGSQ_DEPTH_MAX_THRESHOLDS;
static_assert(MAXT == 8, "two words of four 16-bit fields hold the thresholds");
static_assert(DEPTH_GRANULE <= 0xFFFFu, "a block's count fits a 16-bit field");

// The counts of up to eight thresholds, four 16-bit fields a word.  A thread's field is at most DEPTH_ITEMS and a block's total at
// most DEPTH_GRANULE, so no field carries into its neighbour.
struct Packed {
    unsigned long long w[2];
};
__device__ inline uint32_t field(const Packed &v, uint32_t k) { return (uint32_t)(v.w[k >> 2] >> (16u * (k & 3u))) & 0xFFFFu; }

// What the block's threads in front of this one add up to, field by field, and the whole block; `words` (1 or 2, the same in
// every thread) of the two are scanned.  Two barriers.
__device__ inline Packed block_exclusive_packed(const Packed own, uint32_t words, Packed *total) {
    __shared__ unsigned long long wt[2][BT / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    Packed in = own;
#pragma unroll
    for (uint32_t h = 0; h < 2; h++) {
        if (h >= words) break;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const unsigned long long l = __shfl_up(in.w[h], d);
            if (lane >= d) in.w[h] += l;
        }
        if (lane == 63) wt[h][wave] = in.w[h];
    }
    __syncthreads();
    Packed ex{{0, 0}}, all{{0, 0}};
#pragma unroll
    for (uint32_t h = 0; h < 2; h++) {
        if (h >= words) break;
        for (uint32_t k = 0; k < BT / 64; k++) {
            const unsigned long long w = wt[h][k];
            if (k < wave) ex.w[h] += w;
            all.w[h] += w;
        }
        ex.w[h] += in.w[h] - own.w[h];
    }
    *total = all;
    __syncthreads();
    return ex;
}

// k_depthw_prefix and, from the same read of the tile, per threshold the block-relative inclusive counts cin and the block's total.
__global__ __launch_bounds__(BT) void k_deptht_prefix(const int32_t *__restrict__ diff, uint64_t t0, uint32_t n, const int32_t *__restrict__ bdepth,
                                                      const uint64_t *__restrict__ bP, uint64_t *__restrict__ P, DepthThresholds thr,
                                                      uint16_t *__restrict__ cin, uint64_t stride, uint32_t *__restrict__ bcnt, uint32_t bstride) {
    const uint32_t p = blockIdx.x * DEPTH_GRANULE + threadIdx.x * DEPTH_ITEMS;
    const Items it = load_items(diff, t0, n, p);
    Agg total;
    const Agg e = block_exclusive(it.agg, &total);
    const int32_t din = bdepth[blockIdx.x];
    int32_t depth = din + e.d;
    uint64_t at = bP[blockIdx.x] + (uint64_t)e.s + (uint64_t)((long long)e.n * din); // P[p]
    uint64_t out[DEPTH_ITEMS + 1];
    int32_t dep[DEPTH_ITEMS]; // the depth of the thread's positions; one beyond the tile reaches no threshold
    for (uint32_t j = 0; j < DEPTH_ITEMS; j++) {
        out[j] = at;
        depth += it.v[j];
        dep[j] = p + j < n ? depth : 0;
        at += (uint64_t)(long long)depth;
    }
    out[DEPTH_ITEMS] = at;
    Packed own{{0, 0}};
#pragma unroll
    for (uint32_t k = 0; k < MAXT; k++) {
        if (k >= thr.k) break;
        uint32_t c = 0;
        for (uint32_t j = 0; j < DEPTH_ITEMS; j++) c += dep[j] >= (int32_t)thr.t[k] ? 1u : 0u;
        own.w[k >> 2] += (unsigned long long)c << (16u * (k & 3u));
    }
    Packed all;
    const Packed ex = block_exclusive_packed(own, thr.k > 4u ? 2u : 1u, &all);
    if (threadIdx.x == 0) {
#pragma unroll
        for (uint32_t k = 0; k < MAXT; k++)
            if (k < thr.k) bcnt[(uint64_t)k * bstride + blockIdx.x] = field(all, k);
    }
    if (p >= n) return;
    store_prefix(P, p, n, out);
#pragma unroll
    for (uint32_t k = 0; k < MAXT; k++) {
        if (k >= thr.k) break;
        uint32_t c = field(ex, k);
        ushort4 q;
        c += dep[0] >= (int32_t)thr.t[k] ? 1u : 0u, q.x = (unsigned short)c;
        c += dep[1] >= (int32_t)thr.t[k] ? 1u : 0u, q.y = (unsigned short)c;
        c += dep[2] >= (int32_t)thr.t[k] ? 1u : 0u, q.z = (unsigned short)c;
        c += dep[3] >= (int32_t)thr.t[k] ? 1u : 0u, q.w = (unsigned short)c;
        *reinterpret_cast<ushort4 *>(cin + (uint64_t)k * stride + p) = q; // (8-byte aligned; the row is padded to the granule)
    }
}

// one block: per threshold, the blocks' totals into C_k entering every block, from the carry, which moves on to the tile's end
__global__ __launch_bounds__(BT) void k_deptht_offsets(uint32_t n_blocks, uint32_t K, const uint32_t *__restrict__ bcnt, uint32_t *__restrict__ bC,
                                                       uint32_t bstride, DepthTState *ts) {
    __shared__ uint32_t wt[BT / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t k = 0; k < K; k++) {
        uint32_t run = ts->C[k];
        for (uint32_t base = 0; base < n_blocks; base += BT) {
            const uint32_t i = base + threadIdx.x;
            const uint32_t own = i < n_blocks ? bcnt[(uint64_t)k * bstride + i] : 0u;
            uint32_t in = own;
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint32_t l = __shfl_up(in, d);
                if (lane >= d) in += l;
            }
            if (lane == 63) wt[wave] = in;
            __syncthreads();
            uint32_t before = 0, all = 0;
            for (uint32_t w = 0; w < BT / 64; w++) {
                if (w < wave) before += wt[w];
                all += wt[w];
            }
            __syncthreads();
            if (i < n_blocks) bC[(uint64_t)k * bstride + i] = run + before + in - own;
            run += all;
        }
        if (threadIdx.x == 0) ts->C[k] = run; // (n_blocks >= 1: every thread has read the carry in front of a barrier)
    }
}

// C_k in front of tile position x, x = 0 .. n (depth_windows_kernels.h: the block looked at is that of position x - 1)
__device__ inline uint32_t count_at(const DepthTTileArrays &t, uint32_t k, uint64_t x) {
    if (!x) return t.bC[(uint64_t)k * t.bstride];
    const uint64_t j = x - 1;
    return t.bC[(uint64_t)k * t.bstride + j / DEPTH_GRANULE] + t.cin[(uint64_t)k * t.stride + j];
}

__global__ __launch_bounds__(BT) void k_deptht_window_counts(DepthTTileArrays t, uint32_t K, uint64_t origin, uint32_t window, uint64_t kb, uint32_t count,
                                                             uint32_t hi, uint32_t *__restrict__ cnt, uint64_t cstride, const DepthTState *ts) {
    const uint32_t j = blockIdx.x * BT + threadIdx.x;
    if (j >= count) return;
    const uint64_t end = min((kb + j + 1) * (uint64_t)window, (uint64_t)hi);
    for (uint32_t k = 0; k < K; k++) {
        const uint32_t front = j ? count_at(t, k, (kb + j) * (uint64_t)window - origin) : ts->boundC[k];
        cnt[(uint64_t)k * cstride + j] = count_at(t, k, end - origin) - front;
    }
}

__global__ void k_deptht_bound(DepthTTileArrays t, uint32_t K, uint64_t origin, uint32_t window, uint64_t kb, uint32_t count, uint32_t hi, DepthTState *ts) {
    if (threadIdx.x < K) ts->boundC[threadIdx.x] = count_at(t, threadIdx.x, min((kb + count) * (uint64_t)window, (uint64_t)hi) - origin);
}

__global__ __launch_bounds__(BT) void k_deptht_interval_acc(const ngsq_depth_interval *__restrict__ iv, uint64_t count, DepthTTileArrays t, uint32_t K,
                                                            uint64_t t0, uint32_t n, uint32_t *__restrict__ acc, uint64_t cstride) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (i >= count) return;
    const uint64_t s = iv[i].start, e = iv[i].end;
    const bool has_e = e > t0 && e <= t0 + n, has_s = s >= t0 && s < t0 + n;
    if (!has_e && !has_s) return;
    for (uint32_t k = 0; k < K; k++) {
        uint32_t a = acc[(uint64_t)k * cstride + i];
        if (has_e) a += count_at(t, k, e - t0);
        if (has_s) a -= count_at(t, k, s - t0);
        acc[(uint64_t)k * cstride + i] = a;
    }
}

__device__ inline uint32_t count_of(const DepthTLineSource &s, uint32_t j, uint64_t k) { return s.base.zero ? 0u : s.cnt[(uint64_t)j * s.cstride + k]; }

__global__ __launch_bounds__(BT) void k_deptht_size(DepthTLineSource src, uint64_t k0, uint32_t m, uint32_t name_len, uint64_t *__restrict__ off,
                                                    DepthWState *ws, DepthTState *ts) {
    const uint32_t k = blockIdx.x * BT + threadIdx.x; // (the grid covers m + 1 entries)
    uint64_t bytes = 0, sum = 0;
    if (k < m) {
        const Line l = line_of(src.base, k0 + k);
        uint64_t w;
        uint32_t f;
        mean_of(l, &w, &f);
        bytes = name_len + 3u + digits64(l.start) + digits64(l.end) + digits64(w) + 4u; // three tabs; ".ff\n"
        sum = l.sum;
    }
    for (uint32_t d = 32; d; d >>= 1) sum += __shfl_xor(sum, d);
    if ((threadIdx.x & 63u) == 0 && sum) (void)atomicAdd(&ws->depth_sum, (unsigned long long)sum);
    for (uint32_t j = 0; j < src.K; j++) {
        unsigned long long c = k < m ? count_of(src, j, k0 + k) : 0u;
        if (k < m) bytes += 1u + digits64(c); // "\t<n_j>"
        for (uint32_t d = 32; d; d >>= 1) c += __shfl_xor(c, d);
        if ((threadIdx.x & 63u) == 0 && c) (void)atomicAdd(&ts->covered[j], c);
    }
    if (k <= m) off[k] = bytes;
}

__global__ void k_deptht_total(const uint64_t *off, uint32_t m, uint32_t K, const DepthWState *ws, const DepthTState *ts, unsigned long long *host) {
    host[0] = off[m];
    host[1] = ws->depth_sum;
    for (uint32_t k = 0; k < K; k++) host[DEPTHW_HOST_WORDS + k] = ts->covered[k];
}

// "name\tstart\tend\tw.ff\tn_1\t...\tn_K\n" at dst, `bytes` long: the counts from the end, section 24's line in front of them
__device__ inline void put_line_counts(char *dst, uint32_t bytes, const char *__restrict__ name, uint32_t name_len, const Line &l, const DepthTLineSource &s,
                                       uint64_t k) {
    char *p = dst + bytes;
    *--p = '\n';
    for (uint32_t j = s.K; j-- > 0;) {
        p = put_back(p, count_of(s, j, k));
        *--p = '\t';
    }
    put_line(dst, (uint32_t)(p - dst) + 1u, name, name_len, l); // (its newline falls on the tab in front of n_1)
    *p = '\t';
}

// k_depthw_write with the K columns
__global__ __launch_bounds__(BT) void k_deptht_write(char *__restrict__ text, DepthTLineSource src, uint64_t k0, uint32_t m, const char *__restrict__ name,
                                                     uint32_t name_len, const uint64_t *__restrict__ off) {
    __shared__ uint32_t stage[DEPTH_STAGE_BYTES / 4];
    const uint32_t a0 = blockIdx.x * BT, a1 = min(a0 + BT, m), k = a0 + threadIdx.x;
    const uint64_t b0 = off[a0], b1 = off[a1];
    const uintptr_t g0 = reinterpret_cast<uintptr_t>(text) + b0, g1 = reinterpret_cast<uintptr_t>(text) + b1;
    const uint32_t phase = (uint32_t)(g0 & 3u);
    const bool staged = b1 - b0 + phase <= DEPTH_STAGE_BYTES; // (the same in every thread)
    if (k < a1) {
        const uint64_t at = off[k];
        const uint32_t bytes = (uint32_t)(off[k + 1] - at);
        char *dst = staged ? reinterpret_cast<char *>(stage) + phase + (uint32_t)(at - b0) : text + at;
        put_line_counts(dst, bytes, name, name_len, line_of(src.base, k0 + k), src, k0 + k);
    }
    if (!staged) return;
    __syncthreads();
    store_piece(stage, g0, g1, phase);
}

inline bool k_ok(uint32_t K) { return K >= 1 && K <= MAXT; }

// the count arrays hold a tile of n positions
inline bool tile_arrays_ok(const DepthTTileArrays &t, uint32_t n) {
    const uint64_t blocks = ((uint64_t)n + DEPTH_GRANULE - 1) / DEPTH_GRANULE;
    return t.cin && t.bcnt && t.bC && n && t.stride % DEPTH_GRANULE == 0 && t.stride >= blocks * DEPTH_GRANULE && t.bstride >= blocks;
}

inline bool tsource_ok(const DepthTLineSource &src, uint64_t k0, uint32_t m) {
    if (!k_ok(src.K) || !source_ok(src.base, k0, m)) return false;
    return src.base.zero || (src.cnt && src.cstride >= src.base.count);
}

} // namespace

hipError_t launch_deptht_prefix(const DepthWindow &w, uint64_t t0, uint32_t n, const DepthWTileArrays &a, const DepthTTileArrays &t,
                                const DepthThresholds &thr, DepthWState *ws, DepthTState *ts, hipStream_t s) {
    uint32_t blocks;
    if (!w.diff || !a.bdepth || !a.bsum || !a.bP || !a.P || !ws || !ts || !k_ok(thr.k) || !tile_arrays_ok(t, n)) return hipErrorInvalidValue;
    if (t0 % DEPTH_GRANULE || t0 + n > w.len || !grid_of(n, DEPTH_GRANULE, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_depthw_sums, dim3(blocks), dim3(BT), 0, s, w.diff, t0, n, a.bdepth, a.bsum);
    hipLaunchKernelGGL(k_depthw_offsets, dim3(1), dim3(BT), 0, s, blocks, n, a.bdepth, a.bsum, a.bP, ws);
    hipLaunchKernelGGL(k_deptht_prefix, dim3(blocks), dim3(BT), 0, s, w.diff, t0, n, a.bdepth, a.bP, a.P, thr, t.cin, t.stride, t.bcnt, t.bstride);
    hipLaunchKernelGGL(k_deptht_offsets, dim3(1), dim3(BT), 0, s, blocks, thr.k, t.bcnt, t.bC, t.bstride, ts);
    return hipGetLastError();
}

hipError_t launch_deptht_window_counts(const DepthTTileArrays &t, uint32_t K, uint64_t origin, uint32_t n, uint32_t window, uint64_t kb, uint32_t count,
                                       uint32_t hi, uint32_t *cnt, uint64_t cstride, DepthTState *ts, hipStream_t s) {
    uint32_t blocks;
    if (!cnt || !ts || !window || !k_ok(K) || !tile_arrays_ok(t, n) || cstride < count || !grid_of(count, BT, &blocks)) return hipErrorInvalidValue;
    // (launch_depthw_window_sums' test: every boundary looked up lies in the tile)
    const uint64_t first_end = std::min<uint64_t>((kb + 1) * window, hi), last_end = std::min<uint64_t>((kb + count) * window, hi);
    if (first_end <= origin || last_end > origin + n || (kb + count - 1) * window >= hi) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_deptht_window_counts, dim3(blocks), dim3(BT), 0, s, t, K, origin, window, kb, count, hi, cnt, cstride, ts);
    hipLaunchKernelGGL(k_deptht_bound, dim3(1), dim3(64), 0, s, t, K, origin, window, kb, count, hi, ts);
    return hipGetLastError();
}

hipError_t launch_deptht_interval_acc(const ngsq_depth_interval *iv, uint64_t count, const DepthTTileArrays &t, uint32_t K, uint64_t t0, uint32_t n,
                                      uint32_t *acc, uint64_t cstride, hipStream_t s) {
    uint32_t blocks;
    if (!iv || !acc || !k_ok(K) || !tile_arrays_ok(t, n) || cstride < count || !grid_of(count, BT, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_deptht_interval_acc, dim3(blocks), dim3(BT), 0, s, iv, count, t, K, t0, n, acc, cstride);
    return hipGetLastError();
}

hipError_t launch_deptht_size(const DepthTLineSource &src, uint64_t k0, uint32_t m, uint32_t name_len, uint64_t *off, DepthWState *ws, DepthTState *ts,
                              hipStream_t s) {
    uint32_t blocks;
    if (!off || !ws || !ts || !tsource_ok(src, k0, m) || !grid_of((uint64_t)m + 1, BT, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_deptht_size, dim3(blocks), dim3(BT), 0, s, src, k0, m, name_len, off, ws, ts);
    return hipGetLastError();
}

hipError_t launch_deptht_total(const uint64_t *off, uint32_t m, uint32_t K, const DepthWState *ws, const DepthTState *ts, unsigned long long *host,
                               hipStream_t s) {
    if (!off || !ws || !ts || !host || !m || !k_ok(K)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_deptht_total, dim3(1), dim3(1), 0, s, off, m, K, ws, ts, host);
    return hipGetLastError();
}

hipError_t launch_deptht_write(char *text, const DepthTLineSource &src, uint64_t k0, uint32_t m, const char *name, uint32_t name_len, const uint64_t *off,
                               hipStream_t s) {
    uint32_t blocks;
    if (!text || !off || (!name && name_len) || !tsource_ok(src, k0, m) || !grid_of(m, BT, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_deptht_write, dim3(blocks), dim3(BT), 0, s, text, src, k0, m, name, name_len, off);
    return hipGetLastError();
}

} // namespace ngsq
