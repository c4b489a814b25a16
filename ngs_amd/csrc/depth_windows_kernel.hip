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
    if (p + DEPTH_ITEMS <= n) { // (32-byte aligned: p is a multiple of 4)
        *reinterpret_cast<ulonglong2 *>(P + p) = make_ulonglong2(out[0], out[1]);
        *reinterpret_cast<ulonglong2 *>(P + p + 2) = make_ulonglong2(out[2], out[3]);
        if (p + DEPTH_ITEMS == n) P[n] = out[DEPTH_ITEMS];
    } else {
        for (uint32_t j = 0; p + j <= n; j++) P[p + j] = out[j]; // (the tile's last thread: P[n] as well)
    }
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

} // namespace ngsq
