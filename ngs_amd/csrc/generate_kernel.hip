// generate_kernel.hip -- `ngs generate` on the device (the rules are the reference's
// src/generate/providers/reference_provider.rs:291-393 and src/generate/providers.rs:29-48, the draws this build's own).
//   k_gen_draw   one wave per pair: provider, then attempt after attempt (sequence, start, inner distance) until the fragment
//                lies inside the sequence and holds nothing but ACGTacgt -- the 64 lanes scan it 64 bytes at a time
//   k_gen_total  the batch's text bytes, the error word and the rejection counters to the host
//   k_gen_write  one wave per pair: both records, a byte per lane, with the per-base substitutions
#include <hip/hip_runtime.h>

#include "generate_draw.h"
#include "generate_kernels.h"
#include "../../include/ngsq_generate.h"

namespace ngsq {
namespace {

constexpr uint32_t BT = 256; // four waves, four pairs
constexpr uint32_t PAIRS_PER_BLOCK = BT / 64;

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

__device__ __forceinline__ uint32_t dec_digits(uint64_t v) {
    uint32_t d = 1;
    while (v >= 10) {
        v /= 10;
        d++;
    }
    return d;
}

__device__ __forceinline__ bool is_acgt(uint32_t c) {
    c &= ~0x20u; // (folds case; the four letters have no neighbour that folds onto them)
    return c == 'A' || c == 'C' || c == 'G' || c == 'T';
}

// utils.rs:96-108, case kept
__device__ __forceinline__ uint32_t complement(uint32_t c) {
    const uint32_t low = c & 0x20u, u = c & ~0x20u;
    const uint32_t v = u == 'A' ? 'T' : u == 'C' ? 'G' : u == 'G' ? 'C' : 'A';
    return v | low;
}

// the number of entries of the non-decreasing a[0, n) that are <= x
__device__ __forceinline__ uint32_t count_le(const uint64_t *__restrict__ a, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n; // a[k] <= x for k < lo, a[k] > x for k >= hi
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// bytes of either record of a pair: "@ngs:" file ':' sequence ':' start ':' number "/1\n" bases "\n+\n" Js "\n"
__device__ __forceinline__ uint64_t record_bytes(const GenProviderDev &P, const GenSeqDev &S, uint64_t start, uint64_t number) {
    return 5ull + P.fname_len + 1 + S.name_len + 1 + dec_digits(start) + 1 + dec_digits(number) + 3 + P.read_length + 3 + P.read_length + 1;
}

__global__ __launch_bounds__(BT) void k_gen_draw(GenTables T, uint64_t seed, uint64_t first, uint64_t n, GenPick *__restrict__ pick,
                                                 uint64_t *__restrict__ len, unsigned long long *__restrict__ work) {
    const uint64_t i = (uint64_t)blockIdx.x * PAIRS_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= n) return; // (a whole wave: i is the wave's)
    const uint32_t lane = lane_id();
    const uint64_t pair = first + i, key = gen_pair_key(seed, pair);
    // every lane computes lane 0's draws: they are the wave's
    const uint64_t xw = gen_below(gen_draw(key, GEN_PROVIDER, 0), T.total_weight);
    uint32_t p = 0;
    while (p + 1 < T.n_prov && T.prov[p].weight_end <= xw) p++;
    const GenProviderDev P = T.prov[p];
    const uint64_t L = P.read_length;
    const uint64_t *const cum = T.seq_cum + P.cum_first;
    const uint64_t *const tab = T.inner + P.tab_first;
    uint32_t rej_start = 0, rej_end = 0, rej_base = 0;
    bool found = false;
    GenPick out{};
    for (uint32_t a = 0; a < NGSQ_GENERATE_MAX_ATTEMPTS; a++) {
        const uint64_t xs = gen_below(gen_draw(key, GEN_SEQUENCE, a), P.elig_total);
        const uint32_t s = count_le(cum, P.n_seq + 1, xs) - 1; // cum[s] <= xs < cum[s + 1]: an eligible sequence
        const GenSeqDev S = T.seq[P.seq_first + s];
        const uint64_t start = gen_below(gen_draw(key, GEN_START, a), S.len - 2 * L);
        const uint32_t j = count_le(tab, P.tab_n - 1, gen_draw(key, GEN_INNER, a));
        const uint64_t flen = (uint64_t)((int64_t)(2 * L) + P.inner_lower + (int64_t)j); // >= L: checked up front
        if (start == 0) { // Position is 1-based
            rej_start++;
            continue;
        }
        if (flen > S.len || start - 1 > S.len - flen) { // chr.get(start..end) is None
            rej_end++;
            continue;
        }
        const uint8_t *const f = S.bases + (start - 1);
        bool bad = false;
        for (uint64_t o = 0; o < flen && !bad; o += 64) { // (uniform: the ballot is the wave's)
            const uint64_t k = o + lane;
            const bool mine = k < flen && !is_acgt(f[k]);
            bad = __ballot(mine) != 0;
        }
        if (bad) { // reverse_compliment returns None
            rej_base++;
            continue;
        }
        out.start = start;
        out.flen = flen;
        out.prov = p;
        out.seq = P.seq_first + s;
        found = true;
        break;
    }
    if (lane == 0) {
        pick[i] = out;
        len[i] = found ? record_bytes(P, T.seq[out.seq], out.start, pair + 1) : 0;
        if (i == n - 1) len[n] = 0;
        if (rej_start) (void)atomicAdd(work + GW_REJ_START, (unsigned long long)rej_start);
        if (rej_end) (void)atomicAdd(work + GW_REJ_END, (unsigned long long)rej_end);
        if (rej_base) (void)atomicAdd(work + GW_REJ_BASE, (unsigned long long)rej_base);
        if (!found) (void)atomicMin(work + GW_BAD, (unsigned long long)pair << GEN_ERR_BITS | GEN_E_ATTEMPTS);
    }
}

__global__ void k_gen_total(const uint64_t *__restrict__ off, uint64_t n, const unsigned long long *__restrict__ work, unsigned long long *host) {
    if (threadIdx.x == 0) {
        host[0] = off[n];
        for (uint32_t k = 0; k < GEN_WORK_WORDS; k++) host[1 + k] = work[k];
    }
}

// providers.rs:29-48: with probability 1 / error_freq the base becomes one of A C G T that differs from it, each equally likely
__device__ __forceinline__ uint32_t with_error(uint32_t c, uint64_t key, uint32_t hit, uint32_t base, uint32_t j, uint64_t error_freq) {
    if (gen_below(gen_draw(key, hit, j), error_freq) != 0) return c;
    const uint64_t v = gen_draw(key, base, j);
    const uint32_t ci = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; // 4: lower case, all four differ
    uint32_t k;
    if (ci < 4) {
        k = (uint32_t)gen_below(v, 3);
        k += k >= ci;
    } else {
        k = (uint32_t)gen_below(v, 4);
    }
    return k == 0 ? 'A' : k == 1 ? 'C' : k == 2 ? 'G' : 'T';
}

// decimal digits of v at q[0, d), by one lane
__device__ __forceinline__ void put_dec(char *q, uint64_t v, uint32_t d) {
    for (uint32_t k = d; k-- > 0;) {
        q[k] = (char)('0' + v % 10);
        v /= 10;
    }
}

__global__ __launch_bounds__(BT) void k_gen_write(GenTables T, uint64_t seed, uint64_t first, uint64_t n, const GenPick *__restrict__ pick,
                                                  const uint64_t *__restrict__ off, char *__restrict__ one, char *__restrict__ two) {
    const uint64_t i = (uint64_t)blockIdx.x * PAIRS_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= n) return;
    const uint32_t lane = lane_id();
    const uint64_t pair = first + i, key = gen_pair_key(seed, pair);
    const GenPick pk = pick[i];
    const GenProviderDev P = T.prov[pk.prov];
    const GenSeqDev S = T.seq[pk.seq];
    const uint64_t L = P.read_length;
    char *const d1 = one + off[i], *const d2 = two + off[i];
    // ---- the name line
    uint64_t at = 0;
    if (lane < 5) d1[lane] = d2[lane] = "@ngs:"[lane];
    at = 5;
    for (uint32_t k = lane; k < P.fname_len; k += 64) d1[at + k] = d2[at + k] = T.names[P.fname_off + k];
    at += P.fname_len;
    for (uint32_t k = lane; k < S.name_len; k += 64) d1[at + 1 + k] = d2[at + 1 + k] = T.names[S.name_off + k];
    const uint32_t ds = dec_digits(pk.start), dn = dec_digits(pair + 1);
    if (lane == 0) {
        d1[at] = d2[at] = ':';
        uint64_t q = at + 1 + S.name_len;
        d1[q] = d2[q] = ':';
        put_dec(d1 + q + 1, pk.start, ds);
        put_dec(d2 + q + 1, pk.start, ds);
        q += 1 + ds;
        d1[q] = d2[q] = ':';
        put_dec(d1 + q + 1, pair + 1, dn);
        put_dec(d2 + q + 1, pair + 1, dn);
        q += 1 + dn;
        d1[q] = d2[q] = '/';
        d1[q + 1] = '1';
        d2[q + 1] = '2';
        d1[q + 2] = d2[q + 2] = '\n';
    }
    at += 1 + S.name_len + 1 + ds + 1 + dn + 3;
    // ---- the bases: read one forward from the fragment's start, read two backward from its end, complemented
    const uint8_t *const f = S.bases + (pk.start - 1);
    for (uint64_t j = lane; j < L; j += 64) {
        const uint32_t b1 = f[j], b2 = complement(f[pk.flen - 1 - j]);
        d1[at + j] = (char)with_error(b1, key, GEN_HIT_ONE, GEN_BASE_ONE, (uint32_t)j, P.error_freq);
        d2[at + j] = (char)with_error(b2, key, GEN_HIT_TWO, GEN_BASE_TWO, (uint32_t)j, P.error_freq);
    }
    at += L;
    if (lane < 3) d1[at + lane] = d2[at + lane] = "\n+\n"[lane];
    at += 3;
    for (uint64_t j = lane; j < L; j += 64) d1[at + j] = d2[at + j] = 'J';
    if (lane == 0) d1[at + L] = d2[at + L] = '\n';
}

} // namespace

hipError_t launch_gen_draw(const GenTables &t, uint64_t seed, uint64_t first, uint64_t n, GenPick *pick, uint64_t *len, unsigned long long *work,
                           hipStream_t s) {
    if (!n) return hipSuccess;
    const uint64_t blocks = (n + PAIRS_PER_BLOCK - 1) / PAIRS_PER_BLOCK;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gen_draw, dim3((uint32_t)blocks), dim3(BT), 0, s, t, seed, first, n, pick, len, work);
    return hipGetLastError();
}

hipError_t launch_gen_total(const uint64_t *off, uint64_t n, const unsigned long long *work, unsigned long long *host, hipStream_t s) {
    hipLaunchKernelGGL(k_gen_total, dim3(1), dim3(64), 0, s, off, n, work, host);
    return hipGetLastError();
}

hipError_t launch_gen_write(const GenTables &t, uint64_t seed, uint64_t first, uint64_t n, const GenPick *pick, const uint64_t *off, char *one, char *two,
                            hipStream_t s) {
    if (!n) return hipSuccess;
    const uint64_t blocks = (n + PAIRS_PER_BLOCK - 1) / PAIRS_PER_BLOCK;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gen_write, dim3((uint32_t)blocks), dim3(BT), 0, s, t, seed, first, n, pick, off, one, two);
    return hipGetLastError();
}

} // namespace ngsq
