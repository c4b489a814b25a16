// derive_kernel.hip -- `ngs derive instrument` on the device.  One lane per record reads the name,
// counts its colons and hashes the instrument segment and the flowcell segment; the two exact sets of byte strings are
// open-addressing tables over a string arena.  A launch reads only what earlier launches wrote (a slot's epoch tells), so
// the steady state -- every name already in the table -- is plain loads and no atomic.  A name that is not found is
// appended: by the lane that claims an empty slot (atomicCAS), or as a candidate without a slot when the claim is lost,
// the slot met was claimed in this launch, or the probe ran out.  No wave waits for another, and nothing one workgroup
// stores is read by another within the launch; the host de-duplicates the appended strings exactly (derive.cpp).
#include <hip/hip_runtime.h>

#include "derive_kernels.h"

namespace ngsq {

namespace {

constexpr uint32_t BT = 256;
constexpr uint32_t MAX_PROBES = 64; // slots looked at before a name is given up as a candidate

struct Name {
    const uint8_t *p;
    uint32_t len;
    unsigned long long h; // never 0
};

constexpr unsigned long long FNV_BASIS = 0xCBF29CE484222325ull, FNV_PRIME = 0x100000001B3ull;

__device__ __forceinline__ unsigned long long finish_hash(unsigned long long h, uint32_t len) {
    h ^= (unsigned long long)len * 0x9E3779B97F4A7C15ull;
    h ^= h >> 32;
    h *= 0xD6E8FEB86659FD93ull;
    h ^= h >> 32;
    return h ? h : 1;
}

__device__ __forceinline__ bool bytes_equal(const uint8_t *a, const uint8_t *b, uint32_t n) {
    for (uint32_t k = 0; k < n; k++)
        if (a[k] != b[k]) return false;
    return true;
}

enum Lookup : uint32_t { FOUND = 0, EMPTY_SLOT, NO_SLOT };

// The name among the slots earlier launches filled.  EMPTY_SLOT: it is not there and *slot is where it would go.
// NO_SLOT: a slot with its hash was claimed in this launch (its string cannot be read yet), or MAX_PROBES slots were taken.
__device__ Lookup lookup(const DeriveSlot *__restrict__ T, uint32_t slots, uint32_t epoch, const uint8_t *__restrict__ arena,
                         const Name &q, uint32_t *slot) {
    const uint32_t mask = slots - 1, probes = slots < MAX_PROBES ? slots : MAX_PROBES;
    uint32_t at = (uint32_t)q.h & mask;
    for (uint32_t k = 0; k < probes; k++, at = (at + 1) & mask) {
        const unsigned long long key = T[at].key;
        if (key == 0) {
            *slot = at;
            return EMPTY_SLOT;
        }
        if (key != q.h) continue;
        const uint32_t e = T[at].epoch;
        if (e == 0 || e >= epoch) return NO_SLOT;
        if (T[at].len == q.len && bytes_equal(arena + T[at].off, q.p, q.len)) return FOUND;
        // the same hash and other bytes: a collision, the name's place is further on
    }
    return NO_SLOT;
}

// the string into the arena and the entry list; false: no room (the overflow word is set)
__device__ bool append(const DeriveSets &S, uint32_t set, const Name &q, uint32_t *off_out) {
    DeriveState *st = S.state;
    const unsigned long long off = atomicAdd(&st->arena_used, (unsigned long long)q.len);
    const unsigned long long idx = atomicAdd(&st->n_entries, 1ull);
    if (off + q.len > S.arena_cap || idx >= S.entries_cap) {
        atomicExch(&st->overflow, 1ull);
        return false;
    }
    for (uint32_t k = 0; k < q.len; k++) S.arena[off + k] = q.p[k];
    S.entries[idx] = DeriveEntry{(uint32_t)off, q.len, set};
    *off_out = (uint32_t)off;
    return true;
}

// One set's part of a wave's work.  have: the lane holds a name for this set.  Every lane of the wave calls it.
__device__ void resolve(const DeriveSets &S, uint32_t set, uint32_t epoch, bool have, const Name &q) {
    const uint32_t lane = threadIdx.x & 63u;
    DeriveSlot *T = S.table[set];
    uint32_t slot = 0;
    Lookup r = FOUND;
    if (have) r = lookup(T, S.slots, epoch, S.arena, q, &slot);
    bool need = have && r != FOUND;
    // the lanes of the wave that hold the same string (bytes compared: equal hashes are not enough) append it once
    unsigned long long pending = __ballot(need);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const unsigned long long lh = __shfl(q.h, leader), lp = __shfl((unsigned long long)(uintptr_t)q.p, leader);
        const uint32_t ll = __shfl(q.len, leader);
        if (need && (uint32_t)leader == lane) {
            uint32_t off = 0;
            bool won = false;
            if (r == EMPTY_SLOT && *(volatile unsigned long long *)&S.state->overflow == 0)
                won = atomicCAS(&T[slot].key, 0ull, q.h) == 0ull;
            if (won) {
                if (append(S, set, q, &off)) {
                    // for later launches only: this launch trusts no slot of its own epoch
                    __hip_atomic_store(&T[slot].off, off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&T[slot].len, q.len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&T[slot].epoch, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            } else {
                (void)append(S, set | DERIVE_CANDIDATE, q, &off);
            }
            need = false;
        } else if (need && q.h == lh && q.len == ll && bytes_equal(q.p, reinterpret_cast<const uint8_t *>((uintptr_t)lp), ll)) {
            need = false;
        }
        pending = __ballot(need);
    }
}

__global__ __launch_bounds__(BT) void k_derive_names(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ rec_off, uint64_t n,
                                                     uint64_t base, uint32_t epoch, DeriveSets S) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    Name ins{nullptr, 0, 1}, fc{nullptr, 0, 1};
    bool has_ins = false, has_fc = false, star = false;
    if (i < n) {
        const uint8_t *rec = raw + rec_off[i]; // block_size, then the 32 fixed bytes (l_read_name at 8), then the name
        const uint32_t l_rn = rec[12], len = l_rn ? l_rn - 1 : 0;
        const uint8_t *name = rec + 36;
        if (len == 1 && name[0] == '*') {
            star = true;
        } else {
            uint32_t colons = 0, ins_len = len, fc_at = 0, fc_end = 0;
            unsigned long long hi = FNV_BASIS, hf = FNV_BASIS;
            for (uint32_t k = 0; k < len; k++) {
                const uint32_t ch = name[k];
                if (ch == ':') {
                    colons++;
                    if (colons == 1) ins_len = k;
                    else if (colons == 2) fc_at = k + 1;
                    else if (colons == 3) fc_end = k;
                } else if (colons == 0) {
                    hi = (hi ^ ch) * FNV_PRIME;
                } else if (colons == 2) {
                    hf = (hf ^ ch) * FNV_PRIME;
                }
            }
            if (colons == 4 || colons == 6) {
                has_ins = true;
                ins = Name{name, ins_len, finish_hash(hi, ins_len)};
                if (colons == 6) {
                    has_fc = true;
                    fc = Name{name + fc_at, fc_end - fc_at, finish_hash(hf, fc_end - fc_at)};
                }
            } else {
                atomicMin(&S.state->bad, (unsigned long long)(base + i));
            }
        }
    }
    const uint32_t stars = (uint32_t)__popcll(__ballot(star));
    if (stars && (threadIdx.x & 63u) == 0) atomicAdd(&S.state->skipped, (unsigned long long)stars);
    resolve(S, 0, epoch, has_ins, ins);
    resolve(S, 1, epoch, has_fc, fc);
}

// one wave, behind k_derive_names: the words the host reads
__global__ __launch_bounds__(64) void k_derive_tail(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ rec_off, uint64_t n, uint64_t base,
                                                    const DeriveState *__restrict__ st, unsigned long long *host) {
    const unsigned long long bad = st->bad;
    if (bad != ~0ull && bad >= base && bad - base < n) {
        const uint8_t *rec = raw + rec_off[bad - base];
        const uint32_t l_rn = rec[12], len = l_rn ? l_rn - 1 : 0;
        uint8_t *dst = reinterpret_cast<uint8_t *>(host + 4);
        for (uint32_t k = threadIdx.x; k < len; k += 64) dst[k] = rec[36 + k];
        if (threadIdx.x == 0) host[2] = len;
    }
    if (threadIdx.x == 0) {
        host[0] = bad;
        host[1] = st->overflow;
    }
}

} // namespace

hipError_t launch_derive_names(const ngsq_batch &b, const BatchOrigin &o, uint64_t base, uint32_t epoch, const DeriveSets &sets,
                               unsigned long long *host, hipStream_t s) {
    const uint64_t n = b.n_records;
    if (!n) return hipSuccess;
    if (!sets.slots || (sets.slots & (sets.slots - 1)) || !epoch) return hipErrorInvalidValue;
    const uint64_t blocks = (n + BT - 1) / BT;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_derive_names, dim3((uint32_t)blocks), dim3(BT), 0, s, o.raw, o.rec_off, n, base, epoch, sets);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_derive_tail, dim3(1), dim3(64), 0, s, o.raw, o.rec_off, n, base, sets.state, host);
    return hipGetLastError();
}

} // namespace ngsq
