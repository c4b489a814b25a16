// view_kernel.hip -- `ngs view <BAM> <QUERY>` on the device: the selection of a region's records.  One
// thread per record of the batch: a binary search of the record's virtual offset over the query's merged chunks, the
// sequence and position tests on the batch's columns, and -- only for a record that starts in front of the region -- the
// reference span of its CIGAR (the batch's resolved operations: a long CIGAR's come from its CG tag).  The kept records are
// counted by a popcount per wave and one atomic per wave.
#include <hip/hip_runtime.h>

#include "view_kernels.h"

namespace ngsq {

namespace {

constexpr uint32_t BT = 256;

__global__ __launch_bounds__(BT) void k_view_select(ngsq_batch b, ViewRegion g, uint8_t *__restrict__ keep, unsigned long long *kept) {
    const uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x;
    bool k = false;
    if (i < b.n_records) {
        const int64_t pos = b.pos[i];
        k = b.ref_id[i] == g.ref_id && pos >= 0 && (uint64_t)pos + 1 <= g.end;
        if (k) { // the last chunk that begins at or in front of the record holds it, or none does
            const uint64_t v = b.record_id[i];
            k = v >= g.lo && v < g.hi;
            uint32_t lo = 0, hi = g.n_chunks; // chunks [0, lo) begin at or in front of v
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (g.chunks[mid].begin <= v) lo = mid + 1;
                else hi = mid;
            }
            k = k && lo > 0 && v < g.chunks[lo - 1].end;
        }
        if (k && (uint64_t)pos + 1 < g.start) { // it starts in front of the region: does it reach it?
            uint64_t k0, n_ops;
            if (b.cigar_off) {
                k0 = b.cigar_off[i];
                n_ops = b.cigar_off[i + 1] - k0;
            } else {
                k0 = i * (uint64_t)b.cigar_stride;
                n_ops = min((uint32_t)b.n_cigar[i], b.cigar_stride);
            }
            uint64_t span = 0;
            for (uint64_t c = 0; c < n_ops && (uint64_t)pos + span < g.start; c++) {
                const uint32_t op = b.cigar[k0 + c];
                if ((0x18Du >> (op & 15u)) & 1u) span += op >> 4; // M D N = X
            }
            k = (uint64_t)pos + (span ? span : 1) >= g.start;
        }
        keep[i] = k;
    }
    const unsigned long long m = __ballot(k);
    if ((threadIdx.x & 63u) == 0 && m) (void)atomicAdd(kept, (unsigned long long)__popcll(m));
}

} // namespace

hipError_t launch_view_select(const ngsq_batch &b, const ViewRegion &region, uint8_t *keep, unsigned long long *kept, hipStream_t s) {
    if (!b.n_records) return hipSuccess;
    const uint64_t blocks = (b.n_records + BT - 1) / BT;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_view_select, dim3((uint32_t)blocks), dim3(BT), 0, s, b, region, keep, kept);
    return hipGetLastError();
}

} // namespace ngsq
