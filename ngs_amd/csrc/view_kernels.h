// view_kernels.h -- `ngs view <BAM> <QUERY>` on the device: which records of a batch of the device
// ingest belong to the region.  Launcher only; view_kernel.hip has the kernel, view.cpp the driver.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/ngsq_view.h"

namespace ngsq {

// the region and the merged chunks of its query, on the device
struct ViewRegion {
    const ngsq_view_chunk *chunks; // ascending, disjoint: [begin, end) virtual offsets
    uint32_t n_chunks;
    int32_t ref_id;
    uint64_t start, end; // 1-based, inclusive
    uint64_t lo, hi;     // the walk's own virtual offsets [lo, hi): what lies outside is another walk's (or nobody's)
};

// keep[i] = 1 when record i of the batch is the region's (its record_id lies in the walk and in a chunk, its sequence is the region's,
// pos >= 0, and [pos + 1, pos + max(reference span, 1)] meets [start, end]), else 0; *kept += the records kept.
hipError_t launch_view_select(const ngsq_batch &b, const ViewRegion &region, uint8_t *keep, unsigned long long *kept, hipStream_t s);

} // namespace ngsq
