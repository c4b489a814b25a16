// ingest_consumer.h -- what the code that walks a file through the device ingest shares: the reader itself
// (bam_device_reader.cpp) and its consumers inside the library, `ngs index` (bai.cpp) and `ngs convert` (sam.cpp).
#pragma once

#include <chrono>

#include "bam_reader.h"
#include "ingest_kernels.h"
#include "mem_pool.h"

// a HIP call inside a function that reports through ngsq_bam_fail and returns its code
#define BHIP(expr)                                                                                           \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) return ngsq_bam_fail(NGSQ_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

namespace ngsq {

inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// A consumer walks the file from its first record: it refuses a reader that has handed out records already.
// made: what is made from it, as its message says it ("an index is built", "a SAM file is written").
inline int require_fresh_reader(const ngsq_bam *b, const char *made) {
    if (b->dev || b->host_mode || b->n_read)
        return ngsq_bam_fail(NGSQ_ERR_STATE, "%s: %s from a reader no record has been read from", b->path.c_str(), made);
    return NGSQ_OK;
}

// The next batch of the device ingest and, when it holds records, where they came from.  n_records == 0 ends the walk.
inline int next_batch_with_origin(ngsq_bam *b, ngsq_ctx *c, uint64_t max_records, ngsq_batch *bt, BatchOrigin *o) {
    const int rc = ngsq_bam_next_batch_device(b, c, max_records, bt);
    if (rc || !bt->n_records) return rc;
    return bam_device_batch_origin(b, o);
}

// launch_exclusive_scan_u64 with the scratch it needs: exclusive prefix sums of n + 1 entries in place (entry n = total)
struct ScanScratch {
    DevArray<uint8_t> tmp;
    hipError_t exclusive_scan(uint64_t *data, uint64_t n_plus_1, hipStream_t s) {
        size_t bytes = 0;
        hipError_t e = launch_exclusive_scan_u64(data, n_plus_1, nullptr, &bytes, s); // (asks for the size: no launch)
        if (e == hipSuccess) e = tmp.reserve(bytes);
        if (e != hipSuccess) return e;
        bytes = tmp.cap;
        return launch_exclusive_scan_u64(data, n_plus_1, tmp.p, &bytes, s);
    }
};

} // namespace ngsq
