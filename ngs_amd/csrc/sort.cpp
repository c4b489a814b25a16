// sort.cpp -- include/ngsq_sort.h: host memory in, the permutation in host memory out, sorted on the device (sort_kernel.hip,
// DESIGN.md section 19.3); and sort_pairs_u64, the pass loop that entry and the driver of `ngs convert --sort coordinate`
// (samsort.cpp) share.
#include "../../include/ngsq_sort.h"

#include <cstdarg>
#include <cstring>
#include <string>

#include "device_out.h"
#include "sort_kernels.h"

using namespace ngsq;

namespace {

thread_local std::string g_sort_err;

int ofail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_sort_err = buf;
    return code;
}

} // namespace

namespace ngsq {

hipError_t sort_pairs_u64(uint64_t *keys, uint64_t n, SortScratch &sc, hipStream_t s, const uint32_t **perm) {
    sc.passes_run = sc.passes_skipped = 0;
    if (!n || n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipError_t e = sc.hist.reserve(SORT_DIGITS * SORT_BINS);
    if (e == hipSuccess) e = sc.idx[0].reserve(n);
    if (e == hipSuccess) e = launch_sort_histogram(keys, n, sc.hist.p, s);
    unsigned long long hist[SORT_DIGITS * SORT_BINS];
    if (e == hipSuccess) e = hipMemcpyAsync(hist, sc.hist.p, sizeof hist, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    // a digit that is the same in every key orders nothing
    bool runs[SORT_DIGITS];
    for (uint32_t d = 0; d < SORT_DIGITS; d++) {
        runs[d] = true;
        for (uint32_t b = 0; b < SORT_BINS; b++)
            if (hist[d * SORT_BINS + b] == n) runs[d] = false;
        (runs[d] ? sc.passes_run : sc.passes_skipped)++;
    }
    if (!sc.passes_run) {
        *perm = sc.idx[0].p;
        return launch_sort_iota(sc.idx[0].p, n, s);
    }
    e = sc.keys_b.reserve(n);
    if (e == hipSuccess) e = sc.idx[1].reserve(n);
    if (e == hipSuccess) e = sc.table.reserve(sort_table_entries(n));
    if (e != hipSuccess) return e;
    uint64_t *kin = keys, *kout = sc.keys_b.p;
    const uint32_t *iin = nullptr; // (the first pass numbers the pairs itself)
    uint32_t turn = 0;
    for (uint32_t d = 0; d < SORT_DIGITS; d++) {
        if (!runs[d]) continue;
        uint32_t *iout = sc.idx[turn].p;
        e = launch_sort_count(kin, n, d, sc.table.p, s);
        if (e == hipSuccess) e = sc.scan.exclusive_scan(sc.table.p, sort_table_entries(n), s);
        if (e == hipSuccess) e = launch_sort_scatter(kin, iin, n, d, sc.table.p, kout, iout, s);
        if (e != hipSuccess) return e;
        std::swap(kin, kout);
        iin = iout;
        turn ^= 1;
    }
    *perm = iin;
    return hipSuccess;
}

} // namespace ngsq

extern "C" {

uint32_t ngsq_sort_tile_keys(void) { return SORT_TILE; }
uint64_t ngsq_sort_resident_bytes_per_record(void) { return SORT_BYTES_PER_RECORD; }
uint64_t ngsq_sort_survey_bytes_per_record(void) { return SORT_SURVEY_BYTES_PER_RECORD; }
const char *ngsq_sort_last_error(void) { return g_sort_err.c_str(); }

int ngsq_sort_u64_device(int device, const uint64_t *keys, uint64_t n, uint32_t *perm, ngsq_sort_report *rep) {
    if (rep) memset(rep, 0, sizeof *rep);
    if (n && (!keys || !perm)) return ofail(NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    if (n > 0xFFFFFFFFull) return ofail(NGSQ_ERR_LIMIT, "%llu keys: more than 2^32 - 1", (unsigned long long)n);
    const double t_begin = now_ms();
    if (rep) rep->passes_skipped = SORT_DIGITS;
    if (!n) return NGSQ_OK;
#define OHIP(expr)                                                                                 \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return ofail(NGSQ_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
    OHIP(hipSetDevice(device));
    DevArray<uint64_t> d_keys;
    SortScratch sc;
    HipEvents<2> ev;
    StreamDrain drain{nullptr, true}; // (behind the arrays: it runs first)
    OHIP(pool_stream_get(false, &drain.s));
    const hipStream_t st = drain.s;
    for (auto &x : ev.e) OHIP(hipEventCreate(&x));
    OHIP(d_keys.reserve(n));
    OHIP(hipMemcpyAsync(d_keys.p, keys, n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    OHIP(hipEventRecord(ev.e[0], st));
    const uint32_t *d_perm = nullptr;
    OHIP(sort_pairs_u64(d_keys.p, n, sc, st, &d_perm));
    OHIP(hipEventRecord(ev.e[1], st));
    OHIP(hipMemcpyAsync(perm, d_perm, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    OHIP(hipStreamSynchronize(st));
#undef OHIP
    if (rep) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.e[0], ev.e[1]) == hipSuccess) rep->sort_ms = ms;
        rep->passes_run = sc.passes_run;
        rep->passes_skipped = sc.passes_skipped;
        rep->total_ms = now_ms() - t_begin;
    }
    return NGSQ_OK;
}

} // extern "C"
