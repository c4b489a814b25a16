// sam_run.h -- the SAM formatter the commands that write SAM text share (`ngs convert`, sam.cpp; `ngs view`, view.cpp):
// sam_kernel.hip sizes every record's SAM line of a batch of the device ingest, the ingest's scan turns the sizes into offsets,
// and a second pass writes the lines into a device buffer of the batch's real size.  The output stage of device_out.h carries
// the text of batch k to the file while the main thread ingests and formats batch k+1.  The host never walks the records.
// DESIGN.md sections 13 and 15.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "context.h"
#include "device_out.h"
#include "ingest_consumer.h"
#include "sam_kernels.h"

namespace ngsq {

constexpr uint64_t SAM_BATCH_RECORDS = (uint64_t)1 << 20;

inline const char *sam_error_text(uint32_t code) {
    switch (code) {
    case SAM_E_REF: return "reference sequence id out of range";
    case SAM_E_CIGAR_OP: return "invalid CIGAR operation";
    case SAM_E_QUAL: return "quality score above 93";
    case SAM_E_TAG_TYPE: return "invalid tag value type";
    case SAM_E_STR_NUL: return "Z or H tag value without its NUL";
    case SAM_E_B_SUB: return "invalid B array subtype";
    case SAM_E_OVERRUN: return "tag value runs past the end of the record";
    default: return "invalid record";
    }
}

// What the batches of one run share: the formatter's device arrays, the writer, the counts and times of the report.
struct SamRun {
    ngsq_bam *b = nullptr;
    ngsq_ctx *c = nullptr;
    hipStream_t st = nullptr;
    // the @SQ names on the device, the error word, the words the host reads
    DevArray<uint64_t> d_setup;
    unsigned long long *d_bad = nullptr;
    SamRefs refs{};
    MappedBuf hw;
    // the output stage: the writer (a copy stream, the pinned ring, its thread) and the two slots of d_text
    DeviceWriter w;
    JobSlots slots;
    HipEvents<4> ev; // format brackets: size a/b, write a/b
    DevArray<uint64_t> d_off, d_flist;
    DevArray<uint8_t> d_fmark;
    ScanScratch scan;
    DevArray<char> d_text[2];
    uint64_t records = 0, text_bytes = 0; // records: of the batches formatted, kept or not
    double scan_ms = 0, format_ms = 0;
    bool write_pending = false; // the last write pass's bracket has not been added to format_ms yet

    void add_write_time() {
        float ms = 0;
        if (write_pending && hipEventElapsedTime(&ms, ev.e[2], ev.e[3]) == hipSuccess) format_ms += ms;
        write_pending = false;
    }
    int begin(ngsq_bam *bam, ngsq_ctx *ctx, int fd, uint64_t first_batch_records);
    int format_batch(const ngsq_batch &bt, const BatchOrigin &o, const uint8_t *keep, bool *more, uint64_t *bad);
    int finish(int rc, const char *context);
};

// The device side of a run and its writer thread: the @SQ names, the error word, the events, the per-record arrays for the
// largest batch asked for (a batch's write pass may still read them when the next one begins).
inline int SamRun::begin(ngsq_bam *bam, ngsq_ctx *ctx, int fd, uint64_t first_batch_records) {
    b = bam;
    c = ctx;
    st = ctx->stream;
    const uint32_t n_refs = (uint32_t)b->ref_names.size();
    std::vector<uint64_t> setup(n_refs + 2, 0); // [bad | name_off[n_refs + 1]] then the names
    std::string names;
    for (uint32_t k = 0; k < n_refs; k++) {
        setup[1 + k] = names.size();
        names += b->ref_names[k];
    }
    setup[1 + n_refs] = names.size();
    setup[0] = ~0ull;
    BHIP(d_setup.reserve(setup.size() + (names.size() + 7) / 8));
    BHIP(hipMemcpyAsync(d_setup.p, setup.data(), setup.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (!names.empty()) BHIP(hipMemcpyAsync(d_setup.p + setup.size(), names.data(), names.size(), hipMemcpyHostToDevice, st));
    BHIP(hipStreamSynchronize(st)); // (setup and names are this function's)
    d_bad = reinterpret_cast<unsigned long long *>(d_setup.p);
    refs.names = reinterpret_cast<const char *>(d_setup.p + setup.size());
    refs.name_off = d_setup.p + 1;
    refs.n_refs = n_refs;
    BHIP(hw.reserve(8 * sizeof(unsigned long long)));
    memset(hw.h, 0, 8 * sizeof(unsigned long long));
    BHIP(slots.create());
    for (auto &e : ev.e) BHIP(hipEventCreate(&e));
    BHIP(w.start(fd, c->device));
    const uint64_t n0 = first_batch_records;
    if (d_off.reserve(n0 + 1) != hipSuccess || d_fmark.reserve(n0) != hipSuccess || d_flist.reserve(n0 + 1) != hipSuccess)
        return ngsq_bam_fail(NGSQ_ERR_DEVICE, "allocating the SAM formatter's arrays for %llu records", (unsigned long long)n0);
    return NGSQ_OK;
}

// One batch of the device ingest: sized, scanned, written into a device buffer and handed to the writer.  keep (optional,
// device, [n]): a record with keep[i] == 0 has no line.  *more = false: nothing more can be written (a writer that has failed:
// its error is read at the end).  *bad != ~0: a record that cannot be written, (index in the walk << SAM_ERR_BITS | SamError);
// nothing of the batch has been handed to the writer then.
inline int SamRun::format_batch(const ngsq_batch &bt, const BatchOrigin &o, const uint8_t *keep, bool *more, uint64_t *bad_out) {
    *more = false;
    *bad_out = ~0ull;
    const uint64_t n = bt.n_records;
    BHIP(d_off.reserve(n + 1));
    BHIP(d_fmark.reserve(n));
    BHIP(d_flist.reserve(n + 1));
    const SamFloats fl{d_fmark.p, d_flist.p + 1, reinterpret_cast<unsigned long long *>(d_flist.p)};
    // sizes, offsets, and the batch's text bytes and error word to the host
    BHIP(hipEventRecord(ev.e[0], st));
    BHIP(launch_sam_size(bt, o, refs, d_off.p, d_bad, fl, st, keep));
    BHIP(scan.exclusive_scan(d_off.p, n + 1, st));
    BHIP(launch_sam_total(d_off.p, n, d_bad, static_cast<unsigned long long *>(hw.dev), st));
    BHIP(hipEventRecord(ev.e[1], st));
    BHIP(hipEventSynchronize(ev.e[1]));
    {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.e[0], ev.e[1]) == hipSuccess) format_ms += ms;
    }
    add_write_time();
    const unsigned long long *const h = static_cast<const unsigned long long *>(hw.h);
    const uint64_t bytes = h[0], bad = h[1];
    if (bad != ~0ull) {
        *bad_out = bad;
        return NGSQ_OK;
    }
    if (!slots.acquire(&w)) return NGSQ_OK;
    DevArray<char> &text = d_text[slots.slot()];
    BHIP(text.reserve(bytes + 1));
    BHIP(hipEventRecord(ev.e[2], st));
    BHIP(launch_sam_write(bt, o, refs, d_off.p, text.p, fl, st, keep));
    BHIP(hipEventRecord(ev.e[3], st));
    BHIP(slots.submit(w, text.p, bytes, st));
    write_pending = true;
    records += n;
    text_bytes += bytes;
    *more = !w.werr;
    return NGSQ_OK;
}

// The end of a run whose batches gave `rc`: the stream drained, every queued copy written (or skipped after a failed write),
// the writer's own errors reported under `context` ("writing SAM record").
inline int SamRun::finish(int rc, const char *context) {
    if (rc == NGSQ_OK) {
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = ngsq_bam_fail(NGSQ_ERR_DEVICE, "hipStreamSynchronize: %s", hipGetErrorString(e));
        add_write_time();
    }
    const WriterEnd end = w.end();
    if (rc == NGSQ_OK && end.herr != hipSuccess) rc = ngsq_bam_fail(NGSQ_ERR_DEVICE, "copying the SAM text to the host: %s", hipGetErrorString(end.herr));
    if (rc == NGSQ_OK && end.werr) rc = ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "%s: %s (os error %d)", context, strerror(end.werr), end.werr);
    if (rc != NGSQ_OK) (void)hipStreamSynchronize(st); // (the drain rule, by hand: the callers keep arrays of their own beside the run)
    return rc;
}

} // namespace ngsq
