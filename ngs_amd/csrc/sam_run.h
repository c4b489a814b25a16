// sam_run.h -- what the commands that write SAM text share (`ngs convert`, sam.cpp; `ngs view`, view.cpp): sam_kernel.hip sizes
// every record's SAM line of a batch of the device ingest, the ingest's scan turns the sizes into offsets, and a second pass
// writes the lines into a device buffer of the batch's real size.  A writer thread copies the text of batch k to a pinned ring
// on a second stream (behind an event of the formatter) and writes the ring to the file in order, while the main thread
// ingests and formats batch k+1.  The host never walks the records.  DESIGN.md sections 13 and 15.
#pragma once

#include <hip/hip_runtime_api.h>
#include <errno.h>
#include <unistd.h>

#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "context.h"
#include "ingest_consumer.h"
#include "sam_kernels.h"

namespace ngsq {

constexpr uint64_t SAM_BATCH_RECORDS = (uint64_t)1 << 20;
constexpr uint32_t SAM_RING_SLOTS = 4;
constexpr size_t SAM_RING_PIECE = (size_t)32 << 20; // bytes per slot of the pinned ring

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

// write(2) until done; 0 or errno
inline int write_all(int fd, const char *p, size_t n) {
    while (n) {
        const ssize_t w = write(fd, p, n);
        if (w < 0) {
            if (errno == EINTR) continue;
            return errno;
        }
        if (w == 0) return EIO;
        p += w;
        n -= (size_t)w;
    }
    return 0;
}

// The text of one batch, as the main thread hands it to the writer: copy it once `ready` has completed on the copy stream.
struct SamJob {
    const char *dev;
    uint64_t bytes;
    hipEvent_t ready;
    uint64_t batch;
};

// The writer thread: copies the jobs to the ring, SAM_RING_PIECE bytes per slot, and writes the slots to fd in order, keeping up
// to SAM_RING_SLOTS copies in flight while it writes.
struct SamWriter {
    int fd = -1, device = 0;
    hipStream_t cs = nullptr;
    char *ring = nullptr;
    hipEvent_t t0[SAM_RING_SLOTS] = {}, t1[SAM_RING_SLOTS] = {};
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    std::deque<SamJob> jobs;
    bool finish = false;
    uint64_t batches_copied = 0; // batches whose every copy has completed (their device buffer may be reused)
    int werr = 0;                // errno of a failed write: nothing more is written
    hipError_t herr = hipSuccess;
    double copy_ms = 0, write_ms = 0;
    std::thread th;

    void run() {
        // the ring is pinned here, beside the first batch's ingest and formatting (some 25 ms for 128 MiB)
        herr = hipSetDevice(device);
        if (herr == hipSuccess) {
            void *h = nullptr;
            herr = hipHostMalloc(&h, SAM_RING_SLOTS * SAM_RING_PIECE, hipHostMallocDefault);
            ring = static_cast<char *>(h);
        }
        for (uint32_t s = 0; s < SAM_RING_SLOTS && herr == hipSuccess; s++) {
            herr = hipEventCreate(&t0[s]);
            if (herr == hipSuccess) herr = hipEventCreate(&t1[s]);
        }
        if (herr != hipSuccess) {
            std::lock_guard<std::mutex> g(mu);
            cv_done.notify_all();
        }
        struct Piece {
            uint32_t slot;
            size_t len;
            bool last;
            uint64_t batch;
        };
        std::deque<Piece> inflight;
        SamJob cur{};
        uint64_t cur_off = 0;
        bool have = false;
        uint32_t next_slot = 0;
        for (;;) {
            // queue copies while a slot is free
            while (inflight.size() < SAM_RING_SLOTS) {
                if (!have) {
                    std::lock_guard<std::mutex> g(mu);
                    if (jobs.empty()) break;
                    cur = jobs.front();
                    jobs.pop_front();
                    cur_off = 0;
                    have = true;
                    if (herr == hipSuccess) herr = hipStreamWaitEvent(cs, cur.ready, 0);
                }
                const size_t len = (size_t)std::min<uint64_t>(SAM_RING_PIECE, cur.bytes - cur_off);
                const uint32_t s = next_slot;
                next_slot = (next_slot + 1) % SAM_RING_SLOTS;
                if (herr == hipSuccess && len) {
                    herr = hipEventRecord(t0[s], cs);
                    if (herr == hipSuccess) herr = hipMemcpyAsync(ring + (size_t)s * SAM_RING_PIECE, cur.dev + cur_off, len, hipMemcpyDeviceToHost, cs);
                    if (herr == hipSuccess) herr = hipEventRecord(t1[s], cs);
                }
                cur_off += len;
                const bool last = cur_off >= cur.bytes;
                inflight.push_back(Piece{s, len, last, cur.batch});
                if (last) have = false;
            }
            if (inflight.empty()) {
                std::unique_lock<std::mutex> g(mu);
                cv_work.wait(g, [&] { return finish || !jobs.empty(); });
                if (jobs.empty() && finish) return;
                continue;
            }
            const Piece pc = inflight.front();
            inflight.pop_front();
            if (herr == hipSuccess && pc.len) {
                herr = hipEventSynchronize(t1[pc.slot]);
                float ms = 0;
                if (herr == hipSuccess && hipEventElapsedTime(&ms, t0[pc.slot], t1[pc.slot]) == hipSuccess) copy_ms += ms;
            }
            if (pc.last || herr != hipSuccess) {
                std::lock_guard<std::mutex> g(mu);
                if (pc.last) batches_copied = pc.batch + 1;
                cv_done.notify_all();
            }
            if (herr == hipSuccess && !werr && pc.len) {
                const double w0 = now_ms();
                werr = write_all(fd, ring + (size_t)pc.slot * SAM_RING_PIECE, pc.len);
                write_ms += now_ms() - w0;
            }
        }
    }
    void push(const SamJob &j) {
        {
            std::lock_guard<std::mutex> g(mu);
            jobs.push_back(j);
        }
        cv_work.notify_one();
    }
    // wait until the copies of batches [0, n) have completed; false: a copy failed
    bool wait_copied(uint64_t n) {
        std::unique_lock<std::mutex> g(mu);
        cv_done.wait(g, [&] { return batches_copied >= n || herr != hipSuccess; });
        return herr == hipSuccess;
    }
    void stop() {
        if (!th.joinable()) return;
        {
            std::lock_guard<std::mutex> g(mu);
            finish = true;
        }
        cv_work.notify_one();
        th.join();
    }
    ~SamWriter() {
        stop();
        if (cs) {
            (void)hipStreamSynchronize(cs);
            pool_stream_put(false, cs);
        }
        for (uint32_t s = 0; s < SAM_RING_SLOTS; s++) {
            if (t0[s]) (void)hipEventDestroy(t0[s]);
            if (t1[s]) (void)hipEventDestroy(t1[s]);
        }
        if (ring) (void)hipHostFree(ring);
    }
};

struct SamEvents {
    hipEvent_t e[6] = {};
    ~SamEvents() {
        for (auto x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

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
    // the writer: a copy stream, the pinned ring, its thread
    SamWriter w;
    SamEvents ev; // ready[2]; format brackets: size a/b, write a/b
    DevArray<uint64_t> d_off, d_flist;
    DevArray<uint8_t> d_fmark;
    ScanScratch scan;
    DevArray<char> d_text[2];
    uint64_t records = 0, text_bytes = 0, batches = 0; // records: of the batches formatted, kept or not
    double scan_ms = 0, format_ms = 0;
    bool write_pending = false; // the last write pass's bracket has not been added to format_ms yet

    void add_write_time() {
        float ms = 0;
        if (write_pending && hipEventElapsedTime(&ms, ev.e[4], ev.e[5]) == hipSuccess) format_ms += ms;
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
    w.fd = fd;
    w.device = c->device;
    BHIP(pool_stream_get(false, &w.cs));
    BHIP(hipEventCreateWithFlags(&ev.e[0], hipEventDisableTiming));
    BHIP(hipEventCreateWithFlags(&ev.e[1], hipEventDisableTiming));
    for (int k = 2; k < 6; k++) BHIP(hipEventCreate(&ev.e[k]));
    SamWriter &wr = w;
    wr.th = std::thread([&wr] { wr.run(); });
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
    BHIP(hipEventRecord(ev.e[2], st));
    BHIP(launch_sam_size(bt, o, refs, d_off.p, d_bad, fl, st, keep));
    BHIP(scan.exclusive_scan(d_off.p, n + 1, st));
    BHIP(launch_sam_total(d_off.p, n, d_bad, static_cast<unsigned long long *>(hw.dev), st));
    BHIP(hipEventRecord(ev.e[3], st));
    BHIP(hipEventSynchronize(ev.e[3]));
    {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.e[2], ev.e[3]) == hipSuccess) format_ms += ms;
    }
    add_write_time();
    const unsigned long long *const h = static_cast<const unsigned long long *>(hw.h);
    const uint64_t bytes = h[0], bad = h[1];
    if (bad != ~0ull) {
        *bad_out = bad;
        return NGSQ_OK;
    }
    // the buffer of batch k - 2 is this batch's once its copies have completed
    const uint32_t slot = (uint32_t)(batches & 1);
    if (batches >= 2 && !w.wait_copied(batches - 1)) return NGSQ_OK;
    BHIP(d_text[slot].reserve(bytes + 1));
    BHIP(hipEventRecord(ev.e[4], st));
    BHIP(launch_sam_write(bt, o, refs, d_off.p, d_text[slot].p, fl, st, keep));
    BHIP(hipEventRecord(ev.e[5], st));
    BHIP(hipEventRecord(ev.e[slot], st));
    write_pending = true;
    w.push(SamJob{d_text[slot].p, bytes, ev.e[slot], batches});
    records += n;
    text_bytes += bytes;
    batches++;
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
    w.stop();
    if (rc == NGSQ_OK && w.herr != hipSuccess)
        rc = ngsq_bam_fail(NGSQ_ERR_DEVICE, "copying the SAM text to the host: %s", hipGetErrorString(w.herr));
    if (rc == NGSQ_OK && w.werr) rc = ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "%s: %s (os error %d)", context, strerror(w.werr), w.werr);
    if (rc != NGSQ_OK) (void)hipStreamSynchronize(st); // (the device buffers go back to the cache: nothing may still use them)
    return rc;
}

} // namespace ngsq
