// sam.cpp -- ngsq_bam_write_sam (include/ngsq_sam.h): the device ingest hands out the file's records batch by batch,
// sam_kernel.hip sizes every record's SAM line, the ingest's scan turns the sizes into offsets, and a second pass writes the
// lines into a device buffer of the batch's real size.  A writer thread copies the text of batch k to a pinned ring on a
// second stream (behind an event of the formatter) and writes the ring to the file in order, while the main thread ingests
// and formats batch k+1.  The host never walks the records.  DESIGN.md section 13.
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

#include "../../include/ngsq_sam.h"
#include "context.h"
#include "ingest_consumer.h"
#include "sam_kernels.h"

using namespace ngsq;

namespace {

constexpr uint64_t BATCH_RECORDS = (uint64_t)1 << 20;
constexpr uint32_t RING_SLOTS = 4;
constexpr size_t RING_PIECE = (size_t)32 << 20; // bytes per slot of the pinned ring

const char *sam_error_text(uint32_t code) {
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
int write_all(int fd, const char *p, size_t n) {
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
struct Job {
    const char *dev;
    uint64_t bytes;
    hipEvent_t ready;
    uint64_t batch;
};

// The writer thread: copies the jobs to the ring, RING_PIECE bytes per slot, and writes the slots to fd in order, keeping up
// to RING_SLOTS copies in flight while it writes.
struct Writer {
    int fd = -1, device = 0;
    hipStream_t cs = nullptr;
    char *ring = nullptr;
    hipEvent_t t0[RING_SLOTS] = {}, t1[RING_SLOTS] = {};
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    std::deque<Job> jobs;
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
            herr = hipHostMalloc(&h, RING_SLOTS * RING_PIECE, hipHostMallocDefault);
            ring = static_cast<char *>(h);
        }
        for (uint32_t s = 0; s < RING_SLOTS && herr == hipSuccess; s++) {
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
        Job cur{};
        uint64_t cur_off = 0;
        bool have = false;
        uint32_t next_slot = 0;
        for (;;) {
            // queue copies while a slot is free
            while (inflight.size() < RING_SLOTS) {
                if (!have) {
                    std::lock_guard<std::mutex> g(mu);
                    if (jobs.empty()) break;
                    cur = jobs.front();
                    jobs.pop_front();
                    cur_off = 0;
                    have = true;
                    if (herr == hipSuccess) herr = hipStreamWaitEvent(cs, cur.ready, 0);
                }
                const size_t len = (size_t)std::min<uint64_t>(RING_PIECE, cur.bytes - cur_off);
                const uint32_t s = next_slot;
                next_slot = (next_slot + 1) % RING_SLOTS;
                if (herr == hipSuccess && len) {
                    herr = hipEventRecord(t0[s], cs);
                    if (herr == hipSuccess) herr = hipMemcpyAsync(ring + (size_t)s * RING_PIECE, cur.dev + cur_off, len, hipMemcpyDeviceToHost, cs);
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
                werr = write_all(fd, ring + (size_t)pc.slot * RING_PIECE, pc.len);
                write_ms += now_ms() - w0;
            }
        }
    }
    void push(const Job &j) {
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
    ~Writer() {
        stop();
        if (cs) {
            (void)hipStreamSynchronize(cs);
            pool_stream_put(false, cs);
        }
        for (uint32_t s = 0; s < RING_SLOTS; s++) {
            if (t0[s]) (void)hipEventDestroy(t0[s]);
            if (t1[s]) (void)hipEventDestroy(t1[s]);
        }
        if (ring) (void)hipHostFree(ring);
    }
};

struct Events {
    hipEvent_t e[6] = {};
    ~Events() {
        for (auto x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

// What the batches of one ngsq_bam_write_sam share.
struct SamRun {
    ngsq_bam *b;
    ngsq_ctx *c;
    hipStream_t st = nullptr;
    uint64_t max_records, batch_records;
    // the @SQ names on the device, the error word, the words the host reads
    DevArray<uint64_t> d_setup;
    unsigned long long *d_bad = nullptr;
    SamRefs refs;
    MappedBuf hw;
    // the writer: a copy stream, the pinned ring, its thread
    Writer w;
    Events ev; // ready[2]; format brackets: size a/b, write a/b
    DevArray<uint64_t> d_off, d_flist;
    DevArray<uint8_t> d_fmark;
    ScanScratch scan;
    DevArray<char> d_text[2];
    uint64_t records = 0, text_bytes = 0, batches = 0;
    double scan_ms = 0, format_ms = 0;
    bool write_pending = false; // the last write pass's bracket has not been added to format_ms yet

    void add_write_time() {
        float ms = 0;
        if (write_pending && hipEventElapsedTime(&ms, ev.e[4], ev.e[5]) == hipSuccess) format_ms += ms;
        write_pending = false;
    }
    int next_batch(bool *more);
};

// One batch of the device ingest, in file order: sized, scanned, written into a device buffer and handed to the writer.
// *more = false: that was the last one (the file's end, max_records, or a writer that has failed: its error is read at the end).
int SamRun::next_batch(bool *more) {
    *more = false;
    const uint64_t left = max_records ? max_records - records : ~0ull;
    if (!left) return NGSQ_OK;
    ngsq_batch bt;
    BatchOrigin o;
    const double s0 = now_ms();
    const int rc = next_batch_with_origin(b, c, std::min(batch_records, left), &bt, &o);
    scan_ms += now_ms() - s0;
    if (rc) return rc;
    const uint64_t n = bt.n_records;
    if (!n) return NGSQ_OK;
    BHIP(d_off.reserve(n + 1));
    BHIP(d_fmark.reserve(n));
    BHIP(d_flist.reserve(n + 1));
    const SamFloats fl{d_fmark.p, d_flist.p + 1, reinterpret_cast<unsigned long long *>(d_flist.p)};
    // sizes, offsets, and the batch's text bytes and error word to the host
    BHIP(hipEventRecord(ev.e[2], st));
    BHIP(launch_sam_size(bt, o, refs, d_off.p, d_bad, fl, st));
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
    if (bad != ~0ull)
        return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "writing SAM record: record %llu: %s", (unsigned long long)(bad >> SAM_ERR_BITS),
                             sam_error_text((uint32_t)(bad & ((1u << SAM_ERR_BITS) - 1))));
    // the buffer of batch k - 2 is this batch's once its copies have completed
    const uint32_t slot = (uint32_t)(batches & 1);
    if (batches >= 2 && !w.wait_copied(batches - 1)) return NGSQ_OK;
    BHIP(d_text[slot].reserve(bytes + 1));
    BHIP(hipEventRecord(ev.e[4], st));
    BHIP(launch_sam_write(bt, o, refs, d_off.p, d_text[slot].p, fl, st));
    BHIP(hipEventRecord(ev.e[5], st));
    BHIP(hipEventRecord(ev.e[slot], st));
    write_pending = true;
    w.push(Job{d_text[slot].p, bytes, ev.e[slot], batches});
    records += n;
    text_bytes += bytes;
    batches++;
    *more = !w.werr;
    return NGSQ_OK;
}

} // namespace

extern "C" int ngsq_bam_write_sam(ngsq_bam *b, ngsq_ctx *c, int fd, uint64_t max_records, uint64_t batch_records, ngsq_sam_report *out) {
    if (!b || !c || fd < 0) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    if (out) memset(out, 0, sizeof *out);
    if (const int rc = require_fresh_reader(b, "a SAM file is written")) return rc;
    const double t_begin = now_ms();
    // ---- the header: the text the file holds, with a final newline
    std::string head = b->header_text;
    if (!head.empty() && head.back() != '\n') head += '\n';
    if (const int e = write_all(fd, head.data(), head.size()))
        return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "writing SAM header: %s (os error %d)", strerror(e), e);
    BHIP(hipSetDevice(c->device));
    SamRun r;
    r.b = b;
    r.c = c;
    r.st = c->stream;
    r.max_records = max_records;
    r.batch_records = batch_records ? batch_records : BATCH_RECORDS;
    const uint32_t n_refs = (uint32_t)b->ref_names.size();
    std::vector<uint64_t> setup(n_refs + 2, 0); // [bad | name_off[n_refs + 1]] then the names
    std::string names;
    for (uint32_t k = 0; k < n_refs; k++) {
        setup[1 + k] = names.size();
        names += b->ref_names[k];
    }
    setup[1 + n_refs] = names.size();
    setup[0] = ~0ull;
    BHIP(r.d_setup.reserve(setup.size() + (names.size() + 7) / 8));
    BHIP(hipMemcpyAsync(r.d_setup.p, setup.data(), setup.size() * sizeof(uint64_t), hipMemcpyHostToDevice, r.st));
    if (!names.empty()) BHIP(hipMemcpyAsync(r.d_setup.p + setup.size(), names.data(), names.size(), hipMemcpyHostToDevice, r.st));
    r.d_bad = reinterpret_cast<unsigned long long *>(r.d_setup.p);
    r.refs.names = reinterpret_cast<const char *>(r.d_setup.p + setup.size());
    r.refs.name_off = r.d_setup.p + 1;
    r.refs.n_refs = n_refs;
    BHIP(r.hw.reserve(8 * sizeof(unsigned long long)));
    memset(r.hw.h, 0, 8 * sizeof(unsigned long long));
    r.w.fd = fd;
    r.w.device = c->device;
    BHIP(pool_stream_get(false, &r.w.cs));
    BHIP(hipEventCreateWithFlags(&r.ev.e[0], hipEventDisableTiming));
    BHIP(hipEventCreateWithFlags(&r.ev.e[1], hipEventDisableTiming));
    for (int k = 2; k < 6; k++) BHIP(hipEventCreate(&r.ev.e[k]));
    Writer &w = r.w;
    w.th = std::thread([&w] { w.run(); });
    { // the per-record arrays for the largest batch asked for: a batch's write pass may still read them when the next one begins
        const uint64_t n0 = std::min<uint64_t>(r.batch_records, max_records ? max_records : r.batch_records);
        if (r.d_off.reserve(n0 + 1) != hipSuccess || r.d_fmark.reserve(n0) != hipSuccess || r.d_flist.reserve(n0 + 1) != hipSuccess)
            return ngsq_bam_fail(NGSQ_ERR_DEVICE, "allocating the SAM formatter's arrays for %llu records", (unsigned long long)n0);
    }
    // ---- the scan: every batch of the device ingest, in file order
    int rc = NGSQ_OK;
    for (bool more = true; more && rc == NGSQ_OK;) rc = r.next_batch(&more);
    if (rc == NGSQ_OK) {
        const hipError_t e = hipStreamSynchronize(r.st);
        if (e != hipSuccess) rc = ngsq_bam_fail(NGSQ_ERR_DEVICE, "hipStreamSynchronize: %s", hipGetErrorString(e));
        r.add_write_time();
    }
    w.stop(); // (every queued copy is written, or skipped after a failed write)
    if (rc == NGSQ_OK && w.herr != hipSuccess)
        rc = ngsq_bam_fail(NGSQ_ERR_DEVICE, "copying the SAM text to the host: %s", hipGetErrorString(w.herr));
    if (rc == NGSQ_OK && w.werr) rc = ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "writing SAM record: %s (os error %d)", strerror(w.werr), w.werr);
    if (rc != NGSQ_OK) {
        (void)hipStreamSynchronize(r.st); // (the device buffers go back to the cache: nothing may still use them)
        return rc;
    }
    if (out) {
        out->records = r.records;
        out->header_bytes = head.size();
        out->text_bytes = r.text_bytes;
        out->batches = r.batches;
        out->scan_ms = r.scan_ms;
        out->format_ms = r.format_ms;
        out->copy_ms = w.copy_ms;
        out->write_ms = w.write_ms;
        out->total_ms = now_ms() - t_begin;
    }
    return NGSQ_OK;
}
