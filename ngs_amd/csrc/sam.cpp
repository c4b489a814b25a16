// sam.cpp -- ngsq_bam_write_sam (include/ngsq_sam.h): the device ingest hands out the file's records batch by batch,
// sam_kernel.hip sizes every record's SAM line, the ingest's scan turns the sizes into offsets, and a second pass writes the
// lines into a device buffer of the batch's real size.  A writer thread copies the text of batch k to a pinned ring on a
// second stream (behind an event of the formatter) and writes the ring to the file in order, while the main thread ingests
// and formats batch k+1.  The host never walks the records.  DESIGN.md section 13.
#include <hip/hip_runtime_api.h>
#include <errno.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ngsq_sam.h"
#include "bam_reader.h"
#include "context.h"
#include "mem_pool.h"
#include "sam_kernels.h"

using namespace ngsq;

namespace {

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// a device array from the process's block cache, grown without keeping its contents
template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t cap = 0, bytes = 0;
    hipError_t reserve(size_t n) {
        if (n <= cap) return hipSuccess;
        const size_t want = std::max(n + 64, cap + cap / 2);
        void *q = nullptr;
        size_t got = 0;
        const hipError_t e = pool_device_alloc(&q, want * sizeof(T), &got);
        if (e != hipSuccess) return e;
        pool_device_free(p, bytes);
        p = static_cast<T *>(q);
        cap = got / sizeof(T);
        bytes = got;
        return hipSuccess;
    }
    ~DevBuf() { pool_device_free(p, bytes); }
};

#define SHIP(expr)                                                                                           \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) return ngsq_bam_fail(NGSQ_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

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

} // namespace

extern "C" int ngsq_bam_write_sam(ngsq_bam *b, ngsq_ctx *c, int fd, uint64_t max_records, uint64_t batch_records, ngsq_sam_report *out) {
    if (!b || !c || fd < 0) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    if (out) memset(out, 0, sizeof *out);
    if (b->dev || b->host_mode || b->n_read)
        return ngsq_bam_fail(NGSQ_ERR_STATE, "%s: a SAM file is written from a reader no record has been read from", b->path.c_str());
    const double t_begin = now_ms();
    if (!batch_records) batch_records = BATCH_RECORDS;
    // ---- the header: the text the file holds, with a final newline
    std::string head = b->header_text;
    if (!head.empty() && head.back() != '\n') head += '\n';
    if (const int e = write_all(fd, head.data(), head.size()))
        return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "writing SAM header: %s (os error %d)", strerror(e), e);
    SHIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    // ---- the @SQ names on the device, the error word, the words the host reads
    const uint32_t n_refs = (uint32_t)b->ref_names.size();
    std::vector<uint64_t> setup(n_refs + 2, 0); // [bad | name_off[n_refs + 1]] then the names
    std::string names;
    for (uint32_t r = 0; r < n_refs; r++) {
        setup[1 + r] = names.size();
        names += b->ref_names[r];
    }
    setup[1 + n_refs] = names.size();
    setup[0] = ~0ull;
    DevBuf<uint64_t> d_setup;
    SHIP(d_setup.reserve(setup.size() + (names.size() + 7) / 8));
    SHIP(hipMemcpyAsync(d_setup.p, setup.data(), setup.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (!names.empty()) SHIP(hipMemcpyAsync(d_setup.p + setup.size(), names.data(), names.size(), hipMemcpyHostToDevice, st));
    unsigned long long *const d_bad = reinterpret_cast<unsigned long long *>(d_setup.p);
    SamRefs refs;
    refs.names = reinterpret_cast<const char *>(d_setup.p + setup.size());
    refs.name_off = d_setup.p + 1;
    refs.n_refs = n_refs;
    struct HostWords {
        unsigned long long *h = nullptr;
        ~HostWords() {
            if (h) (void)hipHostFree(h);
        }
    } hw;
    unsigned long long *h_dev = nullptr;
    {
        void *h = nullptr, *dv = nullptr;
        SHIP(hipHostMalloc(&h, 8 * sizeof(unsigned long long), hipHostMallocMapped));
        hw.h = static_cast<unsigned long long *>(h);
        memset(hw.h, 0, 8 * sizeof(unsigned long long));
        SHIP(hipHostGetDevicePointer(&dv, h, 0));
        h_dev = static_cast<unsigned long long *>(dv);
    }
    // ---- the writer: a copy stream, the pinned ring, its thread
    Writer w;
    w.fd = fd;
    w.device = c->device;
    SHIP(pool_stream_get(false, &w.cs));
    Events ev; // ready[2]; format brackets: size a/b, write a/b
    SHIP(hipEventCreateWithFlags(&ev.e[0], hipEventDisableTiming));
    SHIP(hipEventCreateWithFlags(&ev.e[1], hipEventDisableTiming));
    for (int k = 2; k < 6; k++) SHIP(hipEventCreate(&ev.e[k]));
    w.th = std::thread([&w] { w.run(); });
    DevBuf<uint64_t> d_off, d_scan, d_flist;
    DevBuf<uint8_t> d_fmark;
    { // the per-record arrays for the largest batch asked for: a batch's write pass may still read them when the next one begins
        const uint64_t n0 = std::min<uint64_t>(batch_records, max_records ? max_records : batch_records);
        if (d_off.reserve(n0 + 1) != hipSuccess || d_fmark.reserve(n0) != hipSuccess || d_flist.reserve(n0 + 1) != hipSuccess)
            return ngsq_bam_fail(NGSQ_ERR_DEVICE, "allocating the SAM formatter's arrays for %llu records", (unsigned long long)n0);
    }
    DevBuf<char> d_text[2];
    // ---- the scan: every batch of the device ingest, in file order
    uint64_t records = 0, text_bytes = 0, batches = 0;
    double scan_ms = 0, format_ms = 0;
    bool write_pending = false; // the last write pass's bracket has not been added to format_ms yet
    int rc = NGSQ_OK;
    auto add_write_time = [&]() {
        float ms = 0;
        if (write_pending && hipEventElapsedTime(&ms, ev.e[4], ev.e[5]) == hipSuccess) format_ms += ms;
        write_pending = false;
    };
    for (;;) {
        const uint64_t left = max_records ? max_records - records : ~0ull;
        if (!left) break;
        ngsq_batch bt;
        const double s0 = now_ms();
        rc = ngsq_bam_next_batch_device(b, c, std::min(batch_records, left), &bt);
        scan_ms += now_ms() - s0;
        if (rc) break;
        const uint64_t n = bt.n_records;
        if (!n) break;
        BatchOrigin o;
        if ((rc = bam_device_batch_origin(b, &o))) break;
        size_t tmp_bytes = 0;
#define SFAIL(expr)                                                                                  \
    {                                                                                                \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            rc = ngsq_bam_fail(NGSQ_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_));             \
            break;                                                                                   \
        }                                                                                            \
    }
        SFAIL(d_off.reserve(n + 1));
        SFAIL(d_fmark.reserve(n));
        SFAIL(d_flist.reserve(n + 1));
        const SamFloats fl{d_fmark.p, d_flist.p + 1, reinterpret_cast<unsigned long long *>(d_flist.p)};
        SFAIL(launch_exclusive_scan_u64(d_off.p, n + 1, nullptr, &tmp_bytes, st));
        SFAIL(d_scan.reserve(tmp_bytes / sizeof(uint64_t) + 1));
        tmp_bytes = d_scan.cap * sizeof(uint64_t);
        // sizes, offsets, and the batch's text bytes and error word to the host
        SFAIL(hipEventRecord(ev.e[2], st));
        SFAIL(launch_sam_size(bt, o, refs, d_off.p, d_bad, fl, st));
        SFAIL(launch_exclusive_scan_u64(d_off.p, n + 1, d_scan.p, &tmp_bytes, st));
        SFAIL(launch_sam_total(d_off.p, n, d_bad, h_dev, st));
        SFAIL(hipEventRecord(ev.e[3], st));
        SFAIL(hipEventSynchronize(ev.e[3]));
        {
            float ms = 0;
            if (hipEventElapsedTime(&ms, ev.e[2], ev.e[3]) == hipSuccess) format_ms += ms;
        }
        add_write_time();
        const uint64_t bytes = hw.h[0], bad = hw.h[1];
        if (bad != ~0ull) {
            rc = ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "writing SAM record: record %llu: %s", (unsigned long long)(bad >> SAM_ERR_BITS),
                               sam_error_text((uint32_t)(bad & ((1u << SAM_ERR_BITS) - 1))));
            break;
        }
        // the buffer of batch k - 2 is this batch's once its copies have completed
        const uint32_t slot = (uint32_t)(batches & 1);
        if (batches >= 2 && !w.wait_copied(batches - 1)) break;
        SFAIL(d_text[slot].reserve(bytes + 1));
        SFAIL(hipEventRecord(ev.e[4], st));
        SFAIL(launch_sam_write(bt, o, refs, d_off.p, d_text[slot].p, fl, st));
        SFAIL(hipEventRecord(ev.e[5], st));
        SFAIL(hipEventRecord(ev.e[slot], st));
        write_pending = true;
        w.push(Job{d_text[slot].p, bytes, ev.e[slot], batches});
        records += n;
        text_bytes += bytes;
        batches++;
        if (w.werr) break;
    }
#undef SFAIL
    if (rc == NGSQ_OK) {
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = ngsq_bam_fail(NGSQ_ERR_DEVICE, "hipStreamSynchronize: %s", hipGetErrorString(e));
        add_write_time();
    }
    w.stop(); // (every queued copy is written, or skipped after a failed write)
    if (rc == NGSQ_OK && w.herr != hipSuccess)
        rc = ngsq_bam_fail(NGSQ_ERR_DEVICE, "copying the SAM text to the host: %s", hipGetErrorString(w.herr));
    if (rc == NGSQ_OK && w.werr) rc = ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "writing SAM record: %s (os error %d)", strerror(w.werr), w.werr);
    if (rc != NGSQ_OK) {
        (void)hipStreamSynchronize(st); // (the device buffers go back to the cache: nothing may still use them)
        return rc;
    }
    if (out) {
        out->records = records;
        out->header_bytes = head.size();
        out->text_bytes = text_bytes;
        out->batches = batches;
        out->scan_ms = scan_ms;
        out->format_ms = format_ms;
        out->copy_ms = w.copy_ms;
        out->write_ms = w.write_ms;
        out->total_ms = now_ms() - t_begin;
    }
    return NGSQ_OK;
}
