// device_out.h -- the output stage the commands that write a file share: a batch of output bytes
// lies in a device buffer, and a writer thread copies it through a pinned ring to a file descriptor while the main thread
// produces the next batch.  `ngs convert` and `ngs view` hand it SAM text (sam_run.h), `ngs generate` FASTQ text or BGZF blocks,
// one writer per file (generate.cpp).  The three commands that write one BAM file through the device encoder (samtext.cpp,
// and samsort.cpp and bamsort.cpp through sort_resident.h) share BgzfSink at the end of this file: encoder, slots, writer and
// the EOF block.  Nothing above it knows what the bytes are.
#pragma once

#include <hip/hip_runtime_api.h>
#include <errno.h>
#include <unistd.h>

#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <mutex>
#include <thread>

#include "context.h"
#include "deflate_kernels.h"
#include "mem_pool.h"

namespace ngsq {

constexpr uint32_t RING_SLOTS = 4;
constexpr size_t RING_PIECE = (size_t)32 << 20; // bytes per slot of the pinned ring

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

// the EOF block a BGZF file ends with; 0 or errno
inline int write_bgzf_eof(int fd) { return write_all(fd, reinterpret_cast<const char *>(BGZF_EOF_BLOCK), sizeof BGZF_EOF_BLOCK); }

// N events, destroyed with the array (those that were created)
template <int N> struct HipEvents {
    hipEvent_t e[N] = {};
    ~HipEvents() {
        for (auto x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

// The drain rule: every way out of its scope waits for the stream first.  Declare it behind the arrays the stream's kernels and
// copies use, so that it is destroyed before them: they go back to the block cache (or the heap) when they leave scope, and
// nothing queued may still use them.  Without a stream (an early return) it does nothing.  pooled: the stream came from
// pool_stream_get and goes back there, idle.
struct StreamDrain {
    hipStream_t s = nullptr;
    bool pooled = false;
    ~StreamDrain() {
        if (s) (void)hipStreamSynchronize(s);
        if (s && pooled) pool_stream_put(false, s);
    }
};

// The bytes of one job, as the main thread hands them to the writer: copy them once `ready` has completed on the copy stream.
struct DeviceJob {
    const char *dev;
    uint64_t bytes;
    hipEvent_t ready;
    uint64_t batch;
};

// How a writer ended: a failed copy (herr) comes before a failed write (werr, an errno).  Each command has its own words for them.
struct WriterEnd {
    hipError_t herr;
    int werr;
};

// The writer thread: copies the jobs to the ring, RING_PIECE bytes per slot, and writes the slots to fd in order, keeping up to
// RING_SLOTS copies in flight while it writes.
struct DeviceWriter {
    int fd = -1, device = 0;
    hipStream_t cs = nullptr;
    char *ring = nullptr;
    HipEvents<RING_SLOTS> t0, t1; // around the copy into a slot
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    std::deque<DeviceJob> jobs;
    bool finish = false;
    uint64_t batches_copied = 0; // batches whose every copy has completed (their device buffer may be reused)
    int werr = 0;                // errno of a failed write: nothing more is written
    hipError_t herr = hipSuccess;
    double copy_ms = 0, write_ms = 0;
    std::thread th;

    // the copy stream from the pool, then the thread: it writes to fd_ what it copies from device_
    hipError_t start(int fd_, int device_) {
        fd = fd_, device = device_;
        const hipError_t e = pool_stream_get(false, &cs);
        if (e == hipSuccess) th = std::thread([this] { run(); });
        return e;
    }
    void run() {
        // the ring is pinned here, beside the first batch's ingest and formatting (some 25 ms for 128 MiB)
        herr = hipSetDevice(device);
        if (herr == hipSuccess) {
            void *h = nullptr;
            herr = hipHostMalloc(&h, RING_SLOTS * RING_PIECE, hipHostMallocDefault);
            ring = static_cast<char *>(h);
        }
        for (uint32_t s = 0; s < RING_SLOTS && herr == hipSuccess; s++) {
            herr = hipEventCreate(&t0.e[s]);
            if (herr == hipSuccess) herr = hipEventCreate(&t1.e[s]);
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
        DeviceJob cur{};
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
                    herr = hipEventRecord(t0.e[s], cs);
                    if (herr == hipSuccess) herr = hipMemcpyAsync(ring + (size_t)s * RING_PIECE, cur.dev + cur_off, len, hipMemcpyDeviceToHost, cs);
                    if (herr == hipSuccess) herr = hipEventRecord(t1.e[s], cs);
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
                herr = hipEventSynchronize(t1.e[pc.slot]);
                float ms = 0;
                if (herr == hipSuccess && hipEventElapsedTime(&ms, t0.e[pc.slot], t1.e[pc.slot]) == hipSuccess) copy_ms += ms;
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
    void push(const DeviceJob &j) {
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
    // true: nothing more can be written (its error is read at the end of the run)
    bool failed() const { return werr || herr != hipSuccess; }
    // The end of a run: every queued copy is written (or skipped after a failed write), the thread joined.
    WriterEnd end() {
        if (th.joinable()) {
            {
                std::lock_guard<std::mutex> g(mu);
                finish = true;
            }
            cv_work.notify_one();
            th.join();
        }
        return WriterEnd{herr, werr};
    }
    ~DeviceWriter() {
        (void)end();
        if (cs) {
            (void)hipStreamSynchronize(cs);
            pool_stream_put(false, cs);
        }
        if (ring) (void)hipHostFree(ring);
    }
};

// The two-slot rule.  Job k's device buffers are those of slot k & 1: the ones job k - 2 was copied from, free once the
// writers have copied that job.  acquire, launch what fills the buffers of slot(), submit.  The buffers stay with their
// owners (a formatter's text per file, an encoder's blocks); the writers of a run (one per file) share the counter and the events.
struct JobSlots {
    HipEvents<2> ready; // no timing
    uint64_t jobs = 0;

    hipError_t create() {
        const hipError_t e = hipEventCreateWithFlags(&ready.e[0], hipEventDisableTiming);
        return e != hipSuccess ? e : hipEventCreateWithFlags(&ready.e[1], hipEventDisableTiming);
    }
    uint32_t slot() const { return (uint32_t)(jobs & 1); }
    // wait until w[0, n) have copied job k - 2; false: a copy failed (the writer's error is read at the end of the run)
    bool acquire(DeviceWriter *w, uint32_t n = 1) {
        for (uint32_t k = 0; k < n; k++)
            if (jobs >= 2 && !w[k].wait_copied(jobs - 1)) return false;
        return true;
    }
    // what has been queued on st so far fills the job: w[k] copies bytes[k] from src[k] behind it
    hipError_t submit(DeviceWriter *w, uint32_t n, const char *const *src, const uint64_t *bytes, hipStream_t st) {
        const hipEvent_t ev = ready.e[slot()];
        const hipError_t e = hipEventRecord(ev, st);
        if (e != hipSuccess) return e;
        for (uint32_t k = 0; k < n; k++) w[k].push(DeviceJob{src[k], bytes[k], ev, jobs});
        jobs++;
        return hipSuccess;
    }
    hipError_t submit(DeviceWriter &w, const char *src, uint64_t bytes, hipStream_t st) { return submit(&w, 1, &src, &bytes, st); }
};

// The encoder step of a BGZF file: a job's bytes become blocks in the slot's buffer.  launch() queues the encoder; collect()
// reads its words once the caller has waited for it, so that a caller launches, does other work (the encoder of a second
// file, the next chunk's read), waits once and collects.
struct BgzfEncoder {
    DeflateScratch sc;
    const unsigned long long *h = nullptr; // DEFLATE_HOST_WORDS words of the caller's MappedBuf, which the last kernel writes
    unsigned long long *hdev = nullptr;    // (the same words as the device addresses them)
    DevArray<uint8_t> d_comp[2];
    uint64_t comp_bytes = 0, blocks = 0, stored = 0;
    uint32_t effort = DEFLATE_EFFORT_NORMAL; // the context's (ngsq_bgzf_set_effort), set by whoever starts the encoder

    // src[0, bytes) (device, DEFLATE_IN_SLACK readable bytes behind it) into the buffer of `slot`
    hipError_t launch(uint32_t slot, const void *src, uint64_t bytes, hipStream_t st) {
        const hipError_t e = d_comp[slot].reserve(deflate_bound(bytes));
        if (e != hipSuccess) return e;
        return launch_bgzf_deflate(static_cast<const uint8_t *>(src), bytes, d_comp[slot].p, sc, hdev, effort, st);
    }
    // The blocks of the launch the caller has waited for: where they lie and how many bytes they are.  nullptr, or what is
    // wrong with them.
    const char *collect(uint32_t slot, uint64_t bytes, const char **dev, uint64_t *out_bytes) {
        if (h[DH_BYTES] > deflate_bound(bytes)) return "the encoder wrote more than its bound";
        *dev = reinterpret_cast<const char *>(d_comp[slot].p);
        *out_bytes = h[DH_BYTES];
        comp_bytes += h[DH_BYTES];
        blocks += deflate_blocks(bytes);
        stored += h[DH_STORED];
        return nullptr;
    }
};

// One BGZF file through the device encoder: the encoder with the words the host reads of it, the two slots of its block buffers,
// the writer, the EOF block.  Per job: acquire() (waits until job k - 2 has been copied), fill the source, launch(), other
// work, hand_over() (waits for the encoder).  The three stay apart so that each caller keeps its waits where its overlap
// needs them.  A failure leaves its code and its message here; the caller reports it through its own channel.  The sink
// drains nothing: whoever owns it drains the stream of launch() before the sink goes (the drain rule above).
struct BgzfSink {
    BgzfEncoder enc;
    JobSlots slots;
    MappedBuf hw;      // the encoder's words
    HipEvents<1> done; // behind the encoder of the job in flight
    hipStream_t st = nullptr;
    DeviceWriter w; // (behind the encoder's buffers: it ends, and its copies with it, before they go)
    uint64_t bam_bytes = 0; // the bytes handed over, before compression
    double deflate_ms = 0;
    int code = 0;
    std::string err;

    int fail(int code_, const std::string &m) {
        err = m;
        return code = code_;
    }
    int copy_failed(hipError_t e) { return fail(NGSQ_ERR_DEVICE, std::string("copying the BGZF blocks to the host: ") + hipGetErrorString(e)); }
    int write_failed(int e) { return fail(NGSQ_ERR_INVALID_ARGUMENT, std::string("writing BAM record: ") + strerror(e) + " (os error " + std::to_string(e) + ")"); }
#define ZHIP(expr)                                                                                              \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) return fail(NGSQ_ERR_DEVICE, std::string(#expr ": ") + hipGetErrorString(e_)); \
    } while (0)
    // the words, the events, and the writer of fd on `device` (made current); effort: the context's, for every launch
    int start(int fd, int device, uint32_t effort) {
        enc.effort = effort;
        ZHIP(hipSetDevice(device));
        ZHIP(hw.reserve(DEFLATE_HOST_WORDS * sizeof(unsigned long long)));
        memset(hw.h, 0, DEFLATE_HOST_WORDS * sizeof(unsigned long long));
        enc.h = static_cast<const unsigned long long *>(hw.h);
        enc.hdev = static_cast<unsigned long long *>(hw.dev);
        ZHIP(hipEventCreate(&done.e[0]));
        ZHIP(slots.create());
        ZHIP(w.start(fd, device));
        return NGSQ_OK;
    }
    int acquire() { return slots.acquire(&w) ? NGSQ_OK : copy_failed(w.herr); }
    // src[0, bytes) (device, DEFLATE_IN_SLACK readable bytes behind it) through the encoder into the buffer of the job's slot
    int launch(const void *src, uint64_t bytes, hipStream_t stream) {
        st = stream;
        ZHIP(enc.launch(slots.slot(), src, bytes, st));
        ZHIP(hipEventRecord(done.e[0], st));
        return NGSQ_OK;
    }
    // The blocks of the job launched go to the writer once the encoder has ended; its time counts from `since`.  file_at
    // (optional): where the job's first block lies in the file.
    int hand_over(uint64_t bytes, hipEvent_t since, uint64_t *file_at = nullptr) {
        ZHIP(hipEventSynchronize(done.e[0]));
        if (file_at) *file_at = enc.comp_bytes;
        const char *blocks = nullptr;
        uint64_t n = 0;
        if (const char *m = enc.collect(slots.slot(), bytes, &blocks, &n)) return fail(NGSQ_ERR_STATE, m);
        float ms = 0;
        if (hipEventElapsedTime(&ms, since, done.e[0]) == hipSuccess) deflate_ms += ms;
        // (nothing may be queued on st between launch and here: `ready` would cover it and hold the copy back)
        ZHIP(slots.submit(w, blocks, n, st));
        bam_bytes += bytes;
        return NGSQ_OK;
    }
#undef ZHIP
    // The writer ended: every job written, or skipped after a failed write.  Its errors are reported when nothing failed before
    // them (rc), a failed copy before a failed write.
    int stop(int rc) {
        const WriterEnd end = w.end();
        if (rc == NGSQ_OK && end.herr != hipSuccess) rc = copy_failed(end.herr);
        if (rc == NGSQ_OK && end.werr) rc = write_failed(end.werr);
        return rc;
    }
    // stop(), then the EOF block behind a file that is whole
    int end(int rc, int fd) {
        rc = stop(rc);
        if (rc == NGSQ_OK) {
            if (const int e = write_bgzf_eof(fd)) rc = write_failed(e);
            enc.comp_bytes += sizeof BGZF_EOF_BLOCK;
        }
        return rc;
    }
};

} // namespace ngsq
