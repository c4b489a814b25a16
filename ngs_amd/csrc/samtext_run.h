// samtext_run.h -- the chunk pipeline of SAM text, which the two drivers of SAM to BAM share: samtext.cpp
// (records compressed as they are parsed) and samsort.cpp (records resident until their order is known).  The counterpart of
// sam_run.h for the other direction.  The host reads the header and then only moves bytes: the text goes in chunks that end on
// a newline through two pinned buffers to the device on a second stream, samtext_kernel.hip finds the lines, sizes their
// records and writes them where the driver says.  While chunk k is written (and whatever the driver does with it) the host reads
// chunk k + 1 and copies it up.  Per chunk the host reads four words: lines, record bytes, error word, text bytes.
//
// A driver's loop:  open, begin;  while (len) { size; stop if faulty(); write(dst); advance; }  end; verdict.
#pragma once

#include "samtext_host.h"

namespace ngsq {

struct SamTextRun {
    enum Ev { EV_UP0 = 0, EV_UP1, EV_H0, EV_H1, EV_P0, EV_P1, EV_W0, EV_W1, EV_N };
    enum HostWord : uint32_t { HW_LINES = 0, HW_BYTES, HW_BAD, HW_TEXT, HW_WORDS }; // (launch_samtext_total writes HW_BYTES and HW_BAD: adjacent)

    ngsq_ctx *c = nullptr;
    hipStream_t st = nullptr, up = nullptr; // the context's stream; the copy stream of the text, from the pool
    uint64_t max_records = 0, chunk_bytes = 0;
    Fd in;
    SamHeader H;
    RefTable rt;
    DevArray<uint64_t> d_setup, d_tiles, d_start, d_off, d_flist;
    DevArray<uint8_t> d_fmark, d_text[2];
    unsigned long long *d_bad = nullptr;
    SamTextRefs refs{};
    SamTextFloats fl{};
    ScanScratch scan;
    MappedBuf hw;
    TextChunks text;
    HipEvents<EV_N> ev;
    uint64_t records = 0, text_bytes = 0, chunks = 0, bad = ~0ull;
    double h2d_ms = 0, parse_ms = 0;
    bool write_pending = false;         // the last write bracket has not been added to parse_ms yet
    uint64_t len = 0, n = 0, bytes = 0; // the current chunk: its text (0: none is left), and once sized its records and their bytes
    // The drain rule (device_out.h), behind everything above: both streams are idle before the arrays, the words and the pinned
    // text go.  A driver's own arrays are used on `st` as well, so it declares them in front of this object (or drains `st` itself,
    // as SortResident does): this drain then runs before they go, too.
    StreamDrain drain, drain_up{nullptr, true};

#define STHIP(expr)                                                                                     \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return sfail(c, NGSQ_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
    const unsigned long long *h() const { return static_cast<const unsigned long long *>(hw.h); }
    unsigned long long *hdev() const { return static_cast<unsigned long long *>(hw.dev); }
    void elapsed(int a, int b, double *sum) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.e[a], ev.e[b]) == hipSuccess) *sum += ms;
    }
    void add_write_time() {
        if (write_pending) elapsed(EV_W0, EV_W1, &parse_ms);
        write_pending = false;
    }

    // host only: the file and its header
    int open(ngsq_ctx *ctx, const char *sam_path, uint64_t max_records_, uint64_t chunk_bytes_) {
        c = ctx;
        max_records = max_records_;
        chunk_bytes = std::min(chunk_bytes_ ? chunk_bytes_ : ST_CHUNK_DEFAULT, ST_CHUNK_MAX);
        in.fd = ::open(sam_path, O_RDONLY | O_CLOEXEC);
        if (in.fd < 0) {
            const int e = errno;
            return sfail(c, NGSQ_ERR_INVALID_ARGUMENT, "%s%s (os error %d)", ST_OPEN_CTX, strerror(e), e);
        }
        const std::string m = read_header(in.fd, &H);
        if (!m.empty()) return sfail(c, NGSQ_ERR_INVALID_ARGUMENT, "%s%s", ST_OPEN_CTX, m.c_str());
        return NGSQ_OK;
    }
    // the device side: the streams, the reference table, the words, the events, and the first chunk on its way up
    int begin() {
        STHIP(hipSetDevice(c->device));
        st = drain.s = c->stream;
        STHIP(pool_stream_get(false, &up));
        drain_up.s = up;
        rt = RefTable(H);
        STHIP(d_setup.reserve(rt.device_words()));
        STHIP(rt.upload(d_setup.p, st));
        STHIP(hipStreamSynchronize(st));
        d_bad = rt.bad(d_setup.p);
        refs = rt.refs(d_setup.p);
        STHIP(hw.reserve(HW_WORDS * sizeof(unsigned long long)));
        memset(hw.h, 0, HW_WORDS * sizeof(unsigned long long));
        STHIP(text.start(in.fd, chunk_bytes, H.body_at));
        for (int k = 0; k < EV_N; k++) {
            if (k == EV_UP0 || k == EV_UP1) STHIP(hipEventCreateWithFlags(&ev.e[k], hipEventDisableTiming));
            else STHIP(hipEventCreate(&ev.e[k]));
        }
        return next(0);
    }
    // The next chunk into the text's buffer `slot`, len bytes that end on a newline (0: the file has ended), and from there to
    // d_text[slot] on the copy stream; the carry moves to the other buffer first (the copy only reads).
    int next(uint32_t slot) {
        if (const int e = text.fill(slot, &len)) return sfail(c, NGSQ_ERR_INVALID_ARGUMENT, "reading SAM record: %s (os error %d)", strerror(e), e);
        if (!len) return NGSQ_OK;
        text.move_carry(slot, len);
        STHIP(d_text[slot].reserve(len + ST_TEXT_SLACK));
        STHIP(hipEventRecord(ev.e[EV_H0], up));
        STHIP(hipMemcpyAsync(d_text[slot].p, text.pin[slot].p, len, hipMemcpyHostToDevice, up));
        STHIP(hipEventRecord(ev.e[EV_H1], up));
        STHIP(hipEventRecord(ev.e[EV_UP0 + slot], up));
        return NGSQ_OK;
    }
    // The current chunk sized: its n records (the lines, or what max_records leaves of them) take `bytes` bytes; or faulty().
    int size() {
        const uint32_t slot = (uint32_t)(chunks & 1);
        // line starts.  (The last chunk's write pass may still run: it uses none of the arrays touched before the wait below.)
        const uint64_t tiles = samtext_tiles(len);
        STHIP(d_tiles.reserve(tiles + 1));
        STHIP(hipStreamWaitEvent(st, ev.e[EV_UP0 + slot], 0));
        STHIP(hipEventRecord(ev.e[EV_P0], st));
        STHIP(launch_samtext_count(d_text[slot].p, len, d_tiles.p, st));
        STHIP(scan.exclusive_scan(d_tiles.p, tiles + 1, st));
        STHIP(launch_samtext_word(d_tiles.p, tiles, hdev() + HW_LINES, st));
        STHIP(hipStreamSynchronize(st));
        elapsed(EV_H0, EV_H1, &h2d_ms);
        add_write_time();
        const uint64_t lines = h()[HW_LINES];
        n = max_records ? std::min(lines, max_records - records) : lines;
        // sizes, offsets, and the chunk's record bytes and error word to the host
        STHIP(d_start.reserve(n + 1));
        STHIP(d_off.reserve(n + 1));
        STHIP(d_fmark.reserve(n));
        STHIP(d_flist.reserve(n + 1));
        fl = SamTextFloats{d_fmark.p, d_flist.p + 1, reinterpret_cast<unsigned long long *>(d_flist.p)};
        STHIP(launch_samtext_scatter(d_text[slot].p, len, d_tiles.p, n, d_start.p, st));
        STHIP(launch_samtext_word(d_start.p, n, hdev() + HW_TEXT, st));
        STHIP(launch_samtext_size(d_text[slot].p, d_start.p, n, records, refs, d_off.p, d_bad, fl, st));
        STHIP(scan.exclusive_scan(d_off.p, n + 1, st));
        STHIP(launch_samtext_total(d_off.p, n, d_bad, hdev() + HW_BYTES, st));
        STHIP(hipEventRecord(ev.e[EV_P1], st));
        STHIP(hipStreamSynchronize(st));
        elapsed(EV_P0, EV_P1, &parse_ms);
        bytes = h()[HW_BYTES];
        if (h()[HW_BAD] != ~0ull) bad = h()[HW_BAD];
        return NGSQ_OK;
    }
    bool faulty() const { return bad != ~0ull; }
    // The current chunk's records to dst[0, bytes), queued.  also() is queued inside the bracket that parse_ms counts (the keys
    // of samsort.cpp); d_off, the records' offsets in dst, stays as it is until the next chunk is sized.
    template <class F> int write(uint8_t *dst, F &&also) {
        STHIP(hipEventRecord(ev.e[EV_W0], st));
        STHIP(launch_samtext_write(d_text[chunks & 1].p, d_start.p, n, refs, d_off.p, dst, fl, st));
        STHIP(also());
        STHIP(hipEventRecord(ev.e[EV_W1], st));
        write_pending = true;
        return NGSQ_OK;
    }
    int write(uint8_t *dst) {
        return write(dst, [] { return hipSuccess; });
    }
    hipEvent_t written() const { return ev.e[EV_W1]; } // behind the last write
    // The chunk counted, and the next one read and copied up while this one is written -- unless max_records is reached: nothing
    // is read behind the last record.
    int advance() {
        records += n;
        text_bytes += h()[HW_TEXT];
        chunks++;
        len = 0;
        return !max_records || records < max_records ? next((uint32_t)(chunks & 1)) : NGSQ_OK;
    }
    // both streams idle, the last write bracket counted
    int end() {
        STHIP(hipStreamSynchronize(st));
        STHIP(hipStreamSynchronize(up));
        add_write_time();
        return NGSQ_OK;
    }
#undef STHIP
    // what the text itself was refused for: its first faulty record, or a line that does not fit a chunk
    int verdict() const {
        if (faulty())
            return sfail(c, NGSQ_ERR_MALFORMED_RECORD, "reading SAM record: record %llu: %s", (unsigned long long)(bad >> ST_ERR_BITS),
                         samtext_error_text((uint32_t)(bad & ((1u << ST_ERR_BITS) - 1))));
        if (!text.long_line.empty()) return sfail(c, NGSQ_ERR_LIMIT, "reading SAM record: record %llu: %s", (unsigned long long)records, text.long_line.c_str());
        return NGSQ_OK;
    }
};

} // namespace ngsq
