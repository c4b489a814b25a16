// samtext.cpp -- include/ngsq_samtext.h: `ngs convert --gzip device <SAM> <BAM>`.  The host reads the
// header (the leading '@' lines), builds the reference list and its hash table, and then only moves bytes: the text goes in
// chunks that end on a newline through two pinned buffers to the device, samtext_kernel.hip finds the lines and turns them
// into BAM records, the device DEFLATE encoder (deflate_kernels.h) makes BGZF blocks of them, and the output stage of
// device_out.h carries the blocks through its pinned ring to the descriptor.  While chunk k is written and compressed the host
// reads chunk k + 1 and copies it up on a second stream; while chunk k + 1 is parsed the writer copies chunk k down and
// writes it.  Per chunk the host reads four words: lines, record bytes, error word, compressed bytes.
#include "../../include/ngsq_samtext.h"

#include "samtext_host.h"

using namespace ngsq;

namespace {

enum Ev { EV_UP0 = 0, EV_UP1, EV_H0, EV_H1, EV_P0, EV_P1, EV_W0, EV_W1, EV_Z1, EV_N };

enum HostWord : uint32_t { HW_LINES = 0, HW_BYTES, HW_BAD, HW_TEXT, HW_DEFLATE, HW_WORDS = HW_DEFLATE + DEFLATE_HOST_WORDS };

} // namespace

extern "C" {

int ngsq_sam_parse_f32(const char *text, uint32_t len, uint32_t *bits) {
    if (!text || !bits || len > ST_FLOAT_TEXT_MAX) return NGSQ_ERR_INVALID_ARGUMENT;
    return samtext_parse_f32_host(reinterpret_cast<const uint8_t *>(text), len, bits) ? NGSQ_OK : NGSQ_ERR_INVALID_ARGUMENT;
}

int ngsq_sam_check_header(const char *sam_path, uint32_t *n_refs, char *why, size_t why_cap) {
    auto say = [&](const std::string &m) {
        if (why && why_cap) snprintf(why, why_cap, "%s%s", ST_OPEN_CTX, m.c_str());
        return NGSQ_ERR_INVALID_ARGUMENT;
    };
    if (why && why_cap) why[0] = 0;
    if (!sam_path) return say("null argument");
    Fd in;
    in.fd = open(sam_path, O_RDONLY | O_CLOEXEC);
    if (in.fd < 0) {
        const int e = errno;
        return say(std::string(strerror(e)) + " (os error " + std::to_string(e) + ")");
    }
    SamHeader h;
    const std::string m = read_header(in.fd, &h);
    if (!m.empty()) return say(m);
    if (n_refs) *n_refs = (uint32_t)h.names.size();
    return NGSQ_OK;
}

int ngsq_sam_write_bam(ngsq_ctx *c, const char *sam_path, int fd, uint64_t max_records, uint64_t chunk_bytes, ngsq_samtext_report *out) {
    if (out) memset(out, 0, sizeof *out);
    if (!c || !sam_path || fd < 0) return sfail(c, NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    const double t_begin = now_ms();
    if (!chunk_bytes) chunk_bytes = ST_CHUNK_DEFAULT;
    chunk_bytes = std::min(chunk_bytes, ST_CHUNK_MAX);
    Fd in;
    in.fd = open(sam_path, O_RDONLY | O_CLOEXEC);
    if (in.fd < 0) {
        const int e = errno;
        return sfail(c, NGSQ_ERR_INVALID_ARGUMENT, "%s%s (os error %d)", ST_OPEN_CTX, strerror(e), e);
    }
    SamHeader H;
    {
        const std::string m = read_header(in.fd, &H);
        if (!m.empty()) return sfail(c, NGSQ_ERR_INVALID_ARGUMENT, "%s%s", ST_OPEN_CTX, m.c_str());
    }
    const std::string hs = header_stream(H.text, H);
    const RefTable rt(H);

    // ---- the device side; every HIP error leaves through `rc`, so that the writer is stopped either way
#define SHIP(expr)                                                                                  \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) return sfail(c, NGSQ_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
    hipStream_t st = c->stream, up = nullptr;
    DevArray<uint64_t> d_setup, d_tiles, d_start, d_off, d_flist;
    DevArray<uint8_t> d_fmark, d_text[2], d_rec;
    ScanScratch scan;
    BgzfEncoder enc; // d_rec's bytes become the blocks of a job
    JobSlots zslots; // of the encoder's blocks (d_text alternates with the chunks, apart from them)
    MappedBuf hw;
    TextChunks text;
    HipEvents<EV_N> ev;
    DeviceWriter w;
    StreamDrain drain{st}, drain_up{nullptr, true}; // (behind the arrays: they run first)
    uint64_t records = 0, text_bytes = 0, bam_bytes = 0, chunks = 0, bad = ~0ull;
    double h2d_ms = 0, parse_ms = 0, deflate_ms = 0;
    // the next chunk into the text's buffer `slot`: *len bytes that end on a newline (0: the file has ended)
    auto fill = [&](uint32_t slot, uint64_t *len) -> int {
        if (const int e = text.fill(slot, len)) return sfail(c, NGSQ_ERR_INVALID_ARGUMENT, "reading SAM record: %s (os error %d)", strerror(e), e);
        return NGSQ_OK;
    };
    // pin[slot][0, len) to d_text[slot] on the copy stream; the carry moves to the other buffer first (the copy only reads)
    auto upload = [&](uint32_t slot, uint64_t len) -> int {
        text.move_carry(slot, len);
        SHIP(d_text[slot].reserve(len + ST_TEXT_SLACK));
        SHIP(hipEventRecord(ev.e[EV_H0], up));
        SHIP(hipMemcpyAsync(d_text[slot].p, text.pin[slot].p, len, hipMemcpyHostToDevice, up));
        SHIP(hipEventRecord(ev.e[EV_H1], up));
        SHIP(hipEventRecord(ev.e[EV_UP0 + slot], up));
        return NGSQ_OK;
    };
    auto copy_failed = [&](hipError_t e) { return sfail(c, NGSQ_ERR_DEVICE, "copying the BGZF blocks to the host: %s", hipGetErrorString(e)); };
    // bytes of d_rec through the encoder into its buffer of the job's slot; push_job waits for it and hands the blocks to the writer
    auto compress = [&](uint64_t bytes) -> int {
        if (!zslots.acquire(&w)) return copy_failed(w.herr);
        SHIP(enc.launch(zslots.slot(), d_rec.p, bytes, st));
        SHIP(hipEventRecord(ev.e[EV_Z1], st));
        return NGSQ_OK;
    };
    auto push_job = [&](uint64_t bytes) -> int {
        SHIP(hipEventSynchronize(ev.e[EV_Z1]));
        const char *blocks = nullptr;
        uint64_t n = 0;
        if (const char *m = enc.collect(zslots.slot(), bytes, &blocks, &n)) return sfail(c, NGSQ_ERR_STATE, "%s", m);
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.e[EV_W1], ev.e[EV_Z1]) == hipSuccess) deflate_ms += ms;
        // (nothing may be queued on st between compress and here: `ready` would cover it and hold the copy back)
        SHIP(zslots.submit(w, blocks, n, st));
        bam_bytes += bytes;
        return NGSQ_OK;
    };

    auto run = [&]() -> int {
        SHIP(hipSetDevice(c->device));
        SHIP(pool_stream_get(false, &up));
        drain_up.s = up;
        SHIP(d_setup.reserve(rt.device_words()));
        SHIP(rt.upload(d_setup.p, st));
        SHIP(hipStreamSynchronize(st));
        unsigned long long *const d_bad = rt.bad(d_setup.p);
        const SamTextRefs refs = rt.refs(d_setup.p);
        SHIP(hw.reserve(HW_WORDS * sizeof(unsigned long long)));
        memset(hw.h, 0, HW_WORDS * sizeof(unsigned long long));
        unsigned long long *const hdev = static_cast<unsigned long long *>(hw.dev);
        const unsigned long long *const h = static_cast<const unsigned long long *>(hw.h);
        SHIP(text.start(in.fd, chunk_bytes, H.body_at));
        enc.h = h + HW_DEFLATE;
        enc.hdev = hdev + HW_DEFLATE;
        for (int k = 0; k < EV_N; k++) {
            if (k == EV_UP0 || k == EV_UP1) SHIP(hipEventCreateWithFlags(&ev.e[k], hipEventDisableTiming));
            else SHIP(hipEventCreate(&ev.e[k]));
        }
        SHIP(zslots.create());
        SHIP(w.start(fd, c->device));
        // the header's blocks, in front of the first record (as samtools writes them)
        SHIP(d_rec.reserve(hs.size() + DEFLATE_IN_SLACK));
        SHIP(hipMemcpyAsync(d_rec.p, hs.data(), hs.size(), hipMemcpyHostToDevice, st));
        SHIP(hipEventRecord(ev.e[EV_W1], st));
        if (const int rc = compress(hs.size())) return rc;
        if (const int rc = push_job(hs.size())) return rc;
        // the chunks
        uint64_t len = 0;
        if (const int rc = fill(0, &len)) return rc;
        if (len)
            if (const int rc = upload(0, len)) return rc;
        while (len && !w.failed()) {
            const uint32_t slot = (uint32_t)(chunks & 1);
            // line starts
            const uint64_t tiles = samtext_tiles(len);
            SHIP(d_tiles.reserve(tiles + 1));
            SHIP(hipStreamWaitEvent(st, ev.e[EV_UP0 + slot], 0));
            SHIP(hipEventRecord(ev.e[EV_P0], st));
            SHIP(launch_samtext_count(d_text[slot].p, len, d_tiles.p, st));
            SHIP(scan.exclusive_scan(d_tiles.p, tiles + 1, st));
            SHIP(launch_samtext_word(d_tiles.p, tiles, hdev + HW_LINES, st));
            SHIP(hipStreamSynchronize(st));
            {
                float ms = 0;
                if (hipEventElapsedTime(&ms, ev.e[EV_H0], ev.e[EV_H1]) == hipSuccess) h2d_ms += ms;
            }
            const uint64_t lines = h[HW_LINES];
            const uint64_t n = max_records ? std::min(lines, max_records - records) : lines;
            // sizes, offsets, and the chunk's record bytes and error word to the host
            SHIP(d_start.reserve(n + 1));
            SHIP(d_off.reserve(n + 1));
            SHIP(d_fmark.reserve(n));
            SHIP(d_flist.reserve(n + 1));
            const SamTextFloats fl{d_fmark.p, d_flist.p + 1, reinterpret_cast<unsigned long long *>(d_flist.p)};
            SHIP(launch_samtext_scatter(d_text[slot].p, len, d_tiles.p, n, d_start.p, st));
            SHIP(launch_samtext_word(d_start.p, n, hdev + HW_TEXT, st));
            SHIP(launch_samtext_size(d_text[slot].p, d_start.p, n, records, refs, d_off.p, d_bad, fl, st));
            SHIP(scan.exclusive_scan(d_off.p, n + 1, st));
            SHIP(launch_samtext_total(d_off.p, n, d_bad, hdev + HW_BYTES, st));
            SHIP(hipEventRecord(ev.e[EV_P1], st));
            SHIP(hipStreamSynchronize(st));
            {
                float ms = 0;
                if (hipEventElapsedTime(&ms, ev.e[EV_P0], ev.e[EV_P1]) == hipSuccess) parse_ms += ms;
            }
            const uint64_t bytes = h[HW_BYTES];
            if (h[HW_BAD] != ~0ull) {
                bad = h[HW_BAD];
                break;
            }
            // the records, and their blocks
            SHIP(d_rec.reserve(bytes + DEFLATE_IN_SLACK));
            SHIP(hipEventRecord(ev.e[EV_W0], st));
            SHIP(launch_samtext_write(d_text[slot].p, d_start.p, n, refs, d_off.p, d_rec.p, fl, st));
            SHIP(hipEventRecord(ev.e[EV_W1], st));
            if (const int rc = compress(bytes)) return rc;
            records += n;
            text_bytes += h[HW_TEXT];
            chunks++;
            // the next chunk is read and copied up while this one is written and compressed
            uint64_t next = 0;
            if (!max_records || records < max_records) {
                if (const int rc = fill(slot ^ 1, &next)) return rc;
                if (next)
                    if (const int rc = upload(slot ^ 1, next)) return rc;
            }
            if (const int rc = push_job(bytes)) return rc;
            {
                float ms = 0;
                if (hipEventElapsedTime(&ms, ev.e[EV_W0], ev.e[EV_W1]) == hipSuccess) parse_ms += ms;
            }
            len = next;
        }
        SHIP(hipStreamSynchronize(st));
        SHIP(hipStreamSynchronize(up));
        return NGSQ_OK;
    };
    int rc = run();
#undef SHIP
    auto write_failed = [&](int e) { return sfail(c, NGSQ_ERR_INVALID_ARGUMENT, "writing BAM record: %s (os error %d)", strerror(e), e); };
    const WriterEnd end = w.end();
    if (rc == NGSQ_OK && end.herr != hipSuccess) rc = copy_failed(end.herr);
    if (rc == NGSQ_OK && end.werr) rc = write_failed(end.werr);
    if (rc == NGSQ_OK && bad != ~0ull)
        rc = sfail(c, NGSQ_ERR_MALFORMED_RECORD, "reading SAM record: record %llu: %s", (unsigned long long)(bad >> ST_ERR_BITS),
                   samtext_error_text((uint32_t)(bad & ((1u << ST_ERR_BITS) - 1))));
    if (rc == NGSQ_OK && !text.long_line.empty())
        rc = sfail(c, NGSQ_ERR_LIMIT, "reading SAM record: record %llu: %s", (unsigned long long)records, text.long_line.c_str());
    if (rc == NGSQ_OK) {
        if (const int e = write_bgzf_eof(fd)) rc = write_failed(e);
        enc.comp_bytes += sizeof BGZF_EOF_BLOCK;
    }
    if (out) {
        out->records = records;
        out->header_bytes = H.text.size();
        out->text_bytes = text_bytes;
        out->bam_bytes = bam_bytes;
        out->compressed_bytes = enc.comp_bytes;
        out->chunks = chunks;
        out->blocks = enc.blocks;
        out->stored_blocks = enc.stored;
        out->read_ms = text.read_ms;
        out->h2d_ms = h2d_ms;
        out->parse_ms = parse_ms;
        out->deflate_ms = deflate_ms;
        out->d2h_ms = w.copy_ms;
        out->write_ms = w.write_ms;
        out->total_ms = now_ms() - t_begin;
    }
    return rc;
}

} // extern "C"
