// samsort.cpp -- include/ngsq_samtext.h: `ngs convert --gzip device --sort coordinate <SAM> <BAM>`.  Three
// phases on one GPU.  (1) The chunk loop of samtext.cpp through its write pass, but the records stay where they are written, in
// slabs of device memory, and every record leaves its address, its length and its key behind.  (2) and (3) are
// sort_resident.h's, shared with bamsort.cpp: the sort of (key, record index) pairs, then the sorted stream in pieces through
// k_sort_gather, the device DEFLATE encoder and the output stage, behind the header's blocks and in front of the EOF block.
// Every fault of the text is known before the first byte is written.  The host reads a few words per chunk and per piece and
// never walks a record.
#include "../../include/ngsq_samtext.h"

#include "samtext_host.h"
#include "sort_resident.h"

using namespace ngsq;

namespace {

enum Ev { EV_UP0 = 0, EV_UP1, EV_H0, EV_H1, EV_P0, EV_P1, EV_W0, EV_W1, EV_N };

enum HostWord : uint32_t { HW_LINES = 0, HW_BYTES, HW_BAD, HW_TEXT, HW_WORDS };

// both entries; bai_path: nullptr, or where the index of the file goes
int write_sorted(ngsq_ctx *c, const char *sam_path, int fd, uint64_t max_records, uint64_t chunk_bytes, uint64_t piece_bytes,
                 uint64_t max_resident_bytes, ngsq_samsort_report *out, const char *bai_path, uint64_t index_tile_records,
                 ngsq_index_report *index_out) {
    if (out) memset(out, 0, sizeof *out);
    if (index_out) memset(index_out, 0, sizeof *index_out);
    if (!c || !sam_path || fd < 0) return sfail(c, NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    if (bai_path) { // (before any GPU work, and before a byte goes to fd)
        const std::string m = bai_refuse_existing(bai_path);
        if (!m.empty()) return sfail(c, NGSQ_ERR_INVALID_ARGUMENT, "%s", m.c_str());
    }
    const double t_begin = now_ms();
    if (!chunk_bytes) chunk_bytes = ST_CHUNK_DEFAULT;
    chunk_bytes = std::min(chunk_bytes, ST_CHUNK_MAX);
    if (!piece_bytes) piece_bytes = SORT_PIECE_DEFAULT;
    piece_bytes = std::min(piece_bytes, SORT_PIECE_MAX);
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
    const std::string sorted_text = sorted_header_text(H.text.data(), H.text.size());
    if (sorted_text.size() > 0x7FFFFFFFull) return sfail(c, NGSQ_ERR_INVALID_ARGUMENT, "%sheader text longer than 2^31 - 1 bytes", ST_OPEN_CTX);
    const std::string hs = header_stream(sorted_text, H);
    const RefTable rt(H);
    const uint64_t slab_bytes = std::min(std::max(8 * chunk_bytes, SORT_SLAB_MIN), SORT_SLAB_MAX);

    // ---- the device side; every HIP error leaves through `rc`, so that the writer is stopped either way
#define SHIP(expr)                                                                                  \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) return sfail(c, NGSQ_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
    hipStream_t st = c->stream, up = nullptr;
    DevArray<uint64_t> d_setup, d_tiles, d_start, d_off, d_flist;
    DevArray<uint8_t> d_fmark, d_text[2];
    ScanScratch scan;
    MappedBuf hw;
    TextChunks text;
    HipEvents<EV_N> ev;
    SortResident R; // the slabs, the per-record arrays, phases 2 and 3 (behind the arrays: its drain of st runs first)
    StreamDrain drain_up{nullptr, true};
    R.drain.s = st;
    if (bai_path) {
        R.ix.on = true;
        R.ix.path = bai_path;
        R.ix.ctx = "reading SAM record: ";
        R.ix.tile_records = index_tile_records;
        R.ix.ref_lens = H.lens; // @SQ LN
    }
    uint64_t &records = R.records, &rec_bytes = R.rec_bytes;
    uint64_t text_bytes = 0, chunks = 0, bad = ~0ull, budget = max_resident_bytes;
    double h2d_ms = 0, parse_ms = 0;
    int limit_rc = NGSQ_OK; // a refusal of phase 1 (its message is set)

    auto fill = [&](uint32_t slot, uint64_t *len) -> int {
        if (const int e = text.fill(slot, len)) return sfail(c, NGSQ_ERR_INVALID_ARGUMENT, "reading SAM record: %s (os error %d)", strerror(e), e);
        return NGSQ_OK;
    };
    auto upload = [&](uint32_t slot, uint64_t len) -> int {
        text.move_carry(slot, len);
        SHIP(d_text[slot].reserve(len + ST_TEXT_SLACK));
        SHIP(hipEventRecord(ev.e[EV_H0], up));
        SHIP(hipMemcpyAsync(d_text[slot].p, text.pin[slot].p, len, hipMemcpyHostToDevice, up));
        SHIP(hipEventRecord(ev.e[EV_H1], up));
        SHIP(hipEventRecord(ev.e[EV_UP0 + slot], up));
        return NGSQ_OK;
    };
    auto elapsed = [&](int a, int b, double *sum) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.e[a], ev.e[b]) == hipSuccess) *sum += ms;
    };

    // phase 1: every record written into a slab, nothing compressed
    auto parse = [&]() -> int {
        SHIP(hipSetDevice(c->device));
        SHIP(pool_stream_get(false, &up));
        drain_up.s = up;
        if (!budget) {
            size_t free_b = 0, total_b = 0;
            SHIP(hipMemGetInfo(&free_b, &total_b));
            budget = free_b > SORT_DEVICE_RESERVE ? free_b - SORT_DEVICE_RESERVE : 0;
        }
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
        if (const int rc = R.begin(st)) return sfail(c, rc, "%s", R.err.c_str());
        for (int k = 0; k < EV_N; k++) {
            if (k == EV_UP0 || k == EV_UP1) SHIP(hipEventCreateWithFlags(&ev.e[k], hipEventDisableTiming));
            else SHIP(hipEventCreate(&ev.e[k]));
        }
        uint64_t len = 0;
        bool write_timed = true; // false: the last chunk's write pass has not been added to parse_ms
        if (const int rc = fill(0, &len)) return rc;
        if (len)
            if (const int rc = upload(0, len)) return rc;
        while (len) {
            const uint32_t slot = (uint32_t)(chunks & 1);
            // line starts.  (Chunk k - 1's write pass may still run: it uses none of the arrays touched before the wait below.)
            const uint64_t tiles = samtext_tiles(len);
            SHIP(d_tiles.reserve(tiles + 1));
            SHIP(hipStreamWaitEvent(st, ev.e[EV_UP0 + slot], 0));
            SHIP(hipEventRecord(ev.e[EV_P0], st));
            SHIP(launch_samtext_count(d_text[slot].p, len, d_tiles.p, st));
            SHIP(scan.exclusive_scan(d_tiles.p, tiles + 1, st));
            SHIP(launch_samtext_word(d_tiles.p, tiles, hdev + HW_LINES, st));
            SHIP(hipStreamSynchronize(st));
            elapsed(EV_H0, EV_H1, &h2d_ms);
            if (!write_timed) elapsed(EV_W0, EV_W1, &parse_ms), write_timed = true;
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
            elapsed(EV_P0, EV_P1, &parse_ms);
            const uint64_t bytes = h[HW_BYTES];
            if (h[HW_BAD] != ~0ull) {
                bad = h[HW_BAD];
                break;
            }
            if (records + n > 0xFFFFFFFFull) {
                limit_rc = sfail(c, NGSQ_ERR_LIMIT, "reading SAM record: --sort coordinate sorts at most 2^32 - 1 records");
                break;
            }
            const uint64_t need = rec_bytes + bytes + (records + n) * SORT_BYTES_PER_RECORD;
            if (need > budget) {
                limit_rc = sfail(c, NGSQ_ERR_LIMIT, "reading SAM record: --sort coordinate holds the records in device memory: %llu bytes needed, %llu allowed",
                                 (unsigned long long)need, (unsigned long long)budget);
                break;
            }
            // the records stay: behind the last chunk's in the newest slab, or at the front of a new one
            uint8_t *dst = nullptr;
            if (const int rc = R.place(bytes, slab_bytes, ~0u, &dst)) return sfail(c, rc, "%s", R.err.c_str());
            if (const int rc = R.reserve_records(records + n)) return sfail(c, rc, "%s", R.err.c_str());
            SHIP(hipEventRecord(ev.e[EV_W0], st));
            SHIP(launch_samtext_write(d_text[slot].p, d_start.p, n, refs, d_off.p, dst, fl, st));
            SHIP(launch_sort_keys(dst, d_off.p, n, records, R.d_addr.p, R.d_len.p, R.d_key.p, st));
            SHIP(hipEventRecord(ev.e[EV_W1], st));
            write_timed = false;
            rec_bytes += bytes;
            records += n;
            text_bytes += h[HW_TEXT];
            chunks++;
            // the next chunk is read and copied up while this one is written
            uint64_t next = 0;
            if (!max_records || records < max_records) {
                if (const int rc = fill(slot ^ 1, &next)) return rc;
                if (next)
                    if (const int rc = upload(slot ^ 1, next)) return rc;
            }
            len = next;
        }
        SHIP(hipStreamSynchronize(st));
        SHIP(hipStreamSynchronize(up));
        if (!write_timed) elapsed(EV_W0, EV_W1, &parse_ms);
        return NGSQ_OK;
    };

    int rc = parse();
    if (rc == NGSQ_OK && bad != ~0ull)
        rc = sfail(c, NGSQ_ERR_MALFORMED_RECORD, "reading SAM record: record %llu: %s", (unsigned long long)(bad >> ST_ERR_BITS),
                   samtext_error_text((uint32_t)(bad & ((1u << ST_ERR_BITS) - 1))));
    if (rc == NGSQ_OK) rc = limit_rc;
    if (rc == NGSQ_OK && !text.long_line.empty())
        rc = sfail(c, NGSQ_ERR_LIMIT, "reading SAM record: record %llu: %s", (unsigned long long)records, text.long_line.c_str());
    // phases 2 and 3: the order, then header, pieces
    if (rc == NGSQ_OK) rc = R.sort_and_write(fd, c->device, hs, piece_bytes);
#undef SHIP
    rc = R.finish(rc, fd);
    if (rc != NGSQ_OK && !R.err.empty()) sfail(c, rc, "%s", R.err.c_str());
    if (out) {
        out->records = records;
        out->header_bytes = sorted_text.size();
        out->text_bytes = text_bytes;
        out->bam_bytes = R.bam_bytes;
        out->compressed_bytes = R.enc.comp_bytes;
        out->chunks = chunks;
        out->pieces = R.pieces;
        out->blocks = R.enc.blocks;
        out->stored_blocks = R.enc.stored;
        out->resident_bytes = R.resident_bytes();
        out->passes_run = R.sort.passes_run;
        out->passes_skipped = SORT_DIGITS - R.sort.passes_run; // (no records: no pass, as ngsq_sort_u64_device reports it)
        out->read_ms = text.read_ms;
        out->h2d_ms = h2d_ms;
        out->parse_ms = parse_ms;
        out->sort_ms = R.sort_ms;
        out->gather_ms = R.gather_ms;
        out->deflate_ms = R.deflate_ms;
        out->d2h_ms = R.w.copy_ms;
        out->write_ms = R.w.write_ms;
        out->total_ms = now_ms() - t_begin;
    }
    if (bai_path) R.ix.report(records, index_out);
    return rc;
}

} // namespace

extern "C" {

int ngsq_sam_write_sorted_bam(ngsq_ctx *c, const char *sam_path, int fd, uint64_t max_records, uint64_t chunk_bytes, uint64_t piece_bytes,
                              uint64_t max_resident_bytes, ngsq_samsort_report *out) {
    return write_sorted(c, sam_path, fd, max_records, chunk_bytes, piece_bytes, max_resident_bytes, out, nullptr, 0, nullptr);
}

int ngsq_sam_write_sorted_bam_indexed(ngsq_ctx *c, const char *sam_path, int fd, uint64_t max_records, uint64_t chunk_bytes, uint64_t piece_bytes,
                                      uint64_t max_resident_bytes, ngsq_samsort_report *out, const char *bai_path, uint64_t index_tile_records,
                                      ngsq_index_report *index_out) {
    if (!bai_path) return sfail(c, NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    return write_sorted(c, sam_path, fd, max_records, chunk_bytes, piece_bytes, max_resident_bytes, out, bai_path, index_tile_records, index_out);
}

} // extern "C"
