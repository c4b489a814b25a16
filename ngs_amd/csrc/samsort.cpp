// samsort.cpp -- include/ngsq_samtext.h: `ngs convert --gzip device --sort coordinate <SAM> <BAM>`.  Three
// phases on one GPU.  (1) The chunk loop of samtext.cpp through its write pass, but the records stay where they are written, in
// slabs of device memory, and every record leaves its address, its length and its key behind.  (2) sort_pairs_u64 (sort.cpp)
// orders (key, record index) pairs.  (3) The sorted stream is cut into pieces of piece_bytes; per piece k_sort_gather copies the
// records to their sorted offsets, the device DEFLATE encoder makes BGZF blocks of them and the output stage of device_out.h
// writes them, behind the header's blocks and in front of the EOF block.  Every fault of the text is known before the first
// byte is written.  The host reads a few words per chunk and per piece and never walks a record.
#include "../../include/ngsq_samtext.h"

#include <memory>

#include "samtext_host.h"
#include "sort_kernels.h"

using namespace ngsq;

namespace {

constexpr uint64_t SORT_PIECE_DEFAULT = (uint64_t)64 << 20, SORT_PIECE_MAX = (uint64_t)1 << 30;
// Device bytes per resident record beside its own: address 8, length 4, key 8, the sort's second key array and its two index
// arrays 16, the sorted offset 8, and its share of the pass table (half a byte).
constexpr uint64_t SORT_BYTES_PER_RECORD = 48;
// What the default budget leaves free of the memory hipMemGetInfo reports: the two text buffers, a chunk's line and offset
// arrays, the piece buffer, the encoder's scratch and its two block buffers, the unused end of the last slab, and the old
// halves of the per-record arrays while they double.
constexpr uint64_t SORT_DEVICE_RESERVE = (uint64_t)4 << 30;
constexpr uint64_t SORT_SLAB_MIN = (uint64_t)1 << 20, SORT_SLAB_MAX = (uint64_t)512 << 20;

enum Ev { EV_UP0 = 0, EV_UP1, EV_H0, EV_H1, EV_P0, EV_P1, EV_W0, EV_W1, EV_S0, EV_S1, EV_G0, EV_G1, EV_Z1, EV_N };

enum HostWord : uint32_t { HW_LINES = 0, HW_BYTES, HW_BAD, HW_TEXT, HW_TOTAL, HW_DEFLATE, HW_WORDS = HW_DEFLATE + DEFLATE_HOST_WORDS };

} // namespace

extern "C" {

int ngsq_sam_write_sorted_bam(ngsq_ctx *c, const char *sam_path, int fd, uint64_t max_records, uint64_t chunk_bytes, uint64_t piece_bytes,
                              uint64_t max_resident_bytes, ngsq_samsort_report *out) {
    if (out) memset(out, 0, sizeof *out);
    if (!c || !sam_path || fd < 0) return sfail(c, NGSQ_ERR_INVALID_ARGUMENT, "null argument");
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
    DevArray<uint64_t> d_setup, d_tiles, d_start, d_off, d_flist, d_addr, d_key, d_soff;
    DevArray<uint32_t> d_len;
    DevArray<uint8_t> d_fmark, d_text[2], d_piece;
    std::vector<std::unique_ptr<DevArray<uint8_t>>> slabs; // the records: a slab is filled from its front and never moved
    uint64_t slab_used = 0;
    ScanScratch scan;
    SortScratch sort;
    BgzfEncoder enc; // d_piece's bytes become the blocks of a job
    JobSlots zslots;
    MappedBuf hw, hw_first;
    TextChunks text;
    HipEvents<EV_N> ev;
    DeviceWriter w;
    StreamDrain drain{st}, drain_up{nullptr, true}; // (behind the arrays: they run first)
    uint64_t records = 0, text_bytes = 0, rec_bytes = 0, bam_bytes = 0, chunks = 0, pieces = 0, bad = ~0ull, budget = max_resident_bytes;
    double h2d_ms = 0, parse_ms = 0, sort_ms = 0, gather_ms = 0, deflate_ms = 0;
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
    auto copy_failed = [&](hipError_t e) { return sfail(c, NGSQ_ERR_DEVICE, "copying the BGZF blocks to the host: %s", hipGetErrorString(e)); };
    // bytes of d_piece through the encoder into its buffer of the job's slot, the blocks to the writer (as samtext.cpp's jobs)
    auto compress_and_push = [&](uint64_t bytes) -> int {
        SHIP(enc.launch(zslots.slot(), d_piece.p, bytes, st));
        SHIP(hipEventRecord(ev.e[EV_Z1], st));
        SHIP(hipEventSynchronize(ev.e[EV_Z1]));
        const char *blocks = nullptr;
        uint64_t n = 0;
        if (const char *m = enc.collect(zslots.slot(), bytes, &blocks, &n)) return sfail(c, NGSQ_ERR_STATE, "%s", m);
        elapsed(EV_G1, EV_Z1, &deflate_ms);
        SHIP(zslots.submit(w, blocks, n, st));
        bam_bytes += bytes;
        return NGSQ_OK;
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
        enc.h = h + HW_DEFLATE;
        enc.hdev = hdev + HW_DEFLATE;
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
            if (slabs.empty() || slab_used + bytes + SORT_GATHER_SLACK > slabs.back()->cap) {
                slabs.emplace_back(new DevArray<uint8_t>());
                SHIP(slabs.back()->reserve(std::max(slab_bytes, bytes) + SORT_GATHER_SLACK));
                slab_used = 0;
            }
            uint8_t *const dst = slabs.back()->p + slab_used;
            SHIP(d_addr.reserve_keep(records + n, st));
            SHIP(d_len.reserve_keep(records + n, st));
            SHIP(d_key.reserve_keep(records + n, st));
            SHIP(hipEventRecord(ev.e[EV_W0], st));
            SHIP(launch_samtext_write(d_text[slot].p, d_start.p, n, refs, d_off.p, dst, fl, st));
            SHIP(launch_sort_keys(dst, d_off.p, n, records, d_addr.p, d_len.p, d_key.p, st));
            SHIP(hipEventRecord(ev.e[EV_W1], st));
            write_timed = false;
            slab_used += bytes;
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

    // phases 2 and 3: the order, then header, pieces
    auto sort_and_write = [&]() -> int {
        unsigned long long *const hdev = static_cast<unsigned long long *>(hw.dev);
        const unsigned long long *const h = static_cast<const unsigned long long *>(hw.h);
        const uint32_t *perm = nullptr;
        uint64_t total = 0;
        const unsigned long long *first = nullptr;
        if (records) {
            SHIP(hipEventRecord(ev.e[EV_S0], st));
            SHIP(sort_pairs_u64(d_key.p, records, sort, st, &perm));
            // the sorted offsets, and the record every piece begins in
            SHIP(d_soff.reserve(records + 1));
            SHIP(launch_sort_lengths(d_len.p, perm, records, d_soff.p, st));
            SHIP(scan.exclusive_scan(d_soff.p, records + 1, st));
            SHIP(launch_samtext_word(d_soff.p, records, hdev + HW_TOTAL, st));
            SHIP(hipEventRecord(ev.e[EV_S1], st));
            SHIP(hipStreamSynchronize(st));
            elapsed(EV_S0, EV_S1, &sort_ms);
            total = h[HW_TOTAL];
            if (total != rec_bytes) return sfail(c, NGSQ_ERR_STATE, "the sorted records take %llu bytes, the parsed ones %llu", (unsigned long long)total, (unsigned long long)rec_bytes);
            pieces = (total + piece_bytes - 1) / piece_bytes;
            if (pieces >= 0x7FFFFFFFull) return sfail(c, NGSQ_ERR_LIMIT, "writing BAM record: more than 2^31 - 2 pieces of %llu bytes", (unsigned long long)piece_bytes);
            SHIP(hw_first.reserve((pieces + 1) * sizeof(unsigned long long)));
            SHIP(launch_sort_bisect(d_soff.p, records, piece_bytes, pieces, static_cast<unsigned long long *>(hw_first.dev), st));
            SHIP(hipStreamSynchronize(st));
            first = static_cast<const unsigned long long *>(hw_first.h);
        }
        SHIP(zslots.create());
        SHIP(w.start(fd, c->device));
        // the header's blocks, in front of the first record (as samtools writes them)
        SHIP(d_piece.reserve(std::max<uint64_t>(hs.size(), std::min(piece_bytes, total)) + DEFLATE_IN_SLACK));
        SHIP(hipMemcpyAsync(d_piece.p, hs.data(), hs.size(), hipMemcpyHostToDevice, st));
        SHIP(hipEventRecord(ev.e[EV_G1], st));
        if (const int rc = compress_and_push(hs.size())) return rc;
        for (uint64_t j = 0; j < pieces && !w.failed(); j++) {
            const uint64_t lo = j * piece_bytes, hi = std::min(lo + piece_bytes, total);
            // records first[j] .. first[j + 1]: the last of them may begin in this piece and end in the next
            const uint64_t a = first[j], b = std::min<uint64_t>(first[j + 1] + 1, records);
            if (!zslots.acquire(&w)) return copy_failed(w.herr);
            SHIP(hipEventRecord(ev.e[EV_G0], st));
            SHIP(launch_sort_gather(d_addr.p, perm, d_soff.p, a, b, lo, hi, d_piece.p, st));
            SHIP(hipEventRecord(ev.e[EV_G1], st));
            if (const int rc = compress_and_push(hi - lo)) return rc;
            elapsed(EV_G0, EV_G1, &gather_ms);
        }
        SHIP(hipStreamSynchronize(st));
        return NGSQ_OK;
    };

    int rc = parse();
    if (rc == NGSQ_OK && bad != ~0ull)
        rc = sfail(c, NGSQ_ERR_MALFORMED_RECORD, "reading SAM record: record %llu: %s", (unsigned long long)(bad >> ST_ERR_BITS),
                   samtext_error_text((uint32_t)(bad & ((1u << ST_ERR_BITS) - 1))));
    if (rc == NGSQ_OK) rc = limit_rc;
    if (rc == NGSQ_OK && !text.long_line.empty())
        rc = sfail(c, NGSQ_ERR_LIMIT, "reading SAM record: record %llu: %s", (unsigned long long)records, text.long_line.c_str());
    if (rc == NGSQ_OK) rc = sort_and_write();
#undef SHIP
    auto write_failed = [&](int e) { return sfail(c, NGSQ_ERR_INVALID_ARGUMENT, "writing BAM record: %s (os error %d)", strerror(e), e); };
    const WriterEnd end = w.end();
    if (rc == NGSQ_OK && end.herr != hipSuccess) rc = copy_failed(end.herr);
    if (rc == NGSQ_OK && end.werr) rc = write_failed(end.werr);
    if (rc == NGSQ_OK) {
        if (const int e = write_bgzf_eof(fd)) rc = write_failed(e);
        enc.comp_bytes += sizeof BGZF_EOF_BLOCK;
    }
    if (out) {
        out->records = records;
        out->header_bytes = sorted_text.size();
        out->text_bytes = text_bytes;
        out->bam_bytes = bam_bytes;
        out->compressed_bytes = enc.comp_bytes;
        out->chunks = chunks;
        out->pieces = pieces;
        out->blocks = enc.blocks;
        out->stored_blocks = enc.stored;
        out->resident_bytes = rec_bytes + records * SORT_BYTES_PER_RECORD;
        out->passes_run = sort.passes_run;
        out->passes_skipped = SORT_DIGITS - sort.passes_run; // (no records: no pass, as ngsq_sort_u64_device reports it)
        out->read_ms = text.read_ms;
        out->h2d_ms = h2d_ms;
        out->parse_ms = parse_ms;
        out->sort_ms = sort_ms;
        out->gather_ms = gather_ms;
        out->deflate_ms = deflate_ms;
        out->d2h_ms = w.copy_ms;
        out->write_ms = w.write_ms;
        out->total_ms = now_ms() - t_begin;
    }
    return rc;
}

} // extern "C"
