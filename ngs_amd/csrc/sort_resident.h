// sort_resident.h -- what the two drivers of `ngs convert --sort coordinate` share (DESIGN.md sections 19.2 and 20.2): samsort.cpp
// (SAM text in) and bamsort.cpp (BAM in).  A driver's phase 1 leaves the records in slabs of device memory and their addresses,
// lengths and keys in the three per-record arrays; phases 2 and 3 are here: sort_pairs_u64 orders (key, record index) pairs, the
// sorted stream is cut into pieces of piece_bytes, per piece k_sort_gather copies the records to their sorted offsets and the
// sink of device_out.h compresses and writes them, behind the header's blocks and in front of the EOF block.  Also here, once
// for both drivers: the admission of phase 1's records to the slabs (the limits, the default budget, the place) and the fields
// their reports share.  A failure leaves its code and its message in `err`; the driver reports it through its own channel.
// With `ix.on` (--write-index) the BAI of the file is built on the way: an index pass over the sorted order
// before the writer starts, the encoder's block offsets kept per piece, and one translation from stream offsets to virtual
// positions behind the last piece; bai.cpp's writer makes the file once the EOF block is out.
// Phases 2 and 3 come in steps -- the file's beginning, a round, the file's end -- so that bamsort.cpp can sort a BAM beyond the
// budget in rounds: each round's records are resident in turn and continue the same stream of pieces.
// `ngs markdup` (markdup.cpp) keeps its records and writes its pieces through this object too, in an order
// of its own (order_given, write_records) instead of the sort's.
#pragma once

#include <cstdarg>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ngsq_index.h"
#include "bai_host.h"
#include "device_out.h"
#include "samtext_kernels.h" // launch_samtext_word
#include "sort_kernels.h"

namespace ngsq {

constexpr uint64_t SORT_PIECE_DEFAULT = (uint64_t)64 << 20, SORT_PIECE_MAX = (uint64_t)1 << 30;
// What the default budget leaves free of the memory hipMemGetInfo reports: the two text buffers, a chunk's line and offset
// arrays, the piece buffer, the encoder's scratch and its two block buffers, the unused end of the last slab, and the old
// halves of the per-record arrays while they double.
constexpr uint64_t SORT_DEVICE_RESERVE = (uint64_t)4 << 30;
constexpr uint64_t SORT_SLAB_MIN = (uint64_t)1 << 20, SORT_SLAB_MAX = (uint64_t)512 << 20;
// Sorted records per tile of the index pass: the ingest's batch size, so that the tile buffers (a run flag and a tentative run
// per record, 32 bytes) are section 12.2's, 128 MiB, inside SORT_DEVICE_RESERVE.
constexpr uint64_t SORT_INDEX_TILE = (uint64_t)1 << 22;

// the device times of the last indexed call on this thread, in ms (ngsq_sort_index_split)
struct SortIndexSplit {
    double pass_ms = 0, blocks_ms = 0, translate_ms = 0;
};
inline thread_local SortIndexSplit g_sort_index_split;

// What --write-index adds to a SortResident.  The driver calls enable() before sort_and_write; everything else is the shared
// phases'.
struct SortIndex {
    bool on = false;
    std::string path, ctx;
    uint64_t tile_records = SORT_INDEX_TILE;
    std::vector<uint32_t> ref_lens;
    BaiTables T;
    DevArray<uint64_t> d_flag, d_table; // a tile's run flags; the file's block table
    DevArray<BaiRun> d_tmp, d_runs;     // a tile's tentative runs; the run list
    ScanScratch scan;
    uint64_t runs = 0, blocks_per_piece = 0, final_end = 0;
    uint32_t parity = 0; // of the tile carry
    bool begun = false, append_pending = false;
    std::vector<BaiRun> R; // what the end copies to the host: the run list and the windows, translated
    std::vector<unsigned long long> lin;
    SortIndexSplit ms;
    double write_ms = 0;
    BaiFileCounts counts;

    // path_: <TO>.bai; ctx_: the driver's message prefix; tile: sorted records per tile of the index pass (0: SORT_INDEX_TILE);
    // lens: the sequences' lengths
    void enable(const char *path_, const char *ctx_, uint64_t tile, const std::vector<uint32_t> &lens) {
        on = true;
        path = path_;
        ctx = ctx_;
        tile_records = tile;
        ref_lens = lens;
    }
    void report(uint64_t records, ngsq_index_report *out) const {
        if (!on) return;
        g_sort_index_split = ms;
        if (!out) return;
        out->records = records;
        out->n_no_coor = counts.n_no_coor;
        out->runs = runs;
        out->bins = counts.bins;
        out->scan_ms = ms.pass_ms + ms.blocks_ms + ms.translate_ms;
        out->write_ms = write_ms;
    }
};

struct SortResident {
    enum Ev { EV_S0 = 0, EV_S1, EV_G0, EV_G1, EV_I0, EV_I1, EV_B0, EV_B1, EV_N };

    int device = 0;
    uint32_t bgzf_effort = 0; // the context's (ngsq_bgzf_set_effort): what the sink's encoder runs at
    hipStream_t st = nullptr;
    // phase 1 fills these: record i of the input lies at d_addr[i], d_len[i] bytes, with the key d_key[i]
    DevArray<uint64_t> d_addr, d_key;
    DevArray<uint32_t> d_len;
    std::vector<std::unique_ptr<DevArray<uint8_t>>> slabs; // the records: a slab is filled from its front and never moved
    uint64_t slab_used = 0;
    uint64_t records = 0, rec_bytes = 0;
    uint64_t budget = 0; // what resident_bytes() may come to
    // phases 2 and 3
    DevArray<uint64_t> d_soff;
    DevArray<uint8_t> d_piece;
    ScanScratch scan;
    SortScratch sort;
    BgzfSink z;               // d_piece's bytes become the blocks of a job
    MappedBuf hw, hw_first; // the sorted stream's length; the record every piece begins in
    HipEvents<EV_N> ev;
    uint64_t pieces = 0;
    // the file's sorted stream: its length, the piece size, and what the rounds written so far hold of it (bytes, records)
    uint64_t total = 0, piece_bytes = 0, stream_at = 0, rank_at = 0;
    const uint32_t *perm = nullptr; // order(): the resident records' sorted order
    bool over_budget = false;       // admit() refused for the budget
    double sort_ms = 0, gather_ms = 0;
    SortIndex ix;
    int code = 0;
    std::string err;
    // The drain rule (device_out.h), behind everything above: the stream is idle before the slabs, the per-record arrays, the
    // index's arrays and the sink's block buffers go.  A driver's own arrays go after this object or behind a drain of theirs.
    StreamDrain drain;

    int fail(int code_, const char *fmt, ...) {
        char buf[1024];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code = code_;
    }
#define SRHIP(expr)                                                                                  \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) return fail(NGSQ_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

    int sunk(int rc) { return rc ? fail(rc, "%s", z.err.c_str()) : rc; } // a step of the sink: its message becomes this object's

    // the device (made current), the stream the drivers' kernels run on, the events, the word the host reads
    int begin(int device_, hipStream_t stream, uint32_t bgzf_effort_) {
        device = device_;
        bgzf_effort = bgzf_effort_;
        SRHIP(hipSetDevice(device));
        st = drain.s = stream;
        SRHIP(hw.reserve(sizeof(unsigned long long)));
        memset(hw.h, 0, sizeof(unsigned long long));
        for (auto &e : ev.e) SRHIP(hipEventCreate(&e));
        return NGSQ_OK;
    }
    // the budget of a call that names none: what is free on the device now, less SORT_DEVICE_RESERVE
    int default_budget() {
        size_t free_b = 0, total_b = 0;
        SRHIP(hipMemGetInfo(&free_b, &total_b));
        budget = free_b > SORT_DEVICE_RESERVE ? free_b - SORT_DEVICE_RESERVE : 0;
        return NGSQ_OK;
    }
    void elapsed(int a, int b, double *sum) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.e[a], ev.e[b]) == hipSuccess) *sum += ms;
    }

    // Room for `bytes` more record bytes whose first lies at an address of residue `residue` modulo 16 (residue > 15: anywhere):
    // behind the newest slab's records, or at the front of a new slab of slab_bytes (or of what these records need).
    int place(uint64_t bytes, uint64_t slab_bytes, uint32_t residue, uint8_t **dst) {
        auto pad_at = [&](const uint8_t *p) { return residue > 15u ? 0u : (residue - (uint32_t)((uintptr_t)p & 15u)) & 15u; };
        uint32_t pad = slabs.empty() ? 0 : pad_at(slabs.back()->p + slab_used);
        if (slabs.empty() || slab_used + pad + bytes + SORT_GATHER_SLACK > slabs.back()->cap) {
            slabs.emplace_back(new DevArray<uint8_t>());
            SRHIP(slabs.back()->reserve(std::max(slab_bytes, bytes) + (residue > 15u ? 0u : 15u) + SORT_GATHER_SLACK));
            slab_used = 0;
            pad = pad_at(slabs.back()->p);
        }
        *dst = slabs.back()->p + slab_used + pad;
        slab_used += pad + bytes;
        return NGSQ_OK;
    }
    // the three per-record arrays with room for n records, their contents kept
    int reserve_records(uint64_t n) {
        SRHIP(d_addr.reserve_keep(n, st));
        SRHIP(d_len.reserve_keep(n, st));
        SRHIP(d_key.reserve_keep(n, st));
        return NGSQ_OK;
    }
    // Phase 1 asks for n more records of `bytes` bytes (ctx: the driver's message prefix): refused beyond the sort's index
    // width or the budget; else *dst is where they go (place) and the per-record arrays have room for them.  The driver
    // queues what fills them and then adds n and bytes to `records` and `rec_bytes`.
    int admit(uint64_t n, uint64_t bytes, uint64_t slab_bytes, uint32_t residue, const char *ctx, uint8_t **dst) {
        if (records + n > 0xFFFFFFFFull) return fail(NGSQ_ERR_LIMIT, "%s--sort coordinate sorts at most 2^32 - 1 records", ctx);
        const uint64_t need = rec_bytes + bytes + (records + n) * SORT_BYTES_PER_RECORD;
        if ((over_budget = need > budget))
            return fail(NGSQ_ERR_LIMIT, "%s--sort coordinate holds the records in device memory: %llu bytes needed, %llu allowed", ctx,
                        (unsigned long long)need, (unsigned long long)budget);
        if (const int rc = place(bytes, slab_bytes, residue, dst)) return rc;
        return reserve_records(records + n);
    }

    // the time of the last append to the block table, once the stream has passed it
    void add_append_time() {
        if (ix.append_pending) elapsed(EV_B0, EV_B1, &ix.ms.blocks_ms);
        ix.append_pending = false;
    }

    // The index pass: tiles of the sorted order through k_bai_sorted, the scan and the gather, the carry
    // from tile to tile, then k_bai_finish.  Positions are offsets in the sorted stream plus one.  In three steps, so that a file
    // sorted in rounds (section 22.3) runs the tiles of every round between one beginning and one end: the tables, the carry and
    // the run list stay from round to round.
    int index_begin() {
        if (ix.begun) return NGSQ_OK;
        SRHIP(ix.T.create(ix.ref_lens.data(), (uint32_t)ix.ref_lens.size(), 1, st));
        ix.begun = true;
        return NGSQ_OK;
    }
    // the resident records in the order perm, behind rank_at records and stream_at bytes of the sorted stream
    int index_tiles() {
        BaiTables &T = ix.T;
        SRHIP(hipEventRecord(ev.e[EV_I0], st));
        if (const int rc = index_begin()) return rc;
        const uint64_t tile = ix.tile_records ? ix.tile_records : SORT_INDEX_TILE;
        for (uint64_t k0 = 0; k0 < records; k0 += tile) {
            const uint64_t n = std::min(tile, records - k0);
            SRHIP(ix.d_flag.reserve(n + 1));
            SRHIP(ix.d_tmp.reserve(n));
            SRHIP(ix.d_runs.reserve_keep(ix.runs + n, st));
            const BaiSorted t{d_addr.p, perm, d_soff.p, k0, n, rank_at, stream_at};
            SRHIP(launch_bai_sorted(t, T.d_state, ix.parity, T.L, ix.d_flag.p, ix.d_tmp.p, st));
            SRHIP(ix.scan.exclusive_scan(ix.d_flag.p, n + 1, st));
            SRHIP(launch_bai_gather(ix.d_flag.p, ix.d_tmp.p, n, ix.d_runs.p, ix.runs, T.host_count, st));
            SRHIP(hipStreamSynchronize(st)); // (the run list grows by what the tile gave it)
            ix.runs = T.pin_h[0];
            ix.parity ^= 1u;
        }
        SRHIP(hipEventRecord(ev.e[EV_I1], st));
        SRHIP(hipStreamSynchronize(st));
        elapsed(EV_I0, EV_I1, &ix.ms.pass_ms);
        return NGSQ_OK;
    }
    // behind the last tile.  A record the BAI cannot hold is refused here; for a file in one round, before the writer starts.
    int index_end() {
        BaiTables &T = ix.T;
        SRHIP(hipEventRecord(ev.e[EV_I0], st));
        SRHIP(launch_bai_finish(T.L, T.d_state, ix.parity, T.host_fin, st));
        SRHIP(hipEventRecord(ev.e[EV_I1], st));
        SRHIP(hipStreamSynchronize(st));
        elapsed(EV_I0, EV_I1, &ix.ms.pass_ms);
        const unsigned long long *fin = T.fin();
        // (the order check of `ngs index`, kept as a check of the sort itself)
        if (fin[0] != ~0ull)
            return fail(NGSQ_ERR_STATE, "%srecord %llu (0-based) of the sorted output is out of coordinate order", ix.ctx.c_str(), fin[0]);
        if (fin[1] != ~0ull) return limit_refused(fin[1]);
        return NGSQ_OK;
    }
    int limit_refused(uint64_t rank) {
        return fail(NGSQ_ERR_LIMIT, "%srecord %llu (0-based) of the sorted output %s", ix.ctx.c_str(), (unsigned long long)rank, BAI_LIMIT_TEXT);
    }

    // Behind the last piece: the run starts and the filled windows become virtual positions through the block table, and come
    // to the host.  (Every piece has been handed over: z.enc.comp_bytes is where the EOF block will lie.)
    int index_translate(uint64_t piece_bytes, uint64_t total) {
        BaiTables &T = ix.T;
        add_append_time();
        const BaiBlocks B{ix.d_table.p, piece_bytes, ix.blocks_per_piece, total, z.enc.comp_bytes};
        SRHIP(hipEventRecord(ev.e[EV_I0], st));
        SRHIP(launch_bai_translate(B, ix.d_runs.p, ix.runs, T.d_lin.p, T.n_win, st));
        SRHIP(hipEventRecord(ev.e[EV_I1], st));
        ix.R.resize(ix.runs);
        ix.lin.resize(T.n_win);
        if (ix.runs) SRHIP(hipMemcpyAsync(ix.R.data(), ix.d_runs.p, ix.runs * sizeof(BaiRun), hipMemcpyDeviceToHost, st));
        if (T.n_win) SRHIP(hipMemcpyAsync(ix.lin.data(), T.d_lin.p, T.n_win * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        SRHIP(hipStreamSynchronize(st));
        elapsed(EV_I0, EV_I1, &ix.ms.translate_ms);
        ix.final_end = z.enc.comp_bytes << 16;
        return NGSQ_OK;
    }

    // bytes of d_piece, filled before EV_G1, through the sink (acquired by the caller); table (optional): the job's block
    // offsets in the file go there, behind the hand-over.  (To run the encoder beside the next gather, part launch from
    // hand_over here and give the pieces two buffers: DESIGN.md sections 19.5 and 20.5.)
    int compress_and_push(uint64_t bytes, uint64_t *table = nullptr) {
        uint64_t file_at = 0;
        if (sunk(z.launch(d_piece.p, bytes, st)) || sunk(z.hand_over(bytes, ev.e[EV_G1], &file_at))) return code;
        add_append_time(); // (the last job's append lies in front of this encoder)
        if (table) {
            SRHIP(hipEventRecord(ev.e[EV_B0], st));
            SRHIP(launch_bai_blocks(z.enc.sc.off.p, deflate_blocks(bytes), file_at, table, st));
            SRHIP(hipEventRecord(ev.e[EV_B1], st));
            ix.append_pending = true;
        }
        return NGSQ_OK;
    }

    // Phases 2 and 3 in steps.  order() and write_round() are a round's: the records resident now are
    // the next rec_bytes bytes of the file's sorted stream.  write_begin() and write_end() are the file's.  A file in one round is
    // sort_and_write below; bamsort.cpp's rounds begin the file once the survey knows its length, then run round after round.

    // the order of the resident records and their offsets behind stream_at; with the index on, its tiles over them
    int order() {
        perm = nullptr;
        if (records) {
            SRHIP(hipEventRecord(ev.e[EV_S0], st));
            SRHIP(sort_pairs_u64(d_key.p, records, sort, st, &perm));
            SRHIP(d_soff.reserve(records + 1));
            SRHIP(launch_sort_lengths(d_len.p, perm, records, d_soff.p, st));
            SRHIP(scan.exclusive_scan(d_soff.p, records + 1, st));
            SRHIP(launch_samtext_word(d_soff.p, records, static_cast<unsigned long long *>(hw.dev), st));
            SRHIP(hipEventRecord(ev.e[EV_S1], st));
            SRHIP(hipStreamSynchronize(st));
            elapsed(EV_S0, EV_S1, &sort_ms);
            const uint64_t sorted = *static_cast<const unsigned long long *>(hw.h);
            if (sorted != rec_bytes)
                return fail(NGSQ_ERR_STATE, "the sorted records take %llu bytes, the parsed ones %llu", (unsigned long long)sorted, (unsigned long long)rec_bytes);
        }
        return ix.on ? index_tiles() : NGSQ_OK;
    }
    // This order, no sort (`ngs markdup`): the m records order_[0, m) of the resident ones, in that order,
    // are the stream's next bytes.  *bytes receives what they take; write_records(m, *bytes) writes them.
    int order_given(const uint32_t *order_, uint64_t m, uint64_t *bytes) {
        perm = order_;
        *bytes = 0;
        if (!m) return NGSQ_OK;
        SRHIP(d_soff.reserve(m + 1));
        SRHIP(launch_sort_lengths(d_len.p, perm, m, d_soff.p, st));
        SRHIP(scan.exclusive_scan(d_soff.p, m + 1, st));
        SRHIP(launch_samtext_word(d_soff.p, m, static_cast<unsigned long long *>(hw.dev), st));
        SRHIP(hipStreamSynchronize(st));
        *bytes = *static_cast<const unsigned long long *>(hw.h);
        return NGSQ_OK;
    }
    // the writer, and the header stream hs in front of a sorted stream of `stream_bytes` bytes cut into pieces of piece_bytes_
    int write_begin(int fd, const std::string &hs, uint64_t piece_bytes_, uint64_t stream_bytes) {
        piece_bytes = piece_bytes_;
        total = stream_bytes;
        pieces = (total + piece_bytes - 1) / piece_bytes;
        if (pieces >= 0x7FFFFFFFull) return fail(NGSQ_ERR_LIMIT, "writing BAM record: more than 2^31 - 2 pieces of %llu bytes", (unsigned long long)piece_bytes);
        if (ix.on) {
            ix.blocks_per_piece = deflate_blocks(piece_bytes);
            SRHIP(ix.d_table.reserve(pieces * ix.blocks_per_piece + 1));
        }
        if (sunk(z.start(fd, device, bgzf_effort))) return code;
        // the header's blocks, in front of the first record (as samtools writes them)
        SRHIP(d_piece.reserve(std::max<uint64_t>(hs.size(), std::min(piece_bytes, total)) + DEFLATE_IN_SLACK));
        SRHIP(hipMemcpyAsync(d_piece.p, hs.data(), hs.size(), hipMemcpyHostToDevice, st));
        SRHIP(hipEventRecord(ev.e[EV_G1], st));
        return compress_and_push(hs.size());
    }
    // The resident records to their places in the pieces.  Piece j is bytes [j * piece_bytes, (j + 1) * piece_bytes) of the file's
    // sorted stream, whatever round they come from: a piece this round leaves partly filled stays in d_piece, the next round's
    // gather continues behind it, and it is compressed when it is full or the stream ends.
    int write_round() { return write_records(records, rec_bytes); }
    // write_round for an order of the caller's (order_given): the `n` records of perm, `bytes` bytes, are the stream's next
    int write_records(uint64_t n, uint64_t bytes) {
        if (!n) return NGSQ_OK;
        const uint64_t records = n, rec_bytes = bytes; // (what the round writes, in the names the round's steps use)
        const uint64_t begin = stream_at, end = begin + rec_bytes;
        if (end > total) return fail(NGSQ_ERR_STATE, "the rounds' records take more than the %llu bytes of the sorted stream", (unsigned long long)total);
        const uint64_t j0 = begin / piece_bytes, j1 = (end + piece_bytes - 1) / piece_bytes;
        SRHIP(hw_first.reserve((j1 - j0 + 1) * sizeof(unsigned long long)));
        SRHIP(launch_sort_bisect(d_soff.p, records, piece_bytes, j0, begin, j1 - j0, static_cast<unsigned long long *>(hw_first.dev), st));
        SRHIP(hipStreamSynchronize(st));
        const unsigned long long *first = static_cast<const unsigned long long *>(hw_first.h); // the record every piece begins in
        for (uint64_t j = j0; j < j1 && !z.w.failed(); j++) {
            const uint64_t lo = j * piece_bytes, hi = std::min(lo + piece_bytes, total);
            const uint64_t glo = std::max(lo, begin), ghi = std::min(hi, end); // what this round has of the piece
            // records first[j] .. first[j + 1]: the last of them may begin in this piece and end in the next
            const uint64_t a = first[j - j0], b = std::min<uint64_t>(first[j - j0 + 1] + 1, records);
            if (sunk(z.acquire())) return code;
            SRHIP(hipEventRecord(ev.e[EV_G0], st));
            SRHIP(launch_sort_gather(d_addr.p, perm, d_soff.p, a, b, glo - begin, ghi - begin, d_piece.p + (glo - lo), st));
            SRHIP(hipEventRecord(ev.e[EV_G1], st));
            if (ghi == hi) {
                if (const int rc = compress_and_push(hi - lo, ix.on ? ix.d_table.p + j * ix.blocks_per_piece : nullptr)) return rc;
            } else {
                SRHIP(hipStreamSynchronize(st)); // (the piece waits for the next round's records)
            }
            elapsed(EV_G0, EV_G1, &gather_ms);
        }
        stream_at = end;
        rank_at += records;
        return NGSQ_OK;
    }
    // behind the last round: with the index on, the translation
    int write_end() {
        SRHIP(hipStreamSynchronize(st));
        if (!z.w.failed() && stream_at != total)
            return fail(NGSQ_ERR_STATE, "the rounds' records take %llu bytes of a sorted stream of %llu", (unsigned long long)stream_at, (unsigned long long)total);
        if (ix.on && !z.w.failed())
            if (const int rc = index_translate(piece_bytes, total)) return rc;
        return NGSQ_OK;
    }
    // the records of a round are written: the slabs go, the per-record arrays stay for the next round's
    int round_reset() {
        SRHIP(hipStreamSynchronize(st));
        slabs.clear();
        slab_used = 0;
        records = rec_bytes = 0;
        return NGSQ_OK;
    }

    // phases 2 and 3 of a file in one round: the order, then the header stream hs, then the pieces, to fd
    int sort_and_write(int fd, const std::string &hs, uint64_t piece_bytes_) {
        if (const int rc = order()) return rc;
        if (ix.on)
            if (const int rc = index_end()) return rc;
        if (const int rc = write_begin(fd, hs, piece_bytes_, rec_bytes)) return rc;
        if (const int rc = write_round()) return rc;
        return write_end();
    }
#undef SRHIP

    // The end of a call whose phases gave rc (a driver's own failure: this object's `err` is not set and stays so): the sink's
    // end, then the index file.
    int finish(int rc, int fd) {
        const int before = rc;
        rc = z.end(rc, fd);
        if (rc != before) sunk(rc);
        // the index, once the file it describes is complete: beside its place and renamed (bai.cpp's writer)
        if (rc == NGSQ_OK && ix.on) {
            const double t0 = now_ms();
            const std::string m = bai_write_file(ix.path.c_str(), ix.T, ix.R, ix.lin, rank_at, ix.final_end, &ix.counts);
            ix.write_ms = now_ms() - t0;
            if (!m.empty()) rc = fail(NGSQ_ERR_INVALID_ARGUMENT, "%s", m.c_str());
        }
        return rc;
    }
    uint64_t resident_bytes() const { return rec_bytes + records * SORT_BYTES_PER_RECORD; }
    // the fields the two drivers' reports share by name
    template <class Report> void report(Report *out) const {
        out->records = records;
        out->bam_bytes = z.bam_bytes;
        out->compressed_bytes = z.enc.comp_bytes;
        out->pieces = pieces;
        out->blocks = z.enc.blocks;
        out->stored_blocks = z.enc.stored;
        out->resident_bytes = resident_bytes();
        out->passes_run = sort.passes_run;
        out->passes_skipped = SORT_DIGITS - sort.passes_run; // (no records: no pass, as ngsq_sort_u64_device reports it)
        out->sort_ms = sort_ms;
        out->gather_ms = gather_ms;
        out->deflate_ms = z.deflate_ms;
        out->d2h_ms = z.w.copy_ms;
        out->write_ms = z.w.write_ms;
    }
};

} // namespace ngsq
