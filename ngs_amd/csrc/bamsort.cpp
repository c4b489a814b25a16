// bamsort.cpp -- include/ngsq_bamsort.h: `ngs convert --gzip device --sort coordinate <BAM> <BAM>`.  Three
// phases on one GPU.  (1) The batch walk of the device ingest that sam.cpp and bai.cpp use: the records of a batch are one byte
// range of the ingest's view, k_sort_keep copies that range into a slab of device memory and leaves every record's address,
// length and key behind.  The admission of a batch to the slabs, phases (2) and (3) and the shared fields of the report are
// sort_resident.h's, shared with samsort.cpp.  The whole input is walked before the writer starts, so every fault of the file is
// known before the first byte is written.  The host reads two words per batch and a few per piece and never walks a record.
// ngsq_bam_write_sorted_bam_rounds (section 22) goes on where the records do not fit the budget: the file is walked again, a
// survey walk that keeps a key and a length per record and cuts the sorted order into ranges that fit, then one walk per range
// ("round") that keeps that range's records only; the rounds continue one stream of pieces, so the file is the one above.
#include "../../include/ngsq_bamsort.h"

#include <sys/stat.h>

#include "ingest_consumer.h"
#include "samtext_host.h" // sorted_header_text, put32
#include "sort_resident.h"

using namespace ngsq;

namespace {

constexpr uint64_t BATCH_RECORDS = (uint64_t)1 << 22;
constexpr const char *READ_CTX = "reading BAM record: ";

// the ingest's message behind the context
int read_failed(int rc) {
    const std::string m = ngsq_bam_last_error();
    return ngsq_bam_fail(rc, "%s%s", READ_CTX, m.c_str());
}

// a round of the plan: sorted ranks [first, end), whose records take `bytes`, are those with lo <= (key, input ordinal) < hi
struct Round {
    uint64_t first, end, bytes;
    SortBound lo, hi;
};

// the survey's device arrays (SORT_SURVEY_BYTES_PER_RECORD counts them): they go before round 0 begins
struct Survey {
    DevArray<uint64_t> d_key;
    DevArray<uint32_t> d_len;
    DevArray<unsigned long long> d_marked;
    SortScratch sort;
    ScanScratch scan;
};

// the three entries; bai_path: nullptr, or where the index of the file goes; in_rounds: beyond the
// budget the file is sorted in rounds (section 22), and rounds_out (optional) says how
int write_sorted(ngsq_bam *b, ngsq_ctx *c, int fd, uint64_t max_records, uint64_t batch_records, uint64_t piece_bytes, uint64_t max_resident_bytes,
                 ngsq_bamsort_report *out, const char *bai_path, uint64_t index_tile_records, ngsq_index_report *index_out, bool in_rounds,
                 ngsq_bamsort_rounds *rounds_out) {
    if (out) memset(out, 0, sizeof *out);
    if (rounds_out) memset(rounds_out, 0, sizeof *rounds_out);
    if (index_out) memset(index_out, 0, sizeof *index_out);
    if (!b || !c || fd < 0) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    if (const int rc = require_fresh_reader(b, "a sorted BAM file is written")) return rc;
    if (bai_path) { // (before any GPU work, and before a byte goes to fd)
        const std::string m = bai_refuse_existing(bai_path);
        if (!m.empty()) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "%s", m.c_str());
    }
    const double t_begin = now_ms();
    if (!batch_records) batch_records = BATCH_RECORDS;
    if (!piece_bytes) piece_bytes = SORT_PIECE_DEFAULT;
    piece_bytes = std::min(piece_bytes, SORT_PIECE_MAX);
    // ---- the header stream: the text rewritten, the reference list as the file holds it
    const std::string sorted_text = sorted_header_text(b->header_text.data(), b->header_text.size());
    if (sorted_text.size() > 0x7FFFFFFFull) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "%sheader text longer than 2^31 - 1 bytes", READ_CTX);
    std::string hs("BAM\1", 4);
    put32(hs, (uint32_t)sorted_text.size());
    hs += sorted_text;
    hs += b->ref_table;

    hipStream_t st = c->stream;
    HipEvents<2> ev; // around a batch's k_sort_keep
    MappedBuf span;  // where a batch's records lie in the view: two words the host reads
    DevArray<uint64_t> d_cnt, d_off; // a round's walk: which records of a batch it keeps, and where they go
    ScanScratch keep_scan;
    SortResident R;  // the slabs, the per-record arrays, phases 2 and 3; behind `span`: its drain of st runs before the words go
    if (bai_path) R.ix.enable(bai_path, READ_CTX, index_tile_records, b->ref_lens); // the binary reference lengths
    R.budget = max_resident_bytes;
    uint64_t batches = 0, slab_bytes = 0, view_bytes = 0;
    uint64_t walks = 0, n_rounds = 1, survey_bytes = 0, total_records = 0, max_resident = 0, max_slabs = 0;
    uint32_t survey_passes = 0;
    double scan_ms = 0, keep_ms = 0, survey_ms = 0;
    bool keep_pending = false; // the last batch's bracket has not been added to keep_ms yet
    auto add_keep_time = [&]() {
        float ms = 0;
        if (keep_pending && hipEventElapsedTime(&ms, ev.e[0], ev.e[1]) == hipSuccess) keep_ms += ms;
        keep_pending = false;
    };

    // A further walk of the same handle, from the file's first record: `ngs view`'s range walk over the whole file, which hands
    // out the batches of the whole-file walk (its range ends at the file's end: no block is another range's).  The rounds entry
    // begins its first walk this way too, so that the handle takes the next one.
    auto walk_begin = [&]() -> int {
        struct stat sb;
        if (stat(b->path.c_str(), &sb) != 0) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "%scannot stat %s", READ_CTX, b->path.c_str());
        if (const int rc = ngsq_bam_range_begin(b, c, 0, (uint64_t)sb.st_size << 16)) return read_failed(rc);
        walks++;
        return NGSQ_OK;
    };
    // the next batch of a walk that has handed out `seen` records (n = 0: its end)
    auto next_batch = [&](uint64_t seen, ngsq_batch *bt, BatchOrigin *o, uint64_t *n) -> int {
        *n = 0;
        const uint64_t left = max_records ? max_records - seen : ~0ull;
        if (!left) return NGSQ_OK;
        const double s0 = now_ms();
        const int rc = next_batch_with_origin(b, c, std::min(batch_records, left), bt, o);
        scan_ms += now_ms() - s0;
        if (rc) return read_failed(rc);
        *n = bt->n_records;
        return NGSQ_OK;
    };

    // phase 1: every batch's records copied into a slab, nothing compressed.  (R's failures leave their message in R.err.)
    auto keep_all = [&]() -> int {
        if (const int rc = R.begin(c->device, st, c->bgzf_effort)) return rc;
        for (auto &e : ev.e) BHIP(hipEventCreate(&e));
        BHIP(span.reserve(SP_WORDS * sizeof(unsigned long long)));
        const unsigned long long *const sp = static_cast<const unsigned long long *>(span.h);
        if (in_rounds) {
            if (const int rc = walk_begin()) return rc;
        } else {
            walks++;
        }
        for (;;) {
            const uint64_t left = max_records ? max_records - R.records : ~0ull;
            if (!left) break;
            // (what reads the previous batch's view, k_sort_keep, has been queued on the context's stream: the reader may reuse it)
            ngsq_batch bt;
            BatchOrigin o;
            const double s0 = now_ms();
            const int rc = next_batch_with_origin(b, c, std::min(batch_records, left), &bt, &o);
            scan_ms += now_ms() - s0;
            if (rc) return read_failed(rc);
            const uint64_t n = bt.n_records;
            if (!n) break;
            add_keep_time(); // (the ingest has waited for its own kernels, queued behind that copy)
            if (!batches) { // the reader's buffers are there: what is free now is free for the records
                uint64_t chunk_bytes = 0;
                bam_device_view_sizes(b, &chunk_bytes, &view_bytes);
                slab_bytes = std::min(std::max(2 * chunk_bytes, SORT_SLAB_MIN), SORT_SLAB_MAX);
                if (!R.budget)
                    if (const int brc = R.default_budget()) return brc;
            }
            // the batch's byte range in the view
            BHIP(launch_sort_span(o.raw, o.rec_off, n, static_cast<unsigned long long *>(span.dev), st));
            BHIP(hipStreamSynchronize(st));
            const uint64_t begin = sp[0], end = sp[1];
            if (begin >= end || end > view_bytes)
                return ngsq_bam_fail(NGSQ_ERR_STATE, "%sthe records of batch %llu lie at [%llu, %llu) of a view of %llu bytes", READ_CTX,
                                     (unsigned long long)batches, (unsigned long long)begin, (unsigned long long)end, (unsigned long long)view_bytes);
            const uint64_t bytes = end - begin;
            // the records stay: behind the last batch's in the newest slab, at the source's residue modulo 16, or in a new slab
            uint8_t *dst = nullptr;
            if (const int arc = R.admit(n, bytes, slab_bytes, (uint32_t)((uintptr_t)(o.raw + begin) & 15u), READ_CTX, &dst)) return arc;
            BHIP(hipEventRecord(ev.e[0], st));
            BHIP(launch_sort_keep(o.raw, o.rec_off, n, begin, bytes, dst, R.records, R.d_addr.p, R.d_len.p, R.d_key.p, st));
            BHIP(hipEventRecord(ev.e[1], st));
            keep_pending = true;
            R.rec_bytes += bytes;
            R.records += n;
            batches++;
        }
        BHIP(hipStreamSynchronize(st));
        add_keep_time();
        return NGSQ_OK;
    };

    // The survey walk: a key and a length per record at its input ordinal, their sort, the whole file's
    // sorted offsets, and the plan: consecutive ranges of the sorted order that each fit the budget.
    std::vector<Round> plan;
    auto survey = [&]() -> int {
        const double t0 = now_ms();
        Survey S;
        StreamDrain drain{st, false}; // (behind the arrays: it runs first)
        unsigned long long *const sp_dev = static_cast<unsigned long long *>(span.dev);
        const unsigned long long *const sp = static_cast<const unsigned long long *>(span.h);
        if (R.ix.on)
            if (const int rc = R.index_begin()) return rc;
        if (const int rc = walk_begin()) return rc;
        uint64_t seen = 0;
        batches = 0;
        for (;;) {
            ngsq_batch bt;
            BatchOrigin o;
            uint64_t n = 0;
            if (const int rc = next_batch(seen, &bt, &o, &n)) return rc;
            if (!n) break;
            if (seen + n > 0xFFFFFFFFull) return ngsq_bam_fail(NGSQ_ERR_LIMIT, "%s--sort coordinate sorts at most 2^32 - 1 records", READ_CTX);
            const uint64_t need = (seen + n) * SORT_SURVEY_BYTES_PER_RECORD;
            if (need > R.budget)
                return ngsq_bam_fail(NGSQ_ERR_LIMIT, "%s--sort coordinate in rounds holds a key per record in device memory: %llu bytes needed, %llu allowed",
                                     READ_CTX, (unsigned long long)need, (unsigned long long)R.budget);
            BHIP(S.d_key.reserve_keep(seen + n + 1, st)); // (one more: the offsets may come to lie here)
            BHIP(S.d_len.reserve_keep(seen + n, st));
            BHIP(launch_sort_survey(o.raw, o.rec_off, n, seen, S.d_len.p, S.d_key.p, st));
            // (the index on: the record's end by the index pass's own rule, so that its refusal comes before the first byte)
            if (R.ix.on) BHIP(launch_bai_survey(o.raw, o.rec_off, n, seen, R.ix.T.L, SORT_SURVEY_MARK, S.d_len.p, st));
            seen += n;
            batches++;
        }
        total_records = seen;
        survey_bytes = seen * SORT_SURVEY_BYTES_PER_RECORD;
        if (!seen) return ngsq_bam_fail(NGSQ_ERR_STATE, "%sthe input changed between walks: no record in the survey walk", READ_CTX);
        const uint32_t *perm = nullptr;
        BHIP(S.sort.keys_b.reserve(seen + 1)); // (the sort's second half, with room for the offsets)
        BHIP(sort_pairs_u64(S.d_key.p, seen, S.sort, st, &perm));
        survey_passes = S.sort.passes_run;
        // the sorted keys lie in the half of the ping-pong the last pass wrote; the sorted offsets go to the other half
        const bool in_b = S.sort.passes_run & 1u;
        const uint64_t *skey = in_b ? S.sort.keys_b.p : S.d_key.p;
        uint64_t *const soff = in_b ? S.d_key.p : S.sort.keys_b.p;
        BHIP(S.d_marked.reserve(1));
        BHIP(launch_sort_survey_lengths(S.d_len.p, perm, seen, soff, S.d_marked.p, st));
        BHIP(S.scan.exclusive_scan(soff, seen + 1, st));
        unsigned long long marked = ~0ull;
        BHIP(hipMemcpyAsync(&marked, S.d_marked.p, sizeof marked, hipMemcpyDeviceToHost, st));
        BHIP(hipStreamSynchronize(st));
        if (marked != ~0ull) return R.limit_refused(marked);
        for (uint64_t first = 0; first < seen;) {
            BHIP(launch_sort_plan(soff, skey, perm, seen, first, R.budget, SORT_BYTES_PER_RECORD, sp_dev, st));
            BHIP(hipStreamSynchronize(st));
            const uint64_t end = sp[SP_END];
            if (end == first)
                return ngsq_bam_fail(NGSQ_ERR_LIMIT, "%srecord %llu (0-based) of the sorted output alone takes %llu bytes of device memory, %llu allowed",
                                     READ_CTX, (unsigned long long)first, (unsigned long long)(sp[SP_FIRST_LEN] + SORT_BYTES_PER_RECORD),
                                     (unsigned long long)R.budget);
            Round r;
            r.first = first;
            r.end = end;
            r.lo = plan.empty() ? SortBound{0, 0} : plan.back().hi;
            r.hi = SortBound{sp[SP_KEY], sp[SP_ORD]};
            r.bytes = sp[SP_END_OFF]; // (the offset behind the round; made the round's bytes below)
            plan.push_back(r);
            first = end;
        }
        R.total = plan.back().bytes;
        for (size_t k = plan.size(); k-- > 1;) plan[k].bytes -= plan[k - 1].bytes;
        survey_ms = now_ms() - t0;
        return NGSQ_OK;
    };

    // One round: a walk that keeps the records inside the round's two boundaries, compacted in input order; then their order,
    // and their bytes behind the last round's in the pieces.
    auto round = [&](size_t k) -> int {
        const Round &r = plan[k];
        unsigned long long *const sp_dev = static_cast<unsigned long long *>(span.dev);
        const unsigned long long *const sp = static_cast<const unsigned long long *>(span.h);
        if (const int rc = walk_begin()) return rc;
        uint64_t seen = 0;
        for (;;) {
            ngsq_batch bt;
            BatchOrigin o;
            uint64_t n = 0;
            if (const int rc = next_batch(seen, &bt, &o, &n)) return rc;
            if (!n) break;
            add_keep_time();
            BHIP(d_cnt.reserve(n + 1));
            BHIP(d_off.reserve(n + 1));
            BHIP(launch_sort_round_flag(o.raw, o.rec_off, n, seen, r.lo, r.hi, d_cnt.p, d_off.p, st));
            BHIP(keep_scan.exclusive_scan(d_cnt.p, n + 1, st));
            BHIP(keep_scan.exclusive_scan(d_off.p, n + 1, st));
            BHIP(launch_samtext_word(d_cnt.p, n, sp_dev, st));
            BHIP(launch_samtext_word(d_off.p, n, sp_dev + 1, st));
            BHIP(hipStreamSynchronize(st));
            const uint64_t kept = sp[0], bytes = sp[1];
            seen += n;
            if (!kept) continue; // (nothing of this round's in the batch)
            if (R.records + kept > r.end - r.first || R.rec_bytes + bytes > r.bytes) break; // (more than the plan: reported below)
            uint8_t *dst = nullptr;
            if (const int arc = R.admit(kept, bytes, slab_bytes, 16u, READ_CTX, &dst)) return arc;
            BHIP(hipEventRecord(ev.e[0], st));
            BHIP(launch_sort_take(o.raw, o.rec_off, n, d_cnt.p, d_off.p, dst, R.records, R.d_addr.p, R.d_len.p, R.d_key.p, st));
            BHIP(hipEventRecord(ev.e[1], st));
            keep_pending = true;
            R.rec_bytes += bytes;
            R.records += kept;
        }
        BHIP(hipStreamSynchronize(st));
        add_keep_time();
        if (R.records != r.end - r.first || R.rec_bytes != r.bytes || seen != total_records)
            return ngsq_bam_fail(NGSQ_ERR_STATE,
                                 "%sthe input changed between walks: round %llu found %llu records of %llu bytes among %llu, the survey %llu of %llu among %llu",
                                 READ_CTX, (unsigned long long)k, (unsigned long long)R.records, (unsigned long long)R.rec_bytes, (unsigned long long)seen,
                                 (unsigned long long)(r.end - r.first), (unsigned long long)r.bytes, (unsigned long long)total_records);
        max_resident = std::max(max_resident, R.resident_bytes());
        max_slabs = std::max<uint64_t>(max_slabs, R.slabs.size());
        if (const int rc = R.order()) return rc;
        if (const int rc = R.write_round()) return rc;
        return R.round_reset();
    };

    // The first attempt overflowed: what it kept goes, and the file is walked from its beginning again (section 22.2: the
    // restart costs at most one budget's worth of copies, and keeps the path that fits free of the survey).
    auto rounds = [&]() -> int {
        R.err.clear();
        R.code = 0;
        R.over_budget = false;
        if (const int rc = R.round_reset()) return rc;
        if (const int rc = survey()) return rc;
        n_rounds = plan.size();
        const uint64_t stream_bytes = R.total;
        if (const int rc = R.write_begin(fd, hs, piece_bytes, stream_bytes)) return rc;
        for (size_t k = 0; k < plan.size() && !R.z.w.failed(); k++)
            if (const int rc = round(k)) return rc;
        if (R.ix.on && !R.z.w.failed())
            if (const int rc = R.index_end()) return rc;
        return R.write_end();
    };

    int rc = keep_all();
    if (rc == NGSQ_OK) rc = R.sort_and_write(fd, hs, piece_bytes);
    else if (in_rounds && rc == NGSQ_ERR_LIMIT && R.over_budget) rc = rounds();
    rc = R.finish(rc, fd);
    if (rc != NGSQ_OK && !R.err.empty()) ngsq_bam_fail(rc, "%s", R.err.c_str());
    if (out) {
        R.report(out);
        out->header_bytes = sorted_text.size();
        out->batches = batches;
        out->slabs = R.slabs.size();
        out->scan_ms = scan_ms;
        out->keep_ms = keep_ms;
        out->total_ms = now_ms() - t_begin;
        if (n_rounds > 1 || survey_bytes) { // in rounds: the whole file's records, the largest round's residence, the survey's sort
            out->records = R.rank_at;
            out->slabs = max_slabs;
            out->resident_bytes = max_resident;
            out->passes_run = survey_passes;
            out->passes_skipped = SORT_DIGITS - survey_passes;
        }
    }
    if (rounds_out) {
        rounds_out->rounds = n_rounds;
        rounds_out->walks = walks;
        rounds_out->survey_records = total_records;
        rounds_out->survey_bytes = survey_bytes;
        rounds_out->budget = R.budget;
        rounds_out->survey_ms = survey_ms;
    }
    R.ix.report(R.rank_at, index_out);
    return rc;
}

} // namespace

extern "C" {

int ngsq_bam_write_sorted_bam(ngsq_bam *b, ngsq_ctx *c, int fd, uint64_t max_records, uint64_t batch_records, uint64_t piece_bytes,
                              uint64_t max_resident_bytes, ngsq_bamsort_report *out) {
    return write_sorted(b, c, fd, max_records, batch_records, piece_bytes, max_resident_bytes, out, nullptr, 0, nullptr, false, nullptr);
}

int ngsq_bam_write_sorted_bam_indexed(ngsq_bam *b, ngsq_ctx *c, int fd, uint64_t max_records, uint64_t batch_records, uint64_t piece_bytes,
                                      uint64_t max_resident_bytes, ngsq_bamsort_report *out, const char *bai_path, uint64_t index_tile_records,
                                      ngsq_index_report *index_out) {
    if (!bai_path) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    return write_sorted(b, c, fd, max_records, batch_records, piece_bytes, max_resident_bytes, out, bai_path, index_tile_records, index_out, false, nullptr);
}

int ngsq_bam_write_sorted_bam_rounds(ngsq_bam *b, ngsq_ctx *c, int fd, uint64_t max_records, uint64_t batch_records, uint64_t piece_bytes,
                                     uint64_t max_resident_bytes, ngsq_bamsort_report *out, const char *bai_path, uint64_t index_tile_records,
                                     ngsq_index_report *index_out, ngsq_bamsort_rounds *rounds_out) {
    return write_sorted(b, c, fd, max_records, batch_records, piece_bytes, max_resident_bytes, out, bai_path, index_tile_records, index_out, true, rounds_out);
}

void ngsq_sort_index_split(double *pass_ms, double *blocks_ms, double *translate_ms) {
    if (pass_ms) *pass_ms = g_sort_index_split.pass_ms;
    if (blocks_ms) *blocks_ms = g_sort_index_split.blocks_ms;
    if (translate_ms) *translate_ms = g_sort_index_split.translate_ms;
}

} // extern "C"
