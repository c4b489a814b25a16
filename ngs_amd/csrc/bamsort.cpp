// bamsort.cpp -- include/ngsq_bamsort.h: `ngs convert --gzip device --sort coordinate <BAM> <BAM>`.  Three
// phases on one GPU.  (1) The batch walk of the device ingest that sam.cpp and bai.cpp use: the records of a batch are one byte
// range of the ingest's view, k_sort_keep copies that range into a slab of device memory and leaves every record's address,
// length and key behind.  The admission of a batch to the slabs, phases (2) and (3) and the shared fields of the report are
// sort_resident.h's, shared with samsort.cpp.  The whole input is walked before the writer starts, so every fault of the file is
// known before the first byte is written.  The host reads two words per batch and a few per piece and never walks a record.
#include "../../include/ngsq_bamsort.h"

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

// both entries; bai_path: nullptr, or where the index of the file goes
int write_sorted(ngsq_bam *b, ngsq_ctx *c, int fd, uint64_t max_records, uint64_t batch_records, uint64_t piece_bytes, uint64_t max_resident_bytes,
                 ngsq_bamsort_report *out, const char *bai_path, uint64_t index_tile_records, ngsq_index_report *index_out) {
    if (out) memset(out, 0, sizeof *out);
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
    SortResident R;  // the slabs, the per-record arrays, phases 2 and 3; behind `span`: its drain of st runs before the words go
    if (bai_path) R.ix.enable(bai_path, READ_CTX, index_tile_records, b->ref_lens); // the binary reference lengths
    R.budget = max_resident_bytes;
    uint64_t batches = 0, slab_bytes = 0, view_bytes = 0;
    double scan_ms = 0, keep_ms = 0;
    bool keep_pending = false; // the last batch's bracket has not been added to keep_ms yet
    auto add_keep_time = [&]() {
        float ms = 0;
        if (keep_pending && hipEventElapsedTime(&ms, ev.e[0], ev.e[1]) == hipSuccess) keep_ms += ms;
        keep_pending = false;
    };

    // phase 1: every batch's records copied into a slab, nothing compressed.  (R's failures leave their message in R.err.)
    auto keep_all = [&]() -> int {
        if (const int rc = R.begin(c->device, st)) return rc;
        for (auto &e : ev.e) BHIP(hipEventCreate(&e));
        BHIP(span.reserve(2 * sizeof(unsigned long long)));
        const unsigned long long *const sp = static_cast<const unsigned long long *>(span.h);
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

    int rc = keep_all();
    if (rc == NGSQ_OK) rc = R.sort_and_write(fd, hs, piece_bytes);
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
    }
    R.ix.report(R.records, index_out);
    return rc;
}

} // namespace

extern "C" {

int ngsq_bam_write_sorted_bam(ngsq_bam *b, ngsq_ctx *c, int fd, uint64_t max_records, uint64_t batch_records, uint64_t piece_bytes,
                              uint64_t max_resident_bytes, ngsq_bamsort_report *out) {
    return write_sorted(b, c, fd, max_records, batch_records, piece_bytes, max_resident_bytes, out, nullptr, 0, nullptr);
}

int ngsq_bam_write_sorted_bam_indexed(ngsq_bam *b, ngsq_ctx *c, int fd, uint64_t max_records, uint64_t batch_records, uint64_t piece_bytes,
                                      uint64_t max_resident_bytes, ngsq_bamsort_report *out, const char *bai_path, uint64_t index_tile_records,
                                      ngsq_index_report *index_out) {
    if (!bai_path) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    return write_sorted(b, c, fd, max_records, batch_records, piece_bytes, max_resident_bytes, out, bai_path, index_tile_records, index_out);
}

void ngsq_sort_index_split(double *pass_ms, double *blocks_ms, double *translate_ms) {
    if (pass_ms) *pass_ms = g_sort_index_split.pass_ms;
    if (blocks_ms) *blocks_ms = g_sort_index_split.blocks_ms;
    if (translate_ms) *translate_ms = g_sort_index_split.translate_ms;
}

} // extern "C"
