// view.cpp -- ngsq_bam_query_chunks and ngsq_bam_view (include/ngsq_view.h): the query is parsed and its
// chunks are taken from the BAI on the host (view_query.cpp); chunks that lie close together in the file are read by one range
// walk of the device ingest (ngsq_bam_range_begin), view_kernel.hip marks the region's records of every batch, and the run
// of `ngs convert` (sam_run.h) formats and writes the marked ones.  Without a query the whole file is walked and nothing is marked.
#include "../../include/ngsq_view.h"
#include "sam_run.h"
#include "view_kernels.h"
#include "view_query.h"

using namespace ngsq;

namespace {

// merged chunks nearer than this many compressed bytes are read by one range walk: the compressed bytes of one chunk of the
// ingest's pipeline (a design constant, not a measured one: DESIGN.md section 15.4)
constexpr uint64_t COALESCE_GAP = (uint64_t)64 << 20;

int read_file(const std::string &path, std::vector<uint8_t> *out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "reading BAM index: cannot open %s: %s (os error %d)", path.c_str(), strerror(errno), errno);
    uint8_t buf[1 << 16];
    size_t g;
    while ((g = fread(buf, 1, sizeof buf, f)) > 0) out->insert(out->end(), buf, buf + g);
    const bool bad = ferror(f);
    fclose(f);
    if (bad) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "reading BAM index: read error on %s", path.c_str());
    return NGSQ_OK;
}

struct Query {
    uint32_t ref_id = 0;
    uint64_t start = 0, end = 0;
    std::vector<ngsq_view_chunk> chunks;
};

int run_query(const ngsq_bam *b, const char *bai_path, const char *query, Query *q) {
    char err[512] = "";
    // the index first, as the reference reads it in front of the query (view/bam.rs:49-50)
    std::vector<uint8_t> bai;
    if (const int rc = read_file(bai_path ? std::string(bai_path) : b->path + ".bai", &bai)) return rc;
    std::vector<const char *> names(b->ref_names.size());
    for (size_t k = 0; k < names.size(); k++) names[k] = b->ref_names[k].c_str();
    if (ngsq_vq_parse(query, names.data(), (uint32_t)names.size(), &q->ref_id, &q->start, &q->end, err, sizeof err) != NGSQ_VQ_OK)
        return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "%s", err);
    uint64_t n = 0;
    if (ngsq_vq_chunks(bai.data(), bai.size(), q->ref_id, q->start, q->end, nullptr, 0, &n, err, sizeof err) != NGSQ_VQ_OK)
        return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "%s", err);
    q->chunks.resize(n);
    if (ngsq_vq_chunks(bai.data(), bai.size(), q->ref_id, q->start, q->end, q->chunks.data(), n, &n, err, sizeof err) != NGSQ_VQ_OK)
        return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "%s", err);
    return NGSQ_OK;
}

// The view's own device state beside the formatter's.
struct ViewRun {
    SamRun r;
    DevArray<ngsq_view_chunk> d_chunks;
    DevArray<uint8_t> d_keep;
    DevArray<unsigned long long> d_kept;
    HipEvents<2> sel;
    double select_ms = 0;
    uint64_t scanned = 0, ranges = 0;
};

// The 0-based index in the file of the record at virtual offset v: the records in front of it, counted by a walk from the
// file's first record (the error path of a region query, whose walks number their records from their own beginning).
int file_index_of(ViewRun &vr, uint64_t v, uint64_t batch_records, uint64_t *index) {
    SamRun &r = vr.r;
    if (const int rc = ngsq_bam_range_begin(r.b, r.c, 0, v)) return rc;
    unsigned long long *const word = static_cast<unsigned long long *>(r.hw.dev) + 2;
    uint64_t count = 0;
    for (;;) {
        ngsq_batch bt;
        if (const int rc = ngsq_bam_next_batch_device(r.b, r.c, batch_records, &bt)) return rc;
        if (!bt.n_records) break;
        BHIP(launch_count_below_u64(bt.record_id, bt.n_records, v, word, r.st));
        BHIP(hipStreamSynchronize(r.st));
        const uint64_t below = static_cast<const unsigned long long *>(r.hw.h)[2];
        count += below;
        if (below < bt.n_records) break;
    }
    *index = count;
    return NGSQ_OK;
}

// Every batch of the walk the reader is armed for (the whole file when region is null).
int walk(ViewRun &vr, const ViewRegion *region, uint64_t batch_records, bool *more) {
    SamRun &r = vr.r;
    int rc = NGSQ_OK;
    while (*more && rc == NGSQ_OK) {
        ngsq_batch bt;
        BatchOrigin o;
        const double s0 = now_ms();
        rc = next_batch_with_origin(r.b, r.c, batch_records, &bt, &o);
        r.scan_ms += now_ms() - s0;
        if (rc || !bt.n_records) break;
        vr.scanned += bt.n_records;
        const uint8_t *keep = nullptr;
        if (region) {
            // (the formatter's write pass of the batch in front may still read keep: the stream orders the two)
            BHIP(vr.d_keep.reserve(bt.n_records));
            BHIP(hipEventRecord(vr.sel.e[0], r.st));
            BHIP(launch_view_select(bt, *region, vr.d_keep.p, vr.d_kept.p, r.st));
            BHIP(hipEventRecord(vr.sel.e[1], r.st));
            keep = vr.d_keep.p;
        }
        uint64_t bad = ~0ull;
        rc = r.format_batch(bt, o, keep, more, &bad);
        if (rc) break;
        if (region) { // (format_batch has waited for the stream)
            float ms = 0;
            if (hipEventElapsedTime(&ms, vr.sel.e[0], vr.sel.e[1]) == hipSuccess) vr.select_ms += ms;
        }
        if (bad != ~0ull) {
            uint64_t index = bad >> SAM_ERR_BITS; // in the walk
            const uint32_t code = (uint32_t)(bad & ((1u << SAM_ERR_BITS) - 1));
            if (region) {
                uint64_t v = 0;
                BHIP(hipMemcpy(&v, bt.record_id + (index - bt.first_record_index), sizeof v, hipMemcpyDeviceToHost));
                if ((rc = file_index_of(vr, v, batch_records, &index))) break;
            }
            rc = ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "writing record to stream: record %llu: %s", (unsigned long long)index, sam_error_text(code));
        }
    }
    return rc;
}

} // namespace

extern "C" int ngsq_bam_query_chunks(const ngsq_bam *b, const char *bai_path, const char *query, uint32_t *ref_id, uint64_t *start,
                                     uint64_t *end, ngsq_view_chunk *chunks, uint64_t cap, uint64_t *n) {
    if (!b || !query || !n || (cap && !chunks)) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    Query q;
    if (const int rc = run_query(b, bai_path, query, &q)) return rc;
    if (ref_id) *ref_id = q.ref_id;
    if (start) *start = q.start;
    if (end) *end = q.end;
    *n = q.chunks.size();
    for (uint64_t k = 0; k < std::min<uint64_t>(cap, q.chunks.size()); k++) chunks[k] = q.chunks[k];
    return NGSQ_OK;
}

extern "C" int ngsq_bam_view(ngsq_bam *b, ngsq_ctx *c, int fd, const char *query, const char *bai_path, uint32_t mode,
                             uint64_t batch_records, uint64_t coalesce_gap, ngsq_view_report *out) {
    if (!b || fd < 0 || mode > NGSQ_VIEW_RECORDS_ONLY || (!c && mode != NGSQ_VIEW_HEADER_ONLY))
        return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "null or invalid argument");
    if (out) memset(out, 0, sizeof *out);
    const double t_begin = now_ms();
    const std::string &head = b->header_text;
    auto write_header = [&]() -> int {
        if (const int e = write_all(fd, head.data(), head.size()))
            return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "writing BAM header to stream: %s (os error %d)", strerror(e), e);
        if (out) out->header_bytes = head.size();
        return NGSQ_OK;
    };
    if (mode == NGSQ_VIEW_HEADER_ONLY) { // (view/bam.rs:39-42: the query is never looked at)
        const int rc = write_header();
        if (out) out->total_ms = now_ms() - t_begin;
        return rc;
    }
    if (const int rc = require_fresh_reader(b, "a file is viewed")) return rc;
    // ---- the query and the device, in front of the first byte
    Query q;
    if (query)
        if (const int rc = run_query(b, bai_path, query, &q)) return rc;
    BHIP(hipSetDevice(c->device));
    if (!batch_records) batch_records = SAM_BATCH_RECORDS;
    if (!coalesce_gap) coalesce_gap = COALESCE_GAP;
    ViewRun vr;
    SamRun &r = vr.r;
    if (const int rc = r.begin(b, c, fd, batch_records)) return rc;
    ViewRegion region{};
    if (query) {
        BHIP(vr.d_chunks.reserve(q.chunks.size() + 1));
        BHIP(vr.d_kept.reserve(1));
        BHIP(hipMemsetAsync(vr.d_kept.p, 0, sizeof(unsigned long long), r.st));
        if (!q.chunks.empty())
            BHIP(hipMemcpyAsync(vr.d_chunks.p, q.chunks.data(), q.chunks.size() * sizeof(ngsq_view_chunk), hipMemcpyHostToDevice, r.st));
        BHIP(hipStreamSynchronize(r.st));
        for (auto &e : vr.sel.e) BHIP(hipEventCreate(&e));
        BHIP(vr.d_keep.reserve(batch_records));
        region.chunks = vr.d_chunks.p;
        region.n_chunks = (uint32_t)q.chunks.size();
        region.ref_id = (int32_t)q.ref_id;
        region.start = q.start;
        region.end = q.end;
    }
    int rc = NGSQ_OK;
    if (mode == NGSQ_VIEW_FULL) rc = write_header();
    // ---- the records
    bool more = rc == NGSQ_OK;
    if (rc == NGSQ_OK && !query) {
        rc = walk(vr, nullptr, batch_records, &more);
    } else if (rc == NGSQ_OK) {
        // merged chunks whose gap in the file is below coalesce_gap share a walk
        for (size_t k = 0; k < q.chunks.size() && more && rc == NGSQ_OK;) {
            size_t j = k;
            while (coalesce_gap > 1 && j + 1 < q.chunks.size() && (q.chunks[j + 1].begin >> 16) - (q.chunks[j].end >> 16) < coalesce_gap) j++;
            region.lo = q.chunks[k].begin; // (a walk hands out records behind its end, to the end of their block: the next walk's)
            region.hi = q.chunks[j].end;
            rc = ngsq_bam_range_begin(b, c, q.chunks[k].begin, q.chunks[j].end);
            if (rc == NGSQ_OK) {
                vr.ranges++;
                rc = walk(vr, &region, batch_records, &more);
            }
            k = j + 1;
        }
    }
    rc = r.finish(rc, "writing record to stream");
    if (rc != NGSQ_OK) return rc;
    uint64_t written = vr.scanned;
    if (query) {
        unsigned long long kept = 0;
        BHIP(hipMemcpy(&kept, vr.d_kept.p, sizeof kept, hipMemcpyDeviceToHost));
        written = kept;
    }
    if (out) {
        out->records_scanned = vr.scanned;
        out->records_written = written;
        out->text_bytes = r.text_bytes;
        out->chunks = q.chunks.size();
        out->ranges = vr.ranges;
        out->batches = r.slots.jobs;
        out->scan_ms = r.scan_ms;
        out->select_ms = vr.select_ms;
        out->format_ms = r.format_ms;
        out->copy_ms = r.w.copy_ms;
        out->write_ms = r.w.write_ms;
        out->total_ms = now_ms() - t_begin;
    }
    return NGSQ_OK;
}
