// sam.cpp -- ngsq_bam_write_sam (include/ngsq_sam.h): the device ingest hands out the file's records batch by batch and
// sam_run.h formats and writes every one of them (the run `ngs view` shares).  The host never walks the records.
// DESIGN.md section 13.
#include "../../include/ngsq_sam.h"
#include "sam_run.h"

using namespace ngsq;

namespace {

// One batch of the device ingest, in file order.
// *more = false: that was the last one (the file's end, max_records, or a writer that has failed: its error is read at the end).
int next_batch(SamRun &r, uint64_t max_records, uint64_t batch_records, bool *more) {
    *more = false;
    const uint64_t left = max_records ? max_records - r.records : ~0ull;
    if (!left) return NGSQ_OK;
    ngsq_batch bt;
    BatchOrigin o;
    const double s0 = now_ms();
    const int rc = next_batch_with_origin(r.b, r.c, std::min(batch_records, left), &bt, &o);
    r.scan_ms += now_ms() - s0;
    if (rc) return rc;
    if (!bt.n_records) return NGSQ_OK;
    uint64_t bad = ~0ull;
    if (const int frc = r.format_batch(bt, o, nullptr, more, &bad)) return frc;
    if (bad != ~0ull)
        return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "writing SAM record: record %llu: %s", (unsigned long long)(bad >> SAM_ERR_BITS),
                             sam_error_text((uint32_t)(bad & ((1u << SAM_ERR_BITS) - 1))));
    return NGSQ_OK;
}

} // namespace

extern "C" int ngsq_bam_write_sam(ngsq_bam *b, ngsq_ctx *c, int fd, uint64_t max_records, uint64_t batch_records, ngsq_sam_report *out) {
    if (!b || !c || fd < 0) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    if (out) memset(out, 0, sizeof *out);
    if (const int rc = require_fresh_reader(b, "a SAM file is written")) return rc;
    const double t_begin = now_ms();
    // ---- the header: the text the file holds, with a final newline
    std::string head = b->header_text;
    if (!head.empty() && head.back() != '\n') head += '\n';
    if (const int e = write_all(fd, head.data(), head.size()))
        return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "writing SAM header: %s (os error %d)", strerror(e), e);
    BHIP(hipSetDevice(c->device));
    SamRun r;
    if (!batch_records) batch_records = SAM_BATCH_RECORDS;
    if (const int rc = r.begin(b, c, fd, std::min<uint64_t>(batch_records, max_records ? max_records : batch_records))) return rc;
    // ---- the scan: every batch of the device ingest, in file order
    int rc = NGSQ_OK;
    for (bool more = true; more && rc == NGSQ_OK;) rc = next_batch(r, max_records, batch_records, &more);
    rc = r.finish(rc, "writing SAM record");
    if (rc != NGSQ_OK) return rc;
    if (out) {
        out->records = r.records;
        out->header_bytes = head.size();
        out->text_bytes = r.text_bytes;
        out->batches = r.slots.jobs;
        out->scan_ms = r.scan_ms;
        out->format_ms = r.format_ms;
        out->copy_ms = r.w.copy_ms;
        out->write_ms = r.w.write_ms;
        out->total_ms = now_ms() - t_begin;
    }
    return NGSQ_OK;
}
