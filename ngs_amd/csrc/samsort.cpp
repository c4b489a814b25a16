// samsort.cpp -- include/ngsq_samtext.h: `ngs convert --gzip device --sort coordinate <SAM> <BAM>`.  Three
// phases on one GPU.  (1) The chunk parser of samtext_run.h, the one samtext.cpp runs, but the records stay where they are
// written, in slabs of device memory, and every record leaves its address, its length and its key behind: this file admits a
// chunk to the slabs, says where it goes and queues k_sort_keys behind its write pass.  (2) and (3) are sort_resident.h's, shared
// with bamsort.cpp: the sort of (key, record index) pairs, then the sorted stream in pieces through k_sort_gather and the sink
// of device_out.h, behind the header's blocks and in front of the EOF block.  Every fault of the text is known before the
// first byte is written.  The host reads a few words per chunk and per piece and never walks a record.
#include "../../include/ngsq_samtext.h"

#include "samtext_run.h"
#include "sort_resident.h"

using namespace ngsq;

namespace {

constexpr const char *READ_CTX = "reading SAM record: ";

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
    if (!piece_bytes) piece_bytes = SORT_PIECE_DEFAULT;
    piece_bytes = std::min(piece_bytes, SORT_PIECE_MAX);
    // Each of the two drains the context's stream before its own arrays go (the drain rule), and nothing is queued once the
    // first of them has gone: either order of declaration would do.
    SortResident R; // the slabs, the per-record arrays, phases 2 and 3
    SamTextRun P;   // phase 1's parser
    if (const int rc = P.open(c, sam_path, max_records, chunk_bytes)) return rc;
    const std::string sorted_text = sorted_header_text(P.H.text.data(), P.H.text.size());
    if (sorted_text.size() > 0x7FFFFFFFull) return sfail(c, NGSQ_ERR_INVALID_ARGUMENT, "%sheader text longer than 2^31 - 1 bytes", ST_OPEN_CTX);
    const std::string hs = header_stream(sorted_text, P.H);
    const uint64_t slab_bytes = std::min(std::max(8 * P.chunk_bytes, SORT_SLAB_MIN), SORT_SLAB_MAX);
    if (bai_path) R.ix.enable(bai_path, READ_CTX, index_tile_records, P.H.lens); // @SQ LN
    R.budget = max_resident_bytes;

    // phase 1: every record written into a slab, nothing compressed.  (R's failures leave their message in R.err.)
    auto parse = [&]() -> int {
        if (const int rc = R.begin(c->device, c->stream, c->bgzf_effort)) return rc;
        if (!R.budget) // (before the parser's buffers are there, as the reserve is sized)
            if (const int rc = R.default_budget()) return rc;
        if (const int rc = P.begin()) return rc;
        int refused = NGSQ_OK; // a chunk that was not admitted ends the loop; the parser still ends as after any chunk
        while (P.len) {
            if (const int rc = P.size()) return rc;
            if (P.faulty()) break;
            // the records stay: behind the last chunk's in the newest slab, or at the front of a new one
            uint8_t *dst = nullptr;
            if ((refused = R.admit(P.n, P.bytes, slab_bytes, ~0u, READ_CTX, &dst))) break;
            const auto keys = [&] { return launch_sort_keys(dst, P.d_off.p, P.n, R.records, R.d_addr.p, R.d_len.p, R.d_key.p, c->stream); };
            if (const int rc = P.write(dst, keys)) return rc;
            R.rec_bytes += P.bytes;
            R.records += P.n;
            // the next chunk is read and copied up while this one is written
            if (const int rc = P.advance()) return rc;
        }
        const int rc = P.end();
        return refused ? refused : rc;
    };

    int rc = parse();
    // the text's faults, then (phases 2 and 3) the order, the header, the pieces.  (A chunk that was refused ended the loop
    // before the next was read: a refusal never meets a fault or a long line.)
    if (rc == NGSQ_OK) rc = P.verdict();
    if (rc == NGSQ_OK) rc = R.sort_and_write(fd, hs, piece_bytes);
    rc = R.finish(rc, fd);
    if (rc != NGSQ_OK && !R.err.empty()) sfail(c, rc, "%s", R.err.c_str());
    if (out) {
        R.report(out);
        out->header_bytes = sorted_text.size();
        out->text_bytes = P.text_bytes;
        out->chunks = P.chunks;
        out->read_ms = P.text.read_ms;
        out->h2d_ms = P.h2d_ms;
        out->parse_ms = P.parse_ms;
        out->total_ms = now_ms() - t_begin;
    }
    R.ix.report(R.records, index_out);
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
