// samtext.cpp -- include/ngsq_samtext.h: `ngs convert --gzip device <SAM> <BAM>`.  Two shared parts and
// the buffer between them: the chunk parser of samtext_run.h writes a chunk's BAM records into d_rec, and the sink of
// device_out.h makes BGZF blocks of d_rec with the device DEFLATE encoder and carries them to the descriptor, behind the
// header's blocks and in front of the EOF block.  What is this file's is the order of the steps: the encoder of chunk k is
// launched, then the host reads chunk k + 1 and copies it up, then it waits for the encoder and hands the blocks over; while
// chunk k + 1 is parsed the writer copies chunk k down and writes it.
#include "../../include/ngsq_samtext.h"

#include "samtext_run.h"

using namespace ngsq;

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
    // Declaration order is the drain rule's: P, the last, goes first and leaves the context's stream idle; then Z ends its
    // writer before its block buffers go; then d_rec, which the parser's write pass and the encoder have used on that stream.
    DevArray<uint8_t> d_rec; // a chunk's records (first the header stream): what the sink compresses
    HipEvents<1> ev;         // behind the header stream's copy
    BgzfSink Z;
    SamTextRun P;
    if (const int rc = P.open(c, sam_path, max_records, chunk_bytes)) return rc;
    const std::string hs = header_stream(P.H.text, P.H);

    // every failure leaves through `rc`, so that the writer is stopped either way; the sink's messages are forwarded at the end
#define SHIP(expr)                                                                                  \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) return sfail(c, NGSQ_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
    auto run = [&]() -> int {
        hipStream_t st = c->stream;
        if (const int rc = Z.start(fd, c->device, c->bgzf_effort)) return rc; // (first: the writer pins its ring beside the first chunk's read)
        if (const int rc = P.begin()) return rc;
        // the header's blocks, in front of the first record (as samtools writes them)
        SHIP(hipEventCreate(&ev.e[0]));
        SHIP(d_rec.reserve(hs.size() + DEFLATE_IN_SLACK));
        SHIP(hipMemcpyAsync(d_rec.p, hs.data(), hs.size(), hipMemcpyHostToDevice, st));
        SHIP(hipEventRecord(ev.e[0], st));
        if (const int rc = Z.acquire()) return rc;
        if (const int rc = Z.launch(d_rec.p, hs.size(), st)) return rc;
        if (const int rc = Z.hand_over(hs.size(), ev.e[0])) return rc;
        // the chunks
        while (P.len && !Z.w.failed()) {
            if (const int rc = P.size()) return rc;
            if (P.faulty()) break;
            // the records, and their blocks
            const uint64_t bytes = P.bytes;
            SHIP(d_rec.reserve(bytes + DEFLATE_IN_SLACK));
            if (const int rc = P.write(d_rec.p)) return rc;
            if (const int rc = Z.acquire()) return rc;
            if (const int rc = Z.launch(d_rec.p, bytes, st)) return rc;
            // the next chunk is read and copied up while this one is written and compressed
            if (const int rc = P.advance()) return rc;
            if (const int rc = Z.hand_over(bytes, P.written())) return rc;
        }
        return P.end();
    };
    int rc = run();
#undef SHIP
    // the writer's errors come before the text's faults; the EOF block only behind a text without fault
    rc = Z.stop(rc);
    if (rc == NGSQ_OK) rc = P.verdict();
    rc = Z.end(rc, fd);
    if (rc != NGSQ_OK && !Z.err.empty()) sfail(c, rc, "%s", Z.err.c_str());
    if (out) {
        out->records = P.records;
        out->header_bytes = P.H.text.size();
        out->text_bytes = P.text_bytes;
        out->bam_bytes = Z.bam_bytes;
        out->compressed_bytes = Z.enc.comp_bytes;
        out->chunks = P.chunks;
        out->blocks = Z.enc.blocks;
        out->stored_blocks = Z.enc.stored;
        out->read_ms = P.text.read_ms;
        out->h2d_ms = P.h2d_ms;
        out->parse_ms = P.parse_ms;
        out->deflate_ms = Z.deflate_ms;
        out->d2h_ms = Z.w.copy_ms;
        out->write_ms = Z.w.write_ms;
        out->total_ms = now_ms() - t_begin;
    }
    return rc;
}

} // extern "C"
