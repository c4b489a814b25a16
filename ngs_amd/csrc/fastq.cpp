// fastq.cpp -- ngsq_bam_write_fastq (include/ngsq_fastq.h): the device ingest hands out the file's records batch by batch;
// fastq_kernel.hip sizes and classifies every record, the ingest's scan turns the sizes into offsets per output, and a second
// pass writes the kept records' lines into one device buffer per output.  The output stage of device_out.h (one writer thread
// per file) carries the buffers of batch k to the descriptors -- as they are, or as the BGZF blocks the device encoder makes of
// them -- while the main thread ingests and formats batch k+1.  The host never walks the records.  DESIGN.md section 26.
#include "../../include/ngsq_fastq.h"

#include <algorithm>
#include <cstring>

#include "context.h"
#include "device_out.h"
#include "fastq_kernels.h"
#include "ingest_consumer.h"

using namespace ngsq;

namespace {

constexpr uint64_t FASTQ_BATCH_RECORDS = (uint64_t)1 << 20;
const char *const OUTPUT_NAME[FASTQ_OUTPUTS] = {"read one file", "read two file", "other reads file"};

// What the batches of one run share.  The order of the members is the order the drain rule asks for: the stream is drained
// first, the writers end (and their copy streams with them) before the buffers they copy from go.
struct FastqRun {
    ngsq_bam *b = nullptr;
    ngsq_ctx *c = nullptr;
    hipStream_t st = nullptr;
    FastqRules rules{};
    uint32_t n_out = 0, bgzf = 0; // outputs [0, n_out); bit k: output k receives BGZF
    int fd[FASTQ_OUTPUTS] = {-1, -1, -1};
    DevArray<unsigned long long> d_work;
    DevArray<uint64_t> d_off[FASTQ_OUTPUTS];
    DevArray<char> d_text[FASTQ_OUTPUTS][2]; // [output][batch & 1]
    ScanScratch scan;
    MappedBuf hw, zhw; // the formatter's words, the encoders'
    HipEvents<4> ev;   // size a/b, write a/b
    HipEvents<2> zev;  // around a batch's encoder launches
    JobSlots slots;    // of d_text and of the encoders' blocks: the outputs share the batch
    BgzfEncoder enc[FASTQ_OUTPUTS];
    DeviceWriter w[FASTQ_OUTPUTS];
    StreamDrain drain;
    uint64_t records = 0, text_bytes[FASTQ_OUTPUTS] = {0, 0, 0}, counts[FASTQ_WORK_WORDS] = {};
    uint64_t bad = ~0ull;
    double scan_ms = 0, format_ms = 0, deflate_ms = 0;

    int begin(uint64_t first_batch_records);
    int format_batch(const ngsq_batch &bt, const BatchOrigin &o, bool *more);
    int finish(int rc);
};

int FastqRun::begin(uint64_t first_batch_records) {
    st = c->stream;
    drain.s = st;
    BHIP(d_work.reserve(FASTQ_WORK_WORDS));
    BHIP(hw.reserve(FASTQ_HOST_WORDS * sizeof(unsigned long long)));
    memset(hw.h, 0, FASTQ_HOST_WORDS * sizeof(unsigned long long));
    {
        unsigned long long init[FASTQ_WORK_WORDS] = {};
        init[FW_BAD] = ~0ull;
        BHIP(hipMemcpyAsync(d_work.p, init, sizeof init, hipMemcpyHostToDevice, st));
        BHIP(hipStreamSynchronize(st)); // (init is this block's)
    }
    if (bgzf) {
        BHIP(zhw.reserve(FASTQ_OUTPUTS * DEFLATE_HOST_WORDS * sizeof(unsigned long long)));
        memset(zhw.h, 0, FASTQ_OUTPUTS * DEFLATE_HOST_WORDS * sizeof(unsigned long long));
        for (uint32_t k = 0; k < FASTQ_OUTPUTS; k++) {
            enc[k].h = static_cast<const unsigned long long *>(zhw.h) + k * DEFLATE_HOST_WORDS;
            enc[k].hdev = static_cast<unsigned long long *>(zhw.dev) + k * DEFLATE_HOST_WORDS;
            enc[k].effort = c->bgzf_effort;
        }
        for (auto &e : zev.e) BHIP(hipEventCreate(&e));
    }
    BHIP(slots.create());
    for (auto &e : ev.e) BHIP(hipEventCreate(&e));
    for (uint32_t k = 0; k < n_out; k++) {
        BHIP(w[k].start(fd[k], c->device));
        if (d_off[k].reserve(first_batch_records + 1) != hipSuccess)
            return ngsq_bam_fail(NGSQ_ERR_DEVICE, "allocating the FASTQ formatter's arrays for %llu records", (unsigned long long)first_batch_records);
    }
    return NGSQ_OK;
}

// One batch of the device ingest: sized and classified, scanned per output, written into the outputs' device buffers, those
// compressed where the output is BGZF, and handed to the writers.  *more = false: nothing more can be written (a writer that has
// failed: its error is read at the end).  bad != ~0 afterwards: a kept record that cannot be written; nothing of the batch has
// been handed to the writers then.
int FastqRun::format_batch(const ngsq_batch &bt, const BatchOrigin &o, bool *more) {
    *more = false;
    const uint64_t n = bt.n_records;
    FastqOffsets off{};
    for (uint32_t k = 0; k < n_out; k++) {
        BHIP(d_off[k].reserve(n + 1));
        off.v[k] = d_off[k].p;
    }
    // sizes, offsets, and the batch's text bytes and the counts to the host
    BHIP(hipEventRecord(ev.e[0], st));
    BHIP(launch_fastq_size(bt, o, rules, off, d_work.p, st));
    for (uint32_t k = 0; k < n_out; k++) BHIP(scan.exclusive_scan(off.v[k], n + 1, st));
    BHIP(launch_fastq_total(off, n, d_work.p, static_cast<unsigned long long *>(hw.dev), st));
    BHIP(hipEventRecord(ev.e[1], st));
    BHIP(hipEventSynchronize(ev.e[1]));
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev.e[0], ev.e[1]) == hipSuccess) format_ms += ms;
    const unsigned long long *const h = static_cast<const unsigned long long *>(hw.h);
    uint64_t bytes[FASTQ_OUTPUTS];
    for (uint32_t k = 0; k < FASTQ_OUTPUTS; k++) bytes[k] = h[FH_BYTES + k];
    for (uint32_t k = 0; k < FASTQ_WORK_WORDS; k++) counts[k] = h[FH_WORK + k];
    records += n;
    if (!slots.acquire(w, n_out)) return NGSQ_OK;
    const uint32_t slot = slots.slot();
    FastqText text{};
    for (uint32_t k = 0; k < n_out; k++) {
        if (d_text[k][slot].reserve(bytes[k] + 1 + DEFLATE_IN_SLACK) != hipSuccess)
            return ngsq_bam_fail(NGSQ_ERR_DEVICE, "allocating %llu bytes for a batch's FASTQ text", (unsigned long long)bytes[k]);
        text.v[k] = d_text[k][slot].p;
    }
    // the write pass; its error word is read before anything of the batch leaves
    BHIP(hipEventRecord(ev.e[2], st));
    BHIP(launch_fastq_write(bt, o, rules, off, text, d_work.p, static_cast<unsigned long long *>(hw.dev), st));
    BHIP(hipEventRecord(ev.e[3], st));
    BHIP(hipEventSynchronize(ev.e[3]));
    if (hipEventElapsedTime(&ms, ev.e[2], ev.e[3]) == hipSuccess) format_ms += ms;
    if (h[FH_WORK + FW_BAD] != ~0ull) {
        bad = h[FH_WORK + FW_BAD];
        return NGSQ_OK;
    }
    const char *src[FASTQ_OUTPUTS] = {text.v[0], text.v[1], text.v[2]};
    uint64_t job_bytes[FASTQ_OUTPUTS] = {bytes[0], bytes[1], bytes[2]};
    bool any = false;
    for (uint32_t k = 0; k < n_out; k++) any |= (bgzf >> k & 1) && bytes[k];
    if (any) {
        // the text of a compressed output stays on the device: its blocks are what the writer copies.  The host learns their
        // size from the encoder's pinned words, so it waits for the batch here (the writers still work on the one before).
        BHIP(hipEventRecord(zev.e[0], st));
        for (uint32_t k = 0; k < n_out; k++)
            if ((bgzf >> k & 1) && bytes[k]) BHIP(enc[k].launch(slot, text.v[k], bytes[k], st));
        BHIP(hipEventRecord(zev.e[1], st));
        BHIP(hipEventSynchronize(zev.e[1]));
        if (hipEventElapsedTime(&ms, zev.e[0], zev.e[1]) == hipSuccess) deflate_ms += ms;
        for (uint32_t k = 0; k < n_out; k++)
            if ((bgzf >> k & 1) && bytes[k])
                if (const char *m = enc[k].collect(slot, bytes[k], &src[k], &job_bytes[k])) return ngsq_bam_fail(NGSQ_ERR_STATE, "%s", m);
    }
    BHIP(slots.submit(w, n_out, src, job_bytes, st));
    for (uint32_t k = 0; k < n_out; k++) text_bytes[k] += bytes[k];
    *more = true;
    for (uint32_t k = 0; k < n_out; k++)
        if (w[k].failed()) *more = false;
    return NGSQ_OK;
}

// The end of a run whose batches gave `rc`: the stream drained, every queued copy written (or skipped after a failed write), the
// writers' own errors reported, the EOF block behind every BGZF output that is whole, the record that could not be written.
int FastqRun::finish(int rc) {
    if (rc == NGSQ_OK) {
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = ngsq_bam_fail(NGSQ_ERR_DEVICE, "hipStreamSynchronize: %s", hipGetErrorString(e));
    }
    WriterEnd end[FASTQ_OUTPUTS] = {};
    for (uint32_t k = 0; k < n_out; k++) end[k] = w[k].end();
    auto write_failed = [](uint32_t k, int e) {
        return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "could not write record to %s: %s (os error %d)", OUTPUT_NAME[k], strerror(e), e);
    };
    for (uint32_t k = 0; k < n_out && rc == NGSQ_OK; k++) {
        if (end[k].herr != hipSuccess) rc = ngsq_bam_fail(NGSQ_ERR_DEVICE, "copying the FASTQ text to the host: %s", hipGetErrorString(end[k].herr));
        else if (end[k].werr) rc = write_failed(k, end[k].werr);
    }
    for (uint32_t k = 0; k < n_out && rc == NGSQ_OK && bad == ~0ull; k++)
        if (bgzf >> k & 1) {
            if (const int e = write_bgzf_eof(fd[k])) rc = write_failed(k, e);
            enc[k].comp_bytes += sizeof BGZF_EOF_BLOCK;
        }
    if (rc == NGSQ_OK && bad != ~0ull)
        rc = ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "writing FASTQ record: record %llu: quality score above 93", (unsigned long long)(bad >> FASTQ_ERR_BITS));
    return rc;
}

} // namespace

extern "C" int ngsq_bam_write_fastq(ngsq_bam *b, ngsq_ctx *c, int fd_one, int fd_two, int fd_other, const ngsq_fastq_options *opt,
                                    ngsq_fastq_report *out) {
    if (out) memset(out, 0, sizeof *out);
    if (!b || !c || !opt) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    if (opt->struct_size != sizeof *opt)
        return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "ngsq_fastq_options.struct_size is %u, not %zu", opt->struct_size, sizeof *opt);
    if (fd_one < 0) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "no descriptor for the read one file");
    if (fd_two < 0 && fd_other >= 0) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "a file for the other reads needs a read two file");
    if (opt->require_flags > 65535u || opt->exclude_flags > 65535u) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "flag bits above 65535");
    if (opt->default_quality > NGSQ_FASTQ_MAX_QUALITY) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "default quality %u is above 93", opt->default_quality);
    if (opt->name_suffix > 1u) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "name_suffix is 0 or 1");
    const uint32_t n_out = fd_two < 0 ? 1u : fd_other < 0 ? 2u : 3u;
    if (opt->bgzf_mask >> n_out) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "bgzf_mask 0x%x names an output that is not given", opt->bgzf_mask);
    if (const int rc = require_fresh_reader(b, "a FASTQ file is written")) return rc;
    const double t_begin = now_ms();
    BHIP(hipSetDevice(c->device));
    FastqRun r;
    r.b = b;
    r.c = c;
    r.n_out = n_out;
    r.bgzf = opt->bgzf_mask;
    r.fd[0] = fd_one, r.fd[1] = fd_two, r.fd[2] = fd_other;
    r.rules = FastqRules{opt->require_flags, opt->exclude_flags, opt->default_quality, opt->name_suffix, n_out > 1 ? 1u : 0u, n_out > 2 ? 1u : 0u};
    const uint64_t max_records = opt->max_records, batch_records = opt->batch_records ? opt->batch_records : FASTQ_BATCH_RECORDS;
    int rc = r.begin(std::min<uint64_t>(batch_records, max_records ? max_records : batch_records));
    // ---- the scan: every batch of the device ingest, in file order
    for (bool more = true; more && rc == NGSQ_OK;) {
        more = false;
        const uint64_t left = max_records ? max_records - r.records : ~0ull;
        if (!left) break;
        ngsq_batch bt;
        BatchOrigin o;
        const double s0 = now_ms();
        rc = next_batch_with_origin(b, c, std::min(batch_records, left), &bt, &o);
        r.scan_ms += now_ms() - s0;
        if (rc || !bt.n_records) break;
        rc = r.format_batch(bt, o, &more);
        if (r.bad != ~0ull) break;
    }
    rc = r.finish(rc);
    if (out) {
        out->records_scanned = r.records;
        out->excluded = r.counts[FW_EXCLUDED];
        out->no_sequence = r.counts[FW_NO_SEQUENCE];
        out->reads_one = r.counts[FW_ONE];
        out->reads_two = r.counts[FW_TWO];
        out->reads_other = r.counts[FW_OTHER];
        out->dropped_other = r.counts[FW_DROPPED];
        out->batches = r.slots.jobs;
        for (uint32_t k = 0; k < FASTQ_OUTPUTS; k++) {
            out->text_bytes[k] = r.text_bytes[k];
            out->compressed_bytes[k] = r.enc[k].comp_bytes;
            out->blocks += r.enc[k].blocks;
            out->stored_blocks += r.enc[k].stored;
            out->copy_ms += r.w[k].copy_ms;
            out->write_ms += r.w[k].write_ms;
        }
        out->scan_ms = r.scan_ms;
        out->format_ms = r.format_ms;
        out->deflate_ms = r.deflate_ms;
        out->total_ms = now_ms() - t_begin;
    }
    return rc;
}
