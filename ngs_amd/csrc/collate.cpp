// collate.cpp -- ngsq_bam_write_fastq_collated (include/ngsq_collate.h).  Four phases, one after the
// other.  The walk: every batch of the device ingest is flagged, its kept records are compacted into resident slabs
// (launch_sort_take, as a round of `ngs convert --sort coordinate` keeps its records) and their scores checked.  The match: a
// name key per record, sort_pairs_u64, the run check, the mate search.  The order: record i leads a pair iff mate[i] > i, so
// three flag-scan-fill passes over the resident order give the pairs, the singletons and the others in file order without a
// second sort.  The write: each list in pieces, sized, scanned and formatted by fastq_format.h's formatter, and handed to one
// writer thread per output as fastq.cpp hands its batches over.  The host never walks the records.
#include "../../include/ngsq_collate.h"

#include <algorithm>
#include <cstring>

#include "collate_kernels.h"
#include "context.h"
#include "device_out.h"
#include "ingest_consumer.h"
#include "sort_resident.h"

using namespace ngsq;

namespace {

constexpr uint64_t COLLATE_BATCH_RECORDS = (uint64_t)1 << 20;
constexpr uint64_t COLLATE_PIECE_RECORDS = (uint64_t)1 << 20, COLLATE_PIECE_MAX = (uint64_t)1 << 28;
const char *const OUTPUT_NAME[COLLATE_OUTPUTS] = {"read one file", "read two file", "other reads file", "singletons file"};
enum : uint32_t { HW_A = COLLATE_WORK_WORDS, HW_B, HOST_WORDS }; // behind the work words: two totals

// What the phases of one run share.  The order of the members is the order the drain rule asks for: the stream is drained
// first, the writers end (and their copy streams with them) before the buffers they copy from go, the slabs go last.
struct CollateRun {
    ngsq_bam *b = nullptr;
    ngsq_ctx *c = nullptr;
    hipStream_t st = nullptr;
    FastqRules rules{};
    bool two_files = false;
    uint32_t hash_bits = 0;
    uint64_t piece_records = COLLATE_PIECE_RECORDS;
    // the outputs that are given, in the order of their numbers: writer k writes output out_of[k]
    uint32_t n_w = 0, out_of[COLLATE_OUTPUTS] = {}, bgzf = 0; // bgzf: bit k: writer k receives BGZF
    int fd[COLLATE_OUTPUTS] = {-1, -1, -1, -1}, w_of[COLLATE_OUTPUTS] = {-1, -1, -1, -1};
    SortResident R; // the slabs, the three per-record arrays, the sort's scratch (its sink stays unused)
    DevArray<unsigned long long> d_work;
    DevArray<uint64_t> d_cnt, d_off; // a batch's kept flags and bytes; later the lists' scan and a piece's offsets
    DevArray<uint64_t> d_off_b;
    DevArray<uint8_t> d_cls;
    DevArray<uint32_t> d_mate, d_list;
    DevArray<char> d_text[COLLATE_OUTPUTS][2]; // [writer][job & 1]
    ScanScratch scan;
    MappedBuf hw, zhw;
    HipEvents<2> ev, zev;
    JobSlots slots;
    BgzfEncoder enc[COLLATE_OUTPUTS];
    DeviceWriter w[COLLATE_OUTPUTS];
    StreamDrain drain;
    uint64_t scanned = 0, batches = 0, slab_bytes = 0, pieces = 0;
    uint64_t list_n[3] = {0, 0, 0}, list_at[3] = {0, 0, 0}; // the three lists inside d_list
    uint64_t text_bytes[COLLATE_OUTPUTS] = {0, 0, 0, 0}, counts[COLLATE_WORK_WORDS] = {};
    bool writers_on = false, stop = false; // stop: a writer has failed, nothing more can be written
    double scan_ms = 0, walk_ms = 0, match_ms = 0, format_ms = 0, deflate_ms = 0;

    const unsigned long long *h() const { return static_cast<const unsigned long long *>(hw.h); }
    unsigned long long *hdev() const { return static_cast<unsigned long long *>(hw.dev); }
    void add(double *sum) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.e[0], ev.e[1]) == hipSuccess) *sum += ms;
    }
    int begin();
    int walk_batch(const ngsq_batch &bt, const BatchOrigin &o);
    int read_work();
    int match();
    int start_writers();
    int write_list(uint32_t kind);
    int finish(int rc);
};

int CollateRun::begin() {
    st = c->stream;
    drain.s = st;
    if (R.begin(c->device, st, c->bgzf_effort)) return ngsq_bam_fail(R.code, "%s", R.err.c_str());
    BHIP(d_work.reserve(COLLATE_WORK_WORDS));
    BHIP(hw.reserve(HOST_WORDS * sizeof(unsigned long long)));
    memset(hw.h, 0, HOST_WORDS * sizeof(unsigned long long));
    unsigned long long init[COLLATE_WORK_WORDS] = {};
    init[CW_BAD] = ~0ull;
    BHIP(hipMemcpyAsync(d_work.p, init, sizeof init, hipMemcpyHostToDevice, st));
    BHIP(hipStreamSynchronize(st)); // (init is this block's)
    for (auto &e : ev.e) BHIP(hipEventCreate(&e));
    return NGSQ_OK;
}

// One batch of the device ingest: flagged and counted, its kept records admitted against the budget, compacted behind the
// resident ones, their scores checked.
int CollateRun::walk_batch(const ngsq_batch &bt, const BatchOrigin &o) {
    const uint64_t n = bt.n_records;
    if (!batches) { // the reader's buffers are there: what is free now is free for the records
        uint64_t chunk_bytes = 0, view_bytes = 0;
        bam_device_view_sizes(b, &chunk_bytes, &view_bytes);
        slab_bytes = std::min(std::max(2 * chunk_bytes, SORT_SLAB_MIN), SORT_SLAB_MAX);
        if (!R.budget && R.default_budget()) return ngsq_bam_fail(R.code, "%s", R.err.c_str());
    }
    batches++;
    scanned += n;
    BHIP(d_cnt.reserve(n + 1));
    BHIP(d_off.reserve(n + 1));
    BHIP(launch_collate_flag(o.raw, o.rec_off, n, rules, d_cnt.p, d_off.p, d_work.p, st));
    BHIP(scan.exclusive_scan(d_cnt.p, n + 1, st));
    BHIP(scan.exclusive_scan(d_off.p, n + 1, st));
    BHIP(launch_samtext_word(d_cnt.p, n, hdev() + HW_A, st));
    BHIP(launch_samtext_word(d_off.p, n, hdev() + HW_B, st));
    BHIP(hipStreamSynchronize(st));
    const uint64_t kept = h()[HW_A], bytes = h()[HW_B];
    if (!kept) return NGSQ_OK;
    BHIP(launch_collate_qual(o.raw, o.rec_off, n, d_cnt.p, bt.first_record_index, d_work.p, st));
    if (R.records + kept > 0xFFFFFFFFull) return ngsq_bam_fail(NGSQ_ERR_LIMIT, "fastq --collate holds at most 2^32 - 1 kept records");
    const uint64_t need = R.rec_bytes + bytes + (R.records + kept) * COLLATE_BYTES_PER_RECORD;
    if (need > R.budget)
        return ngsq_bam_fail(NGSQ_ERR_LIMIT, "fastq --collate holds the kept records in device memory: %llu bytes needed, %llu allowed",
                             (unsigned long long)need, (unsigned long long)R.budget);
    uint8_t *dst = nullptr;
    if (R.place(bytes, slab_bytes, 16u, &dst) || R.reserve_records(R.records + kept)) return ngsq_bam_fail(R.code, "%s", R.err.c_str());
    BHIP(launch_sort_take(o.raw, o.rec_off, n, d_cnt.p, d_off.p, dst, R.records, R.d_addr.p, R.d_len.p, R.d_key.p, st));
    R.rec_bytes += bytes;
    R.records += kept;
    return NGSQ_OK;
}

int CollateRun::read_work() {
    BHIP(launch_collate_words(d_work.p, hdev(), st));
    BHIP(hipStreamSynchronize(st));
    for (uint32_t k = 0; k < COLLATE_WORK_WORDS; k++) counts[k] = h()[k];
    return NGSQ_OK;
}

// The match and the order: mate[i] for every resident record, then the three lists in file order, side by side in d_list.
int CollateRun::match() {
    const uint64_t n = R.records;
    if (!n) return NGSQ_OK;
    BHIP(hipEventRecord(ev.e[0], st));
    BHIP(d_cls.reserve(n));
    BHIP(d_mate.reserve(n));
    BHIP(d_list.reserve(n));
    BHIP(launch_collate_key(R.d_addr.p, n, hash_bits, R.d_key.p, d_cls.p, st));
    const uint32_t *perm = nullptr;
    BHIP(sort_pairs_u64(R.d_key.p, n, R.sort, st, &perm));
    // the sorted keys lie in the half of the ping-pong the last pass wrote
    const uint64_t *skey = R.sort.passes_run & 1u ? R.sort.keys_b.p : R.d_key.p;
    BHIP(launch_collate_run_limit(skey, n, d_work.p, st));
    if (const int rc = read_work()) return rc;
    if (counts[CW_LONG_RUN])
        return ngsq_bam_fail(NGSQ_ERR_LIMIT, "fastq --collate: more than %u reads share a name or a name hash", NGSQ_COLLATE_MAX_RUN);
    BHIP(launch_collate_match(skey, perm, R.d_addr.p, d_cls.p, n, d_mate.p, d_work.p, st));
    BHIP(d_cnt.reserve(n + 1));
    uint64_t at = 0;
    for (uint32_t kind = CK_LEAD; kind <= CK_OTHER; kind++) {
        BHIP(launch_collate_list_flag(d_cls.p, d_mate.p, n, kind, d_cnt.p, st));
        BHIP(scan.exclusive_scan(d_cnt.p, n + 1, st));
        BHIP(launch_collate_list_fill(d_cls.p, d_mate.p, n, kind, d_cnt.p, d_list.p + at, st));
        BHIP(launch_samtext_word(d_cnt.p, n, hdev() + HW_A, st));
        BHIP(hipStreamSynchronize(st));
        list_at[kind] = at;
        list_n[kind] = h()[HW_A];
        at += list_n[kind];
        if (at > n) return ngsq_bam_fail(NGSQ_ERR_STATE, "fastq --collate: the lists hold more than the %llu resident records", (unsigned long long)n);
    }
    BHIP(hipEventRecord(ev.e[1], st));
    if (const int rc = read_work()) return rc;
    add(&match_ms);
    if (2 * list_n[CK_LEAD] + list_n[CK_SINGLE] + list_n[CK_OTHER] != n)
        return ngsq_bam_fail(NGSQ_ERR_STATE, "fastq --collate: %llu pairs, %llu singletons and %llu others of %llu resident records",
                             (unsigned long long)list_n[CK_LEAD], (unsigned long long)list_n[CK_SINGLE], (unsigned long long)list_n[CK_OTHER],
                             (unsigned long long)n);
    return NGSQ_OK;
}

int CollateRun::start_writers() {
    writers_on = true;
    if (bgzf) {
        BHIP(zhw.reserve(COLLATE_OUTPUTS * DEFLATE_HOST_WORDS * sizeof(unsigned long long)));
        memset(zhw.h, 0, COLLATE_OUTPUTS * DEFLATE_HOST_WORDS * sizeof(unsigned long long));
        for (uint32_t k = 0; k < COLLATE_OUTPUTS; k++) {
            enc[k].h = static_cast<const unsigned long long *>(zhw.h) + k * DEFLATE_HOST_WORDS;
            enc[k].hdev = static_cast<unsigned long long *>(zhw.dev) + k * DEFLATE_HOST_WORDS;
            enc[k].effort = c->bgzf_effort;
        }
        for (auto &e : zev.e) BHIP(hipEventCreate(&e));
    }
    BHIP(slots.create());
    for (uint32_t k = 0; k < n_w; k++) BHIP(w[k].start(fd[out_of[k]], c->device));
    return NGSQ_OK;
}

// One list, in pieces of piece_records entries: sizes, offsets, text, the encoders where an output is BGZF, the writers.  A list
// without an output is not written.  Every job goes to every writer (most with no byte), so that they count the jobs alike.
int CollateRun::write_list(uint32_t kind) {
    const uint32_t mode = kind != CK_LEAD ? CM_RECORD : two_files ? CM_SPLIT : CM_INTERLEAVED;
    const int wa = w_of[kind == CK_LEAD ? NGSQ_FASTQ_ONE : kind == CK_SINGLE ? NGSQ_FASTQ_SINGLE : NGSQ_FASTQ_OTHER];
    const int wb = mode == CM_SPLIT ? w_of[NGSQ_FASTQ_TWO] : -1;
    if (wa < 0) return NGSQ_OK;
    for (uint64_t e0 = 0; e0 < list_n[kind] && !stop; e0 += piece_records) {
        const uint64_t m = std::min(piece_records, list_n[kind] - e0);
        const CollatePiece p{d_list.p + list_at[kind] + e0, m, R.d_addr.p, d_cls.p, d_mate.p, mode};
        BHIP(d_off.reserve(m + 1));
        if (wb >= 0) BHIP(d_off_b.reserve(m + 1));
        BHIP(hipEventRecord(ev.e[0], st));
        BHIP(launch_collate_size(p, rules, d_off.p, wb >= 0 ? d_off_b.p : nullptr, st));
        BHIP(scan.exclusive_scan(d_off.p, m + 1, st));
        BHIP(launch_samtext_word(d_off.p, m, hdev() + HW_A, st));
        if (wb >= 0) {
            BHIP(scan.exclusive_scan(d_off_b.p, m + 1, st));
            BHIP(launch_samtext_word(d_off_b.p, m, hdev() + HW_B, st));
        }
        BHIP(hipEventRecord(ev.e[1], st));
        BHIP(hipEventSynchronize(ev.e[1]));
        add(&format_ms);
        uint64_t bytes[COLLATE_OUTPUTS] = {0, 0, 0, 0};
        bytes[wa] = h()[HW_A];
        if (wb >= 0) bytes[wb] = h()[HW_B];
        pieces++;
        if (!slots.acquire(w, n_w)) {
            stop = true;
            break;
        }
        const uint32_t slot = slots.slot();
        for (const int k : {wa, wb})
            if (k >= 0 && d_text[k][slot].reserve(bytes[k] + 1 + DEFLATE_IN_SLACK) != hipSuccess)
                return ngsq_bam_fail(NGSQ_ERR_DEVICE, "allocating %llu bytes for a piece's FASTQ text", (unsigned long long)bytes[k]);
        BHIP(hipEventRecord(ev.e[0], st));
        BHIP(launch_collate_write(p, rules, d_off.p, wb >= 0 ? d_off_b.p : nullptr, d_text[wa][slot].p, wb >= 0 ? d_text[wb][slot].p : nullptr, st));
        BHIP(hipEventRecord(ev.e[1], st));
        BHIP(hipEventSynchronize(ev.e[1]));
        add(&format_ms);
        const char *src[COLLATE_OUTPUTS] = {nullptr, nullptr, nullptr, nullptr};
        uint64_t job_bytes[COLLATE_OUTPUTS] = {0, 0, 0, 0};
        bool any = false;
        for (const int k : {wa, wb})
            if (k >= 0) {
                src[k] = d_text[k][slot].p;
                job_bytes[k] = bytes[k];
                any |= (bgzf >> k & 1) && bytes[k];
            }
        if (any) {
            // the text of a compressed output stays on the device: its blocks are what the writer copies
            BHIP(hipEventRecord(zev.e[0], st));
            for (const int k : {wa, wb})
                if (k >= 0 && (bgzf >> k & 1) && bytes[k]) BHIP(enc[k].launch(slot, src[k], bytes[k], st));
            BHIP(hipEventRecord(zev.e[1], st));
            BHIP(hipEventSynchronize(zev.e[1]));
            float ms = 0;
            if (hipEventElapsedTime(&ms, zev.e[0], zev.e[1]) == hipSuccess) deflate_ms += ms;
            for (const int k : {wa, wb})
                if (k >= 0 && (bgzf >> k & 1) && bytes[k])
                    if (const char *msg = enc[k].collect(slot, bytes[k], &src[k], &job_bytes[k])) return ngsq_bam_fail(NGSQ_ERR_STATE, "%s", msg);
        }
        BHIP(slots.submit(w, n_w, src, job_bytes, st));
        for (uint32_t k = 0; k < n_w; k++) {
            text_bytes[out_of[k]] += bytes[k];
            if (w[k].failed()) stop = true;
        }
    }
    return NGSQ_OK;
}

// The end of a run whose phases gave `rc`: the stream drained, every queued copy written (or skipped after a failed write), the
// writers' own errors reported, the EOF block behind every BGZF output of a run that wrote.
int CollateRun::finish(int rc) {
    if (rc == NGSQ_OK) {
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = ngsq_bam_fail(NGSQ_ERR_DEVICE, "hipStreamSynchronize: %s", hipGetErrorString(e));
    }
    if (!writers_on) return rc;
    WriterEnd end[COLLATE_OUTPUTS] = {};
    for (uint32_t k = 0; k < n_w; k++) end[k] = w[k].end();
    auto write_failed = [&](uint32_t k, int e) {
        return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "could not write record to %s: %s (os error %d)", OUTPUT_NAME[out_of[k]], strerror(e), e);
    };
    for (uint32_t k = 0; k < n_w && rc == NGSQ_OK; k++) {
        if (end[k].herr != hipSuccess) rc = ngsq_bam_fail(NGSQ_ERR_DEVICE, "copying the FASTQ text to the host: %s", hipGetErrorString(end[k].herr));
        else if (end[k].werr) rc = write_failed(k, end[k].werr);
    }
    for (uint32_t k = 0; k < n_w && rc == NGSQ_OK; k++)
        if (bgzf >> k & 1) {
            if (const int e = write_bgzf_eof(fd[out_of[k]])) rc = write_failed(k, e);
            enc[k].comp_bytes += sizeof BGZF_EOF_BLOCK;
        }
    return rc;
}

} // namespace

extern "C" uint64_t ngsq_collate_bytes_per_record(void) { return COLLATE_BYTES_PER_RECORD; }

extern "C" int ngsq_bam_write_fastq_collated(ngsq_bam *b, ngsq_ctx *c, int fd_one, int fd_two, int fd_other, int fd_single,
                                             const ngsq_collate_options *opt, ngsq_collate_report *out) {
    if (out) memset(out, 0, sizeof *out);
    if (!b || !c || !opt) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    if (opt->struct_size != sizeof *opt)
        return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "ngsq_collate_options.struct_size is %u, not %zu", opt->struct_size, sizeof *opt);
    if (fd_one < 0) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "no descriptor for the read one file");
    if (fd_two < 0 && fd_other >= 0) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "a file for the other reads needs a read two file");
    if (opt->require_flags > 65535u || opt->exclude_flags > 65535u) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "flag bits above 65535");
    if (opt->default_quality > NGSQ_FASTQ_MAX_QUALITY) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "default quality %u is above 93", opt->default_quality);
    if (opt->name_suffix > 1u) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "name_suffix is 0 or 1");
    if (opt->hash_bits > 63u) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "hash_bits is 0 to 63");
    if (opt->reserved) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "ngsq_collate_options.reserved is %u, not 0", opt->reserved);
    const int fds[COLLATE_OUTPUTS] = {fd_one, fd_two, fd_other, fd_single};
    for (uint32_t k = 0; k < COLLATE_OUTPUTS; k++)
        if ((opt->bgzf_mask >> k & 1u) && fds[k] < 0) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "bgzf_mask 0x%x names an output that is not given", opt->bgzf_mask);
    if (opt->bgzf_mask >> COLLATE_OUTPUTS) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "bgzf_mask 0x%x names an output that is not given", opt->bgzf_mask);
    if (const int rc = require_fresh_reader(b, "a FASTQ file is written")) return rc;
    const double t_begin = now_ms();
    BHIP(hipSetDevice(c->device));
    CollateRun r;
    r.b = b;
    r.c = c;
    r.two_files = fd_two >= 0;
    r.hash_bits = opt->hash_bits;
    r.piece_records = std::min(opt->piece_records ? opt->piece_records : COLLATE_PIECE_RECORDS, COLLATE_PIECE_MAX);
    for (uint32_t k = 0; k < COLLATE_OUTPUTS; k++) {
        r.fd[k] = fds[k];
        if (fds[k] < 0) continue;
        if (opt->bgzf_mask >> k & 1u) r.bgzf |= 1u << r.n_w;
        r.w_of[k] = (int)r.n_w;
        r.out_of[r.n_w++] = k;
    }
    // (for the walk every kept record is "written": what is dropped is decided by the lists)
    r.rules = FastqRules{opt->require_flags, opt->exclude_flags, opt->default_quality, opt->name_suffix, 0u, 0u};
    r.R.budget = opt->memory_budget;
    const uint64_t max_records = opt->max_records, batch_records = opt->batch_records ? opt->batch_records : COLLATE_BATCH_RECORDS;
    int rc = r.begin();
    // ---- the walk: every batch of the device ingest, in file order
    while (rc == NGSQ_OK) {
        const uint64_t left = max_records ? max_records - r.scanned : ~0ull;
        if (!left) break;
        ngsq_batch bt;
        BatchOrigin o;
        const double s0 = now_ms();
        rc = next_batch_with_origin(b, c, std::min(batch_records, left), &bt, &o);
        r.scan_ms += now_ms() - s0;
        if (rc || !bt.n_records) break;
        rc = r.walk_batch(bt, o);
    }
    if (rc == NGSQ_OK) rc = r.read_work();
    r.walk_ms = now_ms() - t_begin;
    if (rc == NGSQ_OK && r.counts[CW_BAD] != ~0ull)
        rc = ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "writing FASTQ record: record %llu: quality score above 93",
                           (unsigned long long)(r.counts[CW_BAD] >> FASTQ_ERR_BITS));
    // ---- the match, then the three lists through the writers
    if (rc == NGSQ_OK) rc = r.match();
    if (rc == NGSQ_OK) rc = r.start_writers();
    for (uint32_t kind = CK_LEAD; kind <= CK_OTHER && rc == NGSQ_OK; kind++) rc = r.write_list(kind);
    rc = r.finish(rc);
    if (out) {
        out->records_scanned = r.scanned;
        out->excluded = r.counts[CW_EXCLUDED];
        out->no_sequence = r.counts[CW_NO_SEQUENCE];
        out->reads_one = r.counts[CW_ONE];
        out->reads_two = r.counts[CW_TWO];
        out->reads_other = r.counts[CW_OTHER];
        out->dropped_other = r.w_of[NGSQ_FASTQ_OTHER] < 0 ? r.list_n[CK_OTHER] : 0;
        out->pairs = r.list_n[CK_LEAD];
        out->singletons = r.list_n[CK_SINGLE];
        out->ambiguous = r.counts[CW_AMBIGUOUS];
        out->dropped_singletons = r.w_of[NGSQ_FASTQ_SINGLE] < 0 ? r.list_n[CK_SINGLE] : 0;
        out->name_collisions = r.counts[CW_COLLISIONS];
        out->batches = r.batches;
        out->resident_records = r.R.records;
        out->resident_bytes = r.R.rec_bytes + r.R.records * COLLATE_BYTES_PER_RECORD;
        out->sort_passes = r.R.sort.passes_run;
        out->pieces = r.pieces;
        for (uint32_t k = 0; k < r.n_w; k++) {
            const uint32_t o = r.out_of[k];
            out->text_bytes[o] = r.text_bytes[o];
            out->compressed_bytes[o] = r.enc[k].comp_bytes;
            out->blocks += r.enc[k].blocks;
            out->stored_blocks += r.enc[k].stored;
            out->copy_ms += r.w[k].copy_ms;
            out->write_ms += r.w[k].write_ms;
        }
        out->scan_ms = r.scan_ms;
        out->walk_ms = r.walk_ms;
        out->match_ms = r.match_ms;
        out->format_ms = r.format_ms;
        out->deflate_ms = r.deflate_ms;
        out->total_ms = now_ms() - t_begin;
    }
    return rc;
}
