// markdup.cpp -- ngsq_bam_mark_duplicates (include/ngsq_markdup.h).  Four phases on one stream.  The
// walk is bamsort.cpp's: every batch of the device ingest is one byte range of its view, k_sort_keep copies it into a slab, so
// resident index = file index.  The ends pass gives every record its class, its packed unclipped 5' end and its score and
// refuses an end that cannot be packed.  The match is collate.cpp's: a name key per pair candidate, sort_pairs_u64, the run
// check, the mate search.  The mark runs twice over entries -- the pairs by their two ends, 128 bits in two stable sorts, then
// all candidates by their end -- and leaves a duplicate byte per record; the apply pass stores the flag bytes.  The write is
// sort_resident.h's: the records in the identity order, or the survivors' list, through the gather, the encoder and the
// writer.  Nothing is written before every refusal is known, and the host never walks a record.
#include "../../include/ngsq_markdup.h"

#include <algorithm>
#include <cstring>

#include "context.h"
#include "ingest_consumer.h"
#include "markdup_kernels.h"
#include "samtext_host.h" // put32
#include "sort_resident.h"

using namespace ngsq;

namespace {

constexpr uint64_t BATCH_RECORDS = (uint64_t)1 << 22;
constexpr const char *READ_CTX = "reading BAM record: ";
enum : uint32_t { HW_A = MARKDUP_WORK_WORDS, HOST_WORDS };

// What the phases of one run share.  The drain is the last member, so the stream is idle before any array goes; the slabs and
// the writer, R's, go last.
struct MarkdupRun {
    ngsq_bam *b = nullptr;
    ngsq_ctx *c = nullptr;
    hipStream_t st = nullptr;
    uint32_t hash_bits = 0;
    bool remove = false;
    SortResident R;
    DevArray<unsigned long long> d_work, d_best;
    DevArray<uint8_t> d_cls, d_dup;
    DevArray<uint64_t> d_end, d_hi, d_lo, d_val;
    DevArray<uint32_t> d_score, d_mate, d_list, d_first, d_order;
    ScanScratch scan;
    MappedBuf hw, span;
    HipEvents<2> ev;
    StreamDrain drain;
    uint64_t batches = 0, slab_bytes = 0, view_bytes = 0, pairs = 0, candidates = 0, sort_passes = 0;
    uint64_t out_records = 0, out_bytes = 0;
    uint64_t counts[MARKDUP_WORK_WORDS] = {};
    double scan_ms = 0, ends_ms = 0, match_ms = 0, mark_ms = 0;

    const unsigned long long *h() const { return static_cast<const unsigned long long *>(hw.h); }
    unsigned long long *hdev() const { return static_cast<unsigned long long *>(hw.dev); }
    int begin();
    int walk(uint64_t max_records, uint64_t batch_records);
    int read_work();
    int timed(double *sum);
    int ends();
    int match();
    int list_of(uint32_t kind, uint64_t *m);
    int mark(bool pair_entries, uint64_t m);
    int marks();
    int order_out();
};

int MarkdupRun::begin() {
    st = c->stream;
    drain.s = st;
    if (R.begin(c->device, st, c->bgzf_effort)) return ngsq_bam_fail(R.code, "%s", R.err.c_str());
    BHIP(d_work.reserve(MARKDUP_WORK_WORDS));
    BHIP(hw.reserve(HOST_WORDS * sizeof(unsigned long long)));
    memset(hw.h, 0, HOST_WORDS * sizeof(unsigned long long));
    BHIP(span.reserve(SP_WORDS * sizeof(unsigned long long)));
    unsigned long long init[MARKDUP_WORK_WORDS] = {};
    init[CW_BAD] = ~0ull;
    BHIP(hipMemcpyAsync(d_work.p, init, sizeof init, hipMemcpyHostToDevice, st));
    BHIP(hipStreamSynchronize(st)); // (init is this block's)
    for (auto &e : ev.e) BHIP(hipEventCreate(&e));
    return NGSQ_OK;
}

// Phase 1: every batch's records copied whole into a slab, as `ngs convert --sort coordinate` keeps them (its keys go unused)
int MarkdupRun::walk(uint64_t max_records, uint64_t batch_records) {
    const unsigned long long *const sp = static_cast<const unsigned long long *>(span.h);
    for (;;) {
        const uint64_t left = max_records ? max_records - R.records : ~0ull;
        if (!left) break;
        ngsq_batch bt;
        BatchOrigin o;
        const double s0 = now_ms();
        const int rc = next_batch_with_origin(b, c, std::min(batch_records, left), &bt, &o);
        scan_ms += now_ms() - s0;
        if (rc) {
            const std::string m = ngsq_bam_last_error();
            return ngsq_bam_fail(rc, "%s%s", READ_CTX, m.c_str());
        }
        const uint64_t n = bt.n_records;
        if (!n) break;
        if (!batches) { // the reader's buffers are there: what is free now is free for the records
            uint64_t chunk_bytes = 0;
            bam_device_view_sizes(b, &chunk_bytes, &view_bytes);
            slab_bytes = std::min(std::max(2 * chunk_bytes, SORT_SLAB_MIN), SORT_SLAB_MAX);
            if (!R.budget && R.default_budget()) return ngsq_bam_fail(R.code, "%s", R.err.c_str());
        }
        BHIP(launch_sort_span(o.raw, o.rec_off, n, static_cast<unsigned long long *>(span.dev), st));
        BHIP(hipStreamSynchronize(st));
        const uint64_t begin = sp[0], end = sp[1];
        if (begin >= end || end > view_bytes)
            return ngsq_bam_fail(NGSQ_ERR_STATE, "%sthe records of batch %llu lie at [%llu, %llu) of a view of %llu bytes", READ_CTX,
                                 (unsigned long long)batches, (unsigned long long)begin, (unsigned long long)end, (unsigned long long)view_bytes);
        const uint64_t bytes = end - begin;
        if (R.records + n > 0xFFFFFFFFull) return ngsq_bam_fail(NGSQ_ERR_LIMIT, "markdup holds at most 2^32 - 1 records");
        const uint64_t need = R.rec_bytes + bytes + (R.records + n) * MARKDUP_BYTES_PER_RECORD;
        if (need > R.budget)
            return ngsq_bam_fail(NGSQ_ERR_LIMIT, "markdup holds the records in device memory: %llu bytes needed, %llu allowed", (unsigned long long)need,
                                 (unsigned long long)R.budget);
        uint8_t *dst = nullptr;
        if (R.place(bytes, slab_bytes, (uint32_t)((uintptr_t)(o.raw + begin) & 15u), &dst) || R.reserve_records(R.records + n))
            return ngsq_bam_fail(R.code, "%s", R.err.c_str());
        BHIP(launch_sort_keep(o.raw, o.rec_off, n, begin, bytes, dst, R.records, R.d_addr.p, R.d_len.p, R.d_key.p, st));
        R.rec_bytes += bytes;
        R.records += n;
        batches++;
    }
    BHIP(hipStreamSynchronize(st));
    return NGSQ_OK;
}

int MarkdupRun::read_work() {
    BHIP(launch_markdup_words(d_work.p, hdev(), st));
    BHIP(hipStreamSynchronize(st));
    for (uint32_t k = 0; k < MARKDUP_WORK_WORDS; k++) counts[k] = h()[k];
    return NGSQ_OK;
}

// behind a phase bracketed by the two events: the words, and the phase's stream time
int MarkdupRun::timed(double *sum) {
    BHIP(hipEventRecord(ev.e[1], st));
    if (const int rc = read_work()) return rc;
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev.e[0], ev.e[1]) == hipSuccess) *sum += ms;
    return NGSQ_OK;
}

// Phase 2: class, end and score of every record; the smallest record whose end cannot be packed is refused
int MarkdupRun::ends() {
    const uint64_t n = R.records;
    BHIP(d_cls.reserve(n));
    BHIP(d_end.reserve(n));
    BHIP(d_score.reserve(n));
    BHIP(hipEventRecord(ev.e[0], st));
    BHIP(launch_markdup_ends(R.d_addr.p, n, d_cls.p, d_end.p, d_score.p, d_work.p, st));
    if (const int rc = timed(&ends_ms)) return rc;
    if (counts[CW_BAD] != ~0ull)
        return ngsq_bam_fail(NGSQ_ERR_LIMIT, "%srecord %llu (0-based): unclipped end outside what markdup can hold", READ_CTX, (unsigned long long)counts[CW_BAD]);
    return NGSQ_OK;
}

// Phase 3a: the mates, by section 27's keys, sort, run check and search over this command's classes
int MarkdupRun::match() {
    const uint64_t n = R.records;
    BHIP(d_mate.reserve(n));
    BHIP(hipEventRecord(ev.e[0], st));
    BHIP(launch_markdup_key(R.d_addr.p, d_cls.p, d_end.p, n, hash_bits, R.d_key.p, d_work.p, st));
    const uint32_t *perm = nullptr;
    BHIP(sort_pairs_u64(R.d_key.p, n, R.sort, st, &perm));
    sort_passes += R.sort.passes_run;
    const uint64_t *skey = R.sort.passes_run & 1u ? R.sort.keys_b.p : R.d_key.p;
    BHIP(launch_collate_run_limit(skey, n, d_work.p, st));
    if (const int rc = read_work()) return rc;
    if (counts[CW_LONG_RUN]) return ngsq_bam_fail(NGSQ_ERR_LIMIT, "markdup: more than %u reads share a name or a name hash", NGSQ_COLLATE_MAX_RUN);
    BHIP(launch_collate_match(skey, perm, R.d_addr.p, d_cls.p, n, d_mate.p, d_work.p, st));
    return timed(&match_ms);
}

// d_list = the records of `kind` in file order, *m their number
int MarkdupRun::list_of(uint32_t kind, uint64_t *m) {
    const uint64_t n = R.records;
    BHIP(R.d_soff.reserve(n + 1));
    BHIP(d_list.reserve(n));
    BHIP(launch_markdup_list_flag(d_end.p, d_mate.p, d_dup.p, n, kind, R.d_soff.p, st));
    BHIP(scan.exclusive_scan(R.d_soff.p, n + 1, st));
    BHIP(launch_markdup_list_fill(d_end.p, d_mate.p, d_dup.p, n, kind, R.d_soff.p, d_list.p, st));
    BHIP(launch_samtext_word(R.d_soff.p, n, hdev() + HW_A, st));
    BHIP(hipStreamSynchronize(st));
    *m = h()[HW_A];
    if (*m > n) return ngsq_bam_fail(NGSQ_ERR_STATE, "markdup: a list of %llu of %llu resident records", (unsigned long long)*m, (unsigned long long)n);
    return NGSQ_OK;
}

// The m entries of d_list, pairs by (hi, lo) or candidates by lo: sorted, cut into runs of equal keys, every run's best value
// found, every other entry marked.  (R.d_key, free behind the match, is the sort's key array; R.d_soff holds the run flags.)
int MarkdupRun::mark(bool pair_entries, uint64_t m) {
    if (!m) return NGSQ_OK;
    BHIP(d_lo.reserve(m));
    BHIP(d_val.reserve(m));
    if (pair_entries) BHIP(d_hi.reserve(m));
    uint64_t *const hi = pair_entries ? d_hi.p : nullptr;
    BHIP(launch_markdup_entry_keys(d_list.p, m, d_mate.p, d_end.p, d_score.p, hi, d_lo.p, d_val.p, st));
    const uint32_t *order = nullptr;
    if (pair_entries) {
        // 128 bits in two stable sorts: the high word, then the low word gathered through the first order; the orders composed
        const uint32_t *first = nullptr, *second = nullptr;
        BHIP(hipMemcpyAsync(R.d_key.p, d_hi.p, m * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
        BHIP(sort_pairs_u64(R.d_key.p, m, R.sort, st, &first));
        sort_passes += R.sort.passes_run;
        BHIP(d_first.reserve(m));
        BHIP(d_order.reserve(m));
        BHIP(hipMemcpyAsync(d_first.p, first, m * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        BHIP(launch_markdup_gather(d_lo.p, d_first.p, m, R.d_key.p, st));
        BHIP(sort_pairs_u64(R.d_key.p, m, R.sort, st, &second));
        sort_passes += R.sort.passes_run;
        BHIP(launch_markdup_compose(d_first.p, second, m, d_order.p, st));
        order = d_order.p;
    } else {
        BHIP(hipMemcpyAsync(R.d_key.p, d_lo.p, m * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
        BHIP(sort_pairs_u64(R.d_key.p, m, R.sort, st, &order));
        sort_passes += R.sort.passes_run;
    }
    BHIP(R.d_soff.reserve(m + 1));
    BHIP(launch_markdup_heads(order, hi, d_lo.p, m, R.d_soff.p, st));
    BHIP(scan.exclusive_scan(R.d_soff.p, m + 1, st));
    BHIP(d_best.reserve(m));
    BHIP(hipMemsetAsync(d_best.p, 0, m * sizeof(unsigned long long), st));
    BHIP(launch_markdup_best(order, R.d_soff.p, d_val.p, m, d_best.p, st));
    BHIP(launch_markdup_mark(order, R.d_soff.p, d_val.p, d_best.p, d_list.p, d_mate.p, m, pair_entries, d_dup.p, d_work.p, st));
    return NGSQ_OK;
}

// Phase 3b: the pair mark, the fragment mark, the flag bytes
int MarkdupRun::marks() {
    const uint64_t n = R.records;
    BHIP(d_dup.reserve(n));
    BHIP(hipEventRecord(ev.e[0], st));
    BHIP(hipMemsetAsync(d_dup.p, 0, n, st));
    if (const int rc = list_of(MK_LEAD, &pairs)) return rc;
    if (const int rc = mark(true, pairs)) return rc;
    if (const int rc = list_of(MK_CANDIDATE, &candidates)) return rc;
    if (const int rc = mark(false, candidates)) return rc;
    BHIP(launch_markdup_apply(R.d_addr.p, d_dup.p, n, st));
    if (const int rc = timed(&mark_ms)) return rc;
    if (candidates != counts[MW_CANDIDATES] || 2 * pairs > candidates)
        return ngsq_bam_fail(NGSQ_ERR_STATE, "markdup: %llu pairs and %llu listed candidates of %llu counted ones", (unsigned long long)pairs,
                             (unsigned long long)candidates, (unsigned long long)counts[MW_CANDIDATES]);
    return NGSQ_OK;
}

// Phase 4's order: every record, or with `remove` the survivors, in file order
int MarkdupRun::order_out() {
    const uint64_t n = R.records;
    out_records = n;
    if (remove) {
        if (const int rc = list_of(MK_SURVIVOR, &out_records)) return rc;
    } else {
        BHIP(d_list.reserve(n));
        BHIP(launch_sort_iota(d_list.p, n, st));
    }
    if (R.order_given(d_list.p, out_records, &out_bytes)) return ngsq_bam_fail(R.code, "%s", R.err.c_str());
    if (!remove && out_bytes != R.rec_bytes)
        return ngsq_bam_fail(NGSQ_ERR_STATE, "markdup: the records take %llu bytes in the output's order, %llu resident", (unsigned long long)out_bytes,
                             (unsigned long long)R.rec_bytes);
    return NGSQ_OK;
}

} // namespace

extern "C" uint64_t ngsq_markdup_bytes_per_record(void) { return MARKDUP_BYTES_PER_RECORD; }

extern "C" int ngsq_bam_mark_duplicates(ngsq_bam *b, ngsq_ctx *c, int fd, const ngsq_markdup_options *opt, ngsq_markdup_report *out) {
    if (out) memset(out, 0, sizeof *out);
    if (!b || !c || !opt || fd < 0) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    if (opt->struct_size != sizeof *opt)
        return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "ngsq_markdup_options.struct_size is %u, not %zu", opt->struct_size, sizeof *opt);
    if (opt->remove > 1u) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "remove is 0 or 1");
    if (opt->hash_bits > 63u) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "hash_bits is 0 to 63");
    if (opt->reserved) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "ngsq_markdup_options.reserved is %u, not 0", opt->reserved);
    if (const int rc = require_fresh_reader(b, "a BAM file with its duplicates marked is written")) return rc;
    const double t_begin = now_ms();
    if (b->header_text.size() > 0x7FFFFFFFull) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "%sheader text longer than 2^31 - 1 bytes", READ_CTX);
    // the header stream: the text and the reference list as the file holds them
    std::string hs("BAM\1", 4);
    put32(hs, (uint32_t)b->header_text.size());
    hs += b->header_text;
    hs += b->ref_table;
    BHIP(hipSetDevice(c->device));
    MarkdupRun r;
    r.b = b;
    r.c = c;
    r.hash_bits = opt->hash_bits;
    r.remove = opt->remove != 0;
    r.R.budget = opt->memory_budget;
    const uint64_t piece_bytes = std::min(opt->piece_bytes ? opt->piece_bytes : SORT_PIECE_DEFAULT, SORT_PIECE_MAX);
    int rc = r.begin();
    if (rc == NGSQ_OK) rc = r.walk(opt->max_records, opt->batch_records ? opt->batch_records : BATCH_RECORDS);
    const double walk_ms = now_ms() - t_begin;
    if (rc == NGSQ_OK && r.R.records) {
        rc = r.ends();
        if (rc == NGSQ_OK) rc = r.match();
        if (rc == NGSQ_OK) rc = r.marks();
        if (rc == NGSQ_OK) rc = r.order_out();
    }
    bool writing = false;
    if (rc == NGSQ_OK) {
        SortResident &R = r.R;
        writing = true;
        if (R.write_begin(fd, hs, piece_bytes, r.out_bytes) || R.write_records(r.out_records, r.out_bytes) || R.write_end())
            rc = ngsq_bam_fail(R.code, "%s", R.err.c_str());
    }
    if (writing) {
        const int before = rc;
        rc = r.R.finish(rc, fd);
        if (rc != before) ngsq_bam_fail(rc, "%s", r.R.err.c_str());
    }
    if (out) {
        const uint64_t *k = r.counts;
        out->records = r.R.records;
        out->candidates = k[MW_CANDIDATES];
        out->pairs = r.pairs;
        out->fragments = k[MW_CANDIDATES] - 2 * r.pairs;
        out->duplicate_pairs = k[MW_DUP_PAIRS];
        out->duplicate_fragments = k[MW_DUP_FRAGMENTS];
        out->duplicate_records = k[MW_DUP_FRAGMENTS] + 2 * k[MW_DUP_PAIRS];
        out->cleared = k[MW_CLEARED];
        out->ambiguous = k[CW_AMBIGUOUS];
        out->name_collisions = k[CW_COLLISIONS];
        out->duplication = k[MW_CANDIDATES] ? (double)out->duplicate_records / (double)k[MW_CANDIDATES] : 0.0;
        out->batches = r.batches;
        out->resident_bytes = r.R.rec_bytes + r.R.records * MARKDUP_BYTES_PER_RECORD;
        out->sort_passes = r.sort_passes;
        out->pieces = r.R.pieces;
        out->blocks = r.R.z.enc.blocks;
        out->stored_blocks = r.R.z.enc.stored;
        out->bam_bytes = r.R.z.bam_bytes;
        out->compressed_bytes = r.R.z.enc.comp_bytes;
        out->scan_ms = r.scan_ms;
        out->walk_ms = walk_ms;
        out->ends_ms = r.ends_ms;
        out->match_ms = r.match_ms;
        out->mark_ms = r.mark_ms;
        out->gather_ms = r.R.gather_ms;
        out->deflate_ms = r.R.z.deflate_ms;
        out->d2h_ms = r.R.z.w.copy_ms;
        out->write_ms = r.R.z.w.write_ms;
        out->total_ms = now_ms() - t_begin;
    }
    return rc;
}
