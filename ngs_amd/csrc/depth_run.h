// depth_run.h -- what the two drivers of `ngs depth` share (depth.cpp: per-base runs; depth_windows.cpp:
// means per window or BED interval, section 24): the device side of a call up to the difference array of the sequence at
// hand -- names, state words, the order check, activate / add -- the output stage the text collects in, and the two walks, one
// over the whole file and one over a region's chunks.  A walk does not know what is written: it tells its driver when the
// window at hand is final and when a sequence or region has had no record (the two hooks).
#pragma once

#include "../../include/ngsq_depth.h"

#include <string>
#include <vector>

#include "depth_kernels.h"
#include "device_out.h"
#include "ingest_consumer.h"
#include "view_kernels.h"

namespace ngsq {

constexpr uint64_t DEPTH_BATCH_RECORDS = (uint64_t)1 << 20;
constexpr uint64_t DEPTH_COALESCE_GAP = (uint64_t)64 << 20; // as `ngs view`
constexpr uint64_t DEPTH_TEXT_JOB = (uint64_t)32 << 20;     // a text buffer goes to the writer once it holds this much

inline uint64_t depth_round_up(uint64_t v, uint64_t g) { return (v + g - 1) / g * g; }

struct DepthRun {
    ngsq_bam *b = nullptr;
    ngsq_ctx *c = nullptr;
    hipStream_t st = nullptr;
    uint32_t exclude = 0, min_mapq = 0;
    uint64_t batch_records = 0, tile = 0;
    // The window the whole-file walk gives every sequence: its length, or 0 for a sequence nothing is written of.  count_empty:
    // the records of a sequence without a window are still counted (k_depth_count).
    std::vector<uint32_t> seq_len;
    bool count_empty = false;
    // the sequence names on the device, the state words, the words the host reads
    DevArray<char> d_names;
    std::vector<uint64_t> name_off;
    DevArray<DepthState> d_state;
    MappedBuf hw;
    // the window at hand
    DevArray<int32_t> d_diff;
    DepthWindow win{-1, 0, 0, nullptr};
    bool active = false;
    uint64_t win_records = 0; // records of the batches added to the window: each starts at most two runs
    // a region's selection (view_kernels.h)
    DevArray<ngsq_view_chunk> d_chunks;
    DevArray<uint8_t> d_keep;
    DevArray<unsigned long long> d_kept;
    // the output stage: two text buffers, the slots, the writer
    DevArray<char> d_text[2];
    uint64_t used = 0;     // bytes of the job being filled
    bool acquired = false; // its slot's buffer is ours
    JobSlots slots;
    DeviceWriter w; // (behind the text: it ends, and its copies with it, before the buffers go)
    HipEvents<8> ev; // brackets: add 0/1, the driver's reduction 2/3 (and a batch's order check, waited for at once), size 4/5, write 6/7
    bool add_pending = false, write_pending = false;
    uint32_t parity = 0;
    // what a report takes from here
    uint64_t records_scanned = 0, batches = 0, ranges = 0, text_bytes = 0;
    double scan_ms = 0, add_ms = 0, format_ms = 0;
    StreamDrain drain; // (behind every array the stream uses)

    void add_times() {
        float ms = 0;
        if (add_pending && hipEventElapsedTime(&ms, ev.e[0], ev.e[1]) == hipSuccess) add_ms += ms;
        if (write_pending && hipEventElapsedTime(&ms, ev.e[6], ev.e[7]) == hipSuccess) format_ms += ms;
        add_pending = write_pending = false;
    }
    const unsigned long long *host() const { return static_cast<const unsigned long long *>(hw.h); }
    unsigned long long *host_dev() const { return static_cast<unsigned long long *>(hw.dev); }
    const char *name_of(uint32_t ref) const { return d_names.p + name_off[ref]; }
    uint32_t name_len(uint32_t ref) const { return (uint32_t)(name_off[ref + 1] - name_off[ref]); }

    // The device side of a call and its writer thread.  longest: the longest window there will be.
    int begin(ngsq_bam *bam, ngsq_ctx *ctx, int fd, uint64_t longest) {
        b = bam;
        c = ctx;
        st = ctx->stream;
        drain.s = st;
        std::string names;
        for (const std::string &n : b->ref_names) {
            name_off.push_back(names.size());
            names += n;
        }
        name_off.push_back(names.size());
        BHIP(d_names.reserve(names.size() + 1));
        if (!names.empty()) BHIP(hipMemcpy(d_names.p, names.data(), names.size(), hipMemcpyHostToDevice));
        DepthState s0{};
        s0.bad_order = ~0ull;
        s0.lo_ref = INT32_MAX;
        s0.hi_ref = -1;
        BHIP(d_state.reserve(1));
        BHIP(hipMemcpy(d_state.p, &s0, sizeof s0, hipMemcpyHostToDevice));
        BHIP(hw.reserve(DEPTH_HOST_WORDS * sizeof(unsigned long long)));
        memset(hw.h, 0, DEPTH_HOST_WORDS * sizeof(unsigned long long));
        BHIP(d_diff.reserve(longest + 1 + DEPTH_GRANULE));
        BHIP(slots.create());
        for (auto &e : ev.e) BHIP(hipEventCreate(&e));
        BHIP(w.start(fd, c->device));
        return NGSQ_OK;
    }

    // a walk's first record is compared with none
    int reset_walk() {
        BHIP(hipMemsetAsync(d_state.p->carry, 0, sizeof d_state.p->carry, st));
        return NGSQ_OK;
    }

    // The order of a batch, and the sequences of its placed records: [*lo, *hi], *hi < 0 when it has none.
    int batch_order(const ngsq_batch &bt, int32_t *lo, int32_t *hi) {
        BHIP(hipEventRecord(ev.e[2], st));
        BHIP(launch_depth_order(bt, d_state.p, parity, host_dev(), st));
        BHIP(hipEventRecord(ev.e[3], st));
        BHIP(hipEventSynchronize(ev.e[3]));
        parity ^= 1u;
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.e[2], ev.e[3]) == hipSuccess) add_ms += ms;
        add_times();
        const unsigned long long *h = host();
        if (h[0] != ~0ull)
            return ngsq_bam_fail(NGSQ_ERR_UNSORTED, "reading BAM record: record %llu (0-based) is out of coordinate order: the input BAM must be coordinate-sorted to compute depth",
                                 h[0]);
        *lo = (int32_t)(uint32_t)h[1];
        *hi = std::min<int32_t>((int32_t)(uint32_t)h[2], (int32_t)b->ref_lens.size() - 1);
        return NGSQ_OK;
    }

    // positions [lo, lo + len) of sequence ref become the window at hand: its differences are zeroed
    int activate(int32_t ref, uint32_t lo, uint32_t len) {
        win = DepthWindow{ref, lo, len, nullptr};
        active = true;
        win_records = 0;
        if (!len) return NGSQ_OK;
        BHIP(d_diff.reserve((uint64_t)len + 1 + DEPTH_GRANULE)); // (reserved in begin(): does not move)
        win.diff = d_diff.p;
        BHIP(hipMemsetAsync(win.diff, 0, ((size_t)len + 1) * sizeof(int32_t), st));
        return NGSQ_OK;
    }

    int add(const ngsq_batch &bt, const uint8_t *keep) {
        if (!win.len) {
            if (count_empty) BHIP(launch_depth_count(bt, keep, win.ref, exclude, min_mapq, d_state.p, st));
            return NGSQ_OK;
        }
        add_times(); // (a sync lies between two adds: the batch's order check, or the tiles of the sequence in front)
        BHIP(hipEventRecord(ev.e[0], st));
        BHIP(launch_depth_add(bt, keep, win, exclude, min_mapq, d_state.p, st));
        BHIP(hipEventRecord(ev.e[1], st));
        add_pending = true;
        win_records += bt.n_records;
        return NGSQ_OK;
    }

    // the job being filled goes to the writer
    int submit() {
        if (!used) return NGSQ_OK;
        BHIP(slots.submit(w, d_text[slots.slot()].p, used, st));
        text_bytes += used;
        used = 0;
        acquired = false;
        return NGSQ_OK;
    }

    // `bytes` more fit behind the `used` bytes of the job being filled.  *more = false: the writer has failed (its error is read at the end).
    int room(uint64_t bytes, bool *more) {
        if (used && used + bytes > d_text[slots.slot()].cap)
            if (const int rc = submit()) return rc;
        if (!acquired) {
            if (!slots.acquire(&w) || w.werr) {
                *more = false;
                return NGSQ_OK;
            }
            acquired = true;
        }
        if (!used) BHIP(d_text[slots.slot()].reserve(std::max(bytes, DEPTH_TEXT_JOB) + 8)); // (nothing to keep, and the slot's last job has been copied)
        return NGSQ_OK;
    }

    // The end of a call whose work gave `rc`: the last job handed over, the stream drained, every queued copy written (or skipped
    // after a failed write), the writer's own errors reported.
    int finish(int rc) {
        if (rc == NGSQ_OK) rc = submit();
        if (rc == NGSQ_OK) {
            const hipError_t e = hipStreamSynchronize(st);
            if (e != hipSuccess) rc = ngsq_bam_fail(NGSQ_ERR_DEVICE, "hipStreamSynchronize: %s", hipGetErrorString(e));
            add_times();
        }
        const WriterEnd end = w.end();
        if (rc == NGSQ_OK && end.herr != hipSuccess) rc = ngsq_bam_fail(NGSQ_ERR_DEVICE, "copying the depth text to the host: %s", hipGetErrorString(end.herr));
        if (rc == NGSQ_OK && end.werr) rc = ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "writing depth to stream: %s (os error %d)", strerror(end.werr), end.werr);
        return rc;
    }
};

// The hooks of a walk, as members of the driver `D`:
//   int window_final(bool *more)       the window at hand (run().win, its records added) is final: write it
//   int no_record(uint32_t ref, uint32_t lo, uint32_t hi, bool *more)
//                                      positions [lo, hi) of sequence ref, of which no record was seen: write them
// Both clear *more once the writer has failed, and are not called after that.

// The whole file: every sequence of the header in header order.
template <class D> int depth_walk_file(D &d) {
    DepthRun &r = d.run();
    const uint32_t n_refs = (uint32_t)r.b->ref_lens.size();
    uint32_t next_ref = 0; // the first sequence nothing has been written of
    bool more = true;
    auto finish_active = [&]() -> int {
        if (!r.active) return NGSQ_OK;
        next_ref = (uint32_t)r.win.ref + 1;
        return d.window_final(&more);
    };
    while (more) {
        ngsq_batch bt;
        const double s0 = now_ms();
        const int rc = ngsq_bam_next_batch_device(r.b, r.c, r.batch_records, &bt);
        r.scan_ms += now_ms() - s0;
        if (rc) return rc;
        if (!bt.n_records) break;
        r.records_scanned += bt.n_records;
        r.batches++;
        int32_t lo = 0, hi = -1;
        if (const int rc2 = r.batch_order(bt, &lo, &hi)) return rc2;
        // (in order: lo is the sequence at hand or a later one)
        for (int64_t ref = std::max<int64_t>(lo, r.active ? r.win.ref : (int64_t)next_ref); ref <= hi && more; ref++) {
            if (!r.active || r.win.ref != ref) {
                if (const int rc2 = finish_active()) return rc2;
                for (; next_ref < (uint32_t)ref && more; next_ref++)
                    if (const int rc2 = d.no_record(next_ref, 0, r.seq_len[next_ref], &more)) return rc2;
                if (const int rc2 = r.activate((int32_t)ref, 0, r.seq_len[ref])) return rc2;
            }
            if (const int rc2 = r.add(bt, nullptr)) return rc2;
        }
    }
    if (const int rc = finish_active()) return rc;
    for (; next_ref < n_refs && more; next_ref++)
        if (const int rc = d.no_record(next_ref, 0, r.seq_len[next_ref], &more)) return rc;
    return NGSQ_OK;
}

// One region: positions [lo, hi) of sequence ref, its records found through the merged chunks of the query.
template <class D>
int depth_walk_region(D &d, uint32_t ref, uint64_t start, uint64_t end, uint32_t lo, uint32_t hi, const std::vector<ngsq_view_chunk> &chunks,
                      uint64_t coalesce_gap) {
    DepthRun &r = d.run();
    bool more = true;
    if (chunks.empty()) return d.no_record(ref, lo, hi, &more);
    BHIP(r.d_chunks.reserve(chunks.size()));
    BHIP(r.d_kept.reserve(1));
    BHIP(hipMemsetAsync(r.d_kept.p, 0, sizeof(unsigned long long), r.st));
    BHIP(hipMemcpyAsync(r.d_chunks.p, chunks.data(), chunks.size() * sizeof(ngsq_view_chunk), hipMemcpyHostToDevice, r.st));
    BHIP(hipStreamSynchronize(r.st)); // (chunks is the caller's)
    BHIP(r.d_keep.reserve(r.batch_records));
    ViewRegion region{};
    region.chunks = r.d_chunks.p;
    region.n_chunks = (uint32_t)chunks.size();
    region.ref_id = (int32_t)ref;
    region.start = start;
    region.end = end;
    if (const int rc = r.activate((int32_t)ref, lo, hi - lo)) return rc;
    // merged chunks whose gap in the file is below coalesce_gap share a walk
    for (size_t k = 0; k < chunks.size();) {
        size_t j = k;
        while (coalesce_gap > 1 && j + 1 < chunks.size() && (chunks[j + 1].begin >> 16) - (chunks[j].end >> 16) < coalesce_gap) j++;
        region.lo = chunks[k].begin; // (a walk hands out records behind its end, to the end of their block: the next walk's)
        region.hi = chunks[j].end;
        if (const int rc = ngsq_bam_range_begin(r.b, r.c, chunks[k].begin, chunks[j].end)) return rc;
        if (const int rc = r.reset_walk()) return rc;
        r.ranges++;
        for (;;) {
            ngsq_batch bt;
            const double s0 = now_ms();
            const int rc = ngsq_bam_next_batch_device(r.b, r.c, r.batch_records, &bt);
            r.scan_ms += now_ms() - s0;
            if (rc) return rc;
            if (!bt.n_records) break;
            r.records_scanned += bt.n_records;
            r.batches++;
            int32_t blo = 0, bhi = -1;
            if (const int rc2 = r.batch_order(bt, &blo, &bhi)) return rc2;
            if (blo > (int32_t)ref || bhi < (int32_t)ref) continue; // no record of the region's sequence
            BHIP(r.d_keep.reserve(bt.n_records));
            BHIP(launch_view_select(bt, region, r.d_keep.p, r.d_kept.p, r.st));
            if (const int rc2 = r.add(bt, r.d_keep.p)) return rc2;
        }
        k = j + 1;
    }
    return d.window_final(&more);
}

// The query of a call, in front of the first byte and of any GPU work: the region's sequence, its 1-based bounds, the positions
// [lo, hi) it stands for and its merged chunks.  The errors are those of ngsq_bam_query_chunks.
struct DepthRegion {
    uint32_t ref = 0, lo = 0, hi = 0;
    uint64_t start = 0, end = 0;
    std::vector<ngsq_view_chunk> chunks;
};
inline int depth_region(ngsq_bam *b, const char *query, const char *bai_path, DepthRegion *g) {
    uint64_t n = 0;
    if (const int rc = ngsq_bam_query_chunks(b, bai_path, query, &g->ref, &g->start, &g->end, nullptr, 0, &n)) return rc;
    g->chunks.resize(n);
    if (n)
        if (const int rc = ngsq_bam_query_chunks(b, bai_path, query, &g->ref, &g->start, &g->end, g->chunks.data(), n, &n)) return rc;
    const uint64_t len = b->ref_lens[g->ref];
    g->lo = (uint32_t)std::min<uint64_t>(g->start - 1, len);
    g->hi = (uint32_t)std::min<uint64_t>(g->end, len);
    return NGSQ_OK;
}

} // namespace ngsq
