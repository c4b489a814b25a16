// depth.cpp -- ngsq_bam_depth (include/ngsq_depth.h): the file is walked once through the device ingest, or
// a region's chunks by the range walks of `ngs view`; every batch is checked for order and its first and last sequence come to
// the host in pinned words; the records of the sequence at hand are added to its difference array; a sequence is final when a
// record of a later one, or the walk's end, has been seen, and is then taken through the run path tile by tile: run starts and
// depths, line sizes, their scan, the lines.  The text collects in the two device buffers of the output stage (device_out.h) and
// goes to the file while the next tiles are made.
#include "../../include/ngsq_depth.h"

#include <string>
#include <vector>

#include "depth_kernels.h"
#include "device_out.h"
#include "ingest_consumer.h"
#include "view_kernels.h"

using namespace ngsq;

namespace {

constexpr uint64_t BATCH_RECORDS = (uint64_t)1 << 20;
constexpr uint64_t COALESCE_GAP = (uint64_t)64 << 20; // as `ngs view`
constexpr uint64_t TEXT_JOB = (uint64_t)32 << 20;     // a text buffer goes to the writer once it holds this much

uint64_t round_up(uint64_t v, uint64_t g) { return (v + g - 1) / g * g; }

struct DepthRun {
    ngsq_bam *b = nullptr;
    ngsq_ctx *c = nullptr;
    hipStream_t st = nullptr;
    uint32_t exclude = 0, min_mapq = 0;
    uint64_t batch_records = 0, tile = 0;
    // the sequence names on the device, the state words, the words the host reads
    DevArray<char> d_names;
    std::vector<uint64_t> name_off;
    DevArray<DepthState> d_state;
    MappedBuf hw;
    // the window at hand and the run path's arrays
    DevArray<int32_t> d_diff, d_bsum, d_rdepth;
    DevArray<uint32_t> d_bcnt, d_rstart;
    DevArray<uint64_t> d_off;
    ScanScratch scan;
    DepthTileArrays arr{};
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
    HipEvents<8> ev; // brackets: add 0/1, runs 2/3 (and a batch's order check, waited for at once), size 4/5, write 6/7
    bool add_pending = false, write_pending = false;
    uint32_t parity = 0;
    ngsq_depth_report rep{};
    StreamDrain drain; // (behind every array the stream uses)

    void add_times() {
        float ms = 0;
        if (add_pending && hipEventElapsedTime(&ms, ev.e[0], ev.e[1]) == hipSuccess) rep.add_ms += ms;
        if (write_pending && hipEventElapsedTime(&ms, ev.e[6], ev.e[7]) == hipSuccess) rep.format_ms += ms;
        add_pending = write_pending = false;
    }
    const unsigned long long *host() const { return static_cast<const unsigned long long *>(hw.h); }
    unsigned long long *host_dev() const { return static_cast<unsigned long long *>(hw.dev); }
    const char *name_of(uint32_t ref) const { return d_names.p + name_off[ref]; }
    uint32_t name_len(uint32_t ref) const { return (uint32_t)(name_off[ref + 1] - name_off[ref]); }

    int begin(ngsq_bam *bam, ngsq_ctx *ctx, int fd, uint64_t longest);
    int reset_walk();
    int batch_order(const ngsq_batch &bt, int32_t *lo, int32_t *hi);
    int activate(int32_t ref, uint32_t lo, uint32_t len);
    int add(const ngsq_batch &bt, const uint8_t *keep);
    int room(uint64_t bytes, bool *more);
    int submit();
    int finalize(bool *more);
    int zero_line(uint32_t ref, uint32_t start, uint32_t end, bool *more);
    int finish(int rc);
};

// The device side of a call and its writer thread.  longest: the longest window there will be.
int DepthRun::begin(ngsq_bam *bam, ngsq_ctx *ctx, int fd, uint64_t longest) {
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
    // the run path's arrays for the largest tile there will be
    const uint64_t t = std::min(tile, round_up(std::max<uint64_t>(longest, 1), DEPTH_GRANULE));
    BHIP(d_bsum.reserve(t / DEPTH_GRANULE));
    BHIP(d_bcnt.reserve(t / DEPTH_GRANULE));
    BHIP(d_rstart.reserve(t + 1));
    BHIP(d_rdepth.reserve(t + 1));
    BHIP(d_off.reserve(t + 2));
    arr = DepthTileArrays{d_bsum.p, d_bcnt.p, d_rstart.p, d_rdepth.p, d_off.p};
    BHIP(d_diff.reserve(longest + 1 + DEPTH_GRANULE));
    BHIP(slots.create());
    for (auto &e : ev.e) BHIP(hipEventCreate(&e));
    BHIP(w.start(fd, c->device));
    return NGSQ_OK;
}

// a walk's first record is compared with none
int DepthRun::reset_walk() {
    BHIP(hipMemsetAsync(d_state.p->carry, 0, sizeof d_state.p->carry, st));
    return NGSQ_OK;
}

// The order of a batch, and the sequences of its placed records: [*lo, *hi], *hi < 0 when it has none.
int DepthRun::batch_order(const ngsq_batch &bt, int32_t *lo, int32_t *hi) {
    BHIP(hipEventRecord(ev.e[2], st));
    BHIP(launch_depth_order(bt, d_state.p, parity, host_dev(), st));
    BHIP(hipEventRecord(ev.e[3], st));
    BHIP(hipEventSynchronize(ev.e[3]));
    parity ^= 1u;
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev.e[2], ev.e[3]) == hipSuccess) rep.add_ms += ms;
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
int DepthRun::activate(int32_t ref, uint32_t lo, uint32_t len) {
    win = DepthWindow{ref, lo, len, nullptr};
    active = true;
    win_records = 0;
    if (!len) return NGSQ_OK;
    BHIP(d_diff.reserve((uint64_t)len + 1 + DEPTH_GRANULE)); // (reserved in begin(): does not move)
    win.diff = d_diff.p;
    BHIP(hipMemsetAsync(win.diff, 0, ((size_t)len + 1) * sizeof(int32_t), st));
    return NGSQ_OK;
}

int DepthRun::add(const ngsq_batch &bt, const uint8_t *keep) {
    if (!win.len) return NGSQ_OK;
    add_times(); // (a sync lies between two adds: the batch's order check, or the tiles of the sequence in front)
    BHIP(hipEventRecord(ev.e[0], st));
    BHIP(launch_depth_add(bt, keep, win, exclude, min_mapq, d_state.p, st));
    BHIP(hipEventRecord(ev.e[1], st));
    add_pending = true;
    win_records += bt.n_records;
    return NGSQ_OK;
}

// the job being filled goes to the writer
int DepthRun::submit() {
    if (!used) return NGSQ_OK;
    BHIP(slots.submit(w, d_text[slots.slot()].p, used, st));
    rep.text_bytes += used;
    used = 0;
    acquired = false;
    return NGSQ_OK;
}

// `bytes` more fit behind the `used` bytes of the job being filled.  *more = false: the writer has failed (its error is read at the end).
int DepthRun::room(uint64_t bytes, bool *more) {
    if (used && used + bytes > d_text[slots.slot()].cap)
        if (const int rc = submit()) return rc;
    if (!acquired) {
        if (!slots.acquire(&w) || w.werr) {
            *more = false;
            return NGSQ_OK;
        }
        acquired = true;
    }
    if (!used) BHIP(d_text[slots.slot()].reserve(std::max(bytes, TEXT_JOB) + 8)); // (nothing to keep, and the slot's last job has been copied)
    return NGSQ_OK;
}

// The window at hand is final: tile by tile through the run path.
int DepthRun::finalize(bool *more) {
    const DepthWindow wn = win;
    active = false;
    win = DepthWindow{-1, 0, 0, nullptr};
    if (!wn.len) return NGSQ_OK;
    const uint32_t final_end = wn.lo + wn.len, nl = name_len((uint32_t)wn.ref);
    const char *const name = name_of((uint32_t)wn.ref);
    rep.sequences++;
    for (uint64_t t0 = 0; t0 < wn.len && *more; t0 += tile) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(tile, wn.len - t0);
        const bool final = t0 + n == wn.len;
        BHIP(hipEventRecord(ev.e[2], st));
        BHIP(launch_depth_runs(wn, t0, n, arr, d_state.p, st));
        BHIP(hipEventRecord(ev.e[3], st));
        BHIP(hipEventRecord(ev.e[4], st));
        // lines + 1 entries at most: the run held back, the window's first position, two run starts per record
        const uint64_t entries = std::min<uint64_t>((uint64_t)n + 2, 2 * win_records + 3);
        BHIP(launch_depth_size(entries, final, final_end, nl, arr, d_state.p, st));
        BHIP(scan.exclusive_scan(arr.off, entries, st));
        BHIP(launch_depth_total(final, arr, d_state.p, host_dev(), st));
        BHIP(hipEventRecord(ev.e[5], st));
        BHIP(hipEventSynchronize(ev.e[5]));
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.e[2], ev.e[3]) == hipSuccess) rep.runs_ms += ms;
        if (hipEventElapsedTime(&ms, ev.e[4], ev.e[5]) == hipSuccess) rep.format_ms += ms;
        add_times();
        const uint64_t bytes = host()[0], lines = host()[1];
        rep.tiles++;
        if (lines + 1 > entries) return ngsq_bam_fail(NGSQ_ERR_STATE, "the run path gave more lines than the window's records allow");
        if (!lines) continue;
        if (const int rc = room(bytes, more)) return rc;
        if (!*more) break;
        BHIP(hipEventRecord(ev.e[6], st));
        BHIP(launch_depth_write(d_text[slots.slot()].p + used, (uint32_t)lines, final, final_end, name, nl, arr, st));
        BHIP(hipEventRecord(ev.e[7], st));
        write_pending = true;
        used += bytes;
        rep.runs += lines;
        if (used >= TEXT_JOB)
            if (const int rc = submit()) return rc;
    }
    return NGSQ_OK;
}

// a sequence or region no record was seen of: one line, in closed form
int DepthRun::zero_line(uint32_t ref, uint32_t start, uint32_t end, bool *more) {
    if (start >= end || !*more) return NGSQ_OK;
    const uint64_t bytes = name_len(ref) + 4u + depth_digits(start) + depth_digits(end) + 1u;
    if (const int rc = room(bytes, more)) return rc;
    if (!*more) return NGSQ_OK;
    BHIP(launch_depth_zero_line(d_text[slots.slot()].p + used, name_of(ref), name_len(ref), start, end, st));
    used += bytes;
    rep.runs++;
    rep.sequences++;
    if (used >= TEXT_JOB) return submit();
    return NGSQ_OK;
}

// The end of a call whose work gave `rc`: the last job handed over, the stream drained, every queued copy written (or skipped
// after a failed write), the writer's own errors reported.
int DepthRun::finish(int rc) {
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

// The whole file: every sequence of the header in header order.
int walk_file(DepthRun &r) {
    const uint32_t n_refs = (uint32_t)r.b->ref_lens.size();
    uint32_t next_ref = 0; // the first sequence nothing has been written of
    bool more = true;
    auto finish_active = [&]() -> int {
        if (!r.active) return NGSQ_OK;
        next_ref = (uint32_t)r.win.ref + 1;
        return r.finalize(&more);
    };
    while (more) {
        ngsq_batch bt;
        const double s0 = now_ms();
        const int rc = ngsq_bam_next_batch_device(r.b, r.c, r.batch_records, &bt);
        r.rep.scan_ms += now_ms() - s0;
        if (rc) return rc;
        if (!bt.n_records) break;
        r.rep.records_scanned += bt.n_records;
        r.rep.batches++;
        int32_t lo = 0, hi = -1;
        if (const int rc2 = r.batch_order(bt, &lo, &hi)) return rc2;
        // (in order: lo is the sequence at hand or a later one)
        for (int64_t ref = std::max<int64_t>(lo, r.active ? r.win.ref : (int64_t)next_ref); ref <= hi && more; ref++) {
            if (!r.active || r.win.ref != ref) {
                if (const int rc2 = finish_active()) return rc2;
                for (; next_ref < (uint32_t)ref && more; next_ref++)
                    if (const int rc2 = r.zero_line(next_ref, 0, r.b->ref_lens[next_ref], &more)) return rc2;
                if (const int rc2 = r.activate((int32_t)ref, 0, r.b->ref_lens[ref])) return rc2;
            }
            if (const int rc2 = r.add(bt, nullptr)) return rc2;
        }
    }
    if (const int rc = finish_active()) return rc;
    for (; next_ref < n_refs && more; next_ref++)
        if (const int rc = r.zero_line(next_ref, 0, r.b->ref_lens[next_ref], &more)) return rc;
    return NGSQ_OK;
}

// One region: positions [lo, hi) of sequence ref, its records found through the merged chunks of the query.
int walk_region(DepthRun &r, uint32_t ref, uint64_t start, uint64_t end, uint32_t lo, uint32_t hi, const std::vector<ngsq_view_chunk> &chunks,
                uint64_t coalesce_gap) {
    bool more = true;
    if (chunks.empty()) return r.zero_line(ref, lo, hi, &more);
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
        r.rep.ranges++;
        for (;;) {
            ngsq_batch bt;
            const double s0 = now_ms();
            const int rc = ngsq_bam_next_batch_device(r.b, r.c, r.batch_records, &bt);
            r.rep.scan_ms += now_ms() - s0;
            if (rc) return rc;
            if (!bt.n_records) break;
            r.rep.records_scanned += bt.n_records;
            r.rep.batches++;
            int32_t blo = 0, bhi = -1;
            if (const int rc2 = r.batch_order(bt, &blo, &bhi)) return rc2;
            if (blo > (int32_t)ref || bhi < (int32_t)ref) continue; // no record of the region's sequence
            BHIP(r.d_keep.reserve(bt.n_records));
            BHIP(launch_view_select(bt, region, r.d_keep.p, r.d_kept.p, r.st));
            if (const int rc2 = r.add(bt, r.d_keep.p)) return rc2;
        }
        k = j + 1;
    }
    return r.finalize(&more);
}

} // namespace

extern "C" uint64_t ngsq_depth_tile_positions(uint64_t requested) {
    if (!requested) return DEPTH_TILE_DEFAULT;
    return round_up(std::min(requested, DEPTH_TILE_MAX), DEPTH_GRANULE);
}

extern "C" int ngsq_bam_depth(ngsq_bam *b, ngsq_ctx *c, int fd, const char *query, const char *bai_path, uint32_t exclude_flags,
                              uint32_t min_mapq, uint64_t batch_records, uint64_t coalesce_gap, uint64_t tile_positions, ngsq_depth_report *out) {
    if (!b || !c || fd < 0 || exclude_flags > 65535u || min_mapq > 255u) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "null or invalid argument");
    if (out) memset(out, 0, sizeof *out);
    const double t_begin = now_ms();
    if (const int rc = require_fresh_reader(b, "the depth is computed")) return rc;
    if (!ngsq_bam_sorted_by_coordinate(b)) return ngsq_bam_fail(NGSQ_ERR_UNSORTED, "the input BAM must be coordinate-sorted to compute depth");
    // ---- the query and the index, in front of the first byte and of any GPU work
    uint32_t ref = 0, lo = 0, hi = 0;
    uint64_t start = 0, end = 0;
    std::vector<ngsq_view_chunk> chunks;
    if (query) {
        uint64_t n = 0;
        if (const int rc = ngsq_bam_query_chunks(b, bai_path, query, &ref, &start, &end, nullptr, 0, &n)) return rc;
        chunks.resize(n);
        if (n)
            if (const int rc = ngsq_bam_query_chunks(b, bai_path, query, &ref, &start, &end, chunks.data(), n, &n)) return rc;
        const uint64_t len = b->ref_lens[ref];
        lo = (uint32_t)std::min<uint64_t>(start - 1, len);
        hi = (uint32_t)std::min<uint64_t>(end, len);
        if (lo >= hi) { // an empty interval: no line
            if (out) out->total_ms = now_ms() - t_begin;
            return NGSQ_OK;
        }
    }
    uint64_t longest = query ? hi - lo : 0;
    if (!query)
        for (const uint32_t l : b->ref_lens) longest = std::max<uint64_t>(longest, l);
    BHIP(hipSetDevice(c->device));
    DepthRun r;
    r.exclude = exclude_flags;
    r.min_mapq = min_mapq;
    r.batch_records = batch_records ? batch_records : BATCH_RECORDS;
    r.tile = ngsq_depth_tile_positions(tile_positions);
    int rc = r.begin(b, c, fd, longest);
    if (rc == NGSQ_OK) rc = query ? walk_region(r, ref, start, end, lo, hi, chunks, coalesce_gap ? coalesce_gap : COALESCE_GAP) : walk_file(r);
    rc = r.finish(rc);
    if (rc != NGSQ_OK) return rc;
    unsigned long long counted = 0;
    BHIP(hipMemcpy(&counted, &r.d_state.p->counted, sizeof counted, hipMemcpyDeviceToHost));
    if (out) {
        *out = r.rep;
        out->records_counted = counted;
        out->copy_ms = r.w.copy_ms;
        out->write_ms = r.w.write_ms;
        out->total_ms = now_ms() - t_begin;
    }
    return NGSQ_OK;
}
