// depth_windows.cpp -- ngsq_bam_depth_windows (include/ngsq_depth.h): the mean depth of every window of N
// positions, or of every interval of a BED file.  The walks, the order check and the difference array are `ngs depth`'s
// (depth_run.h).  A final window goes through the reduce pass tile by tile: 64-bit prefix sums P of the depth, kept absolute over
// the window by a carry in the device state; --by N takes the sums of the windows that end in the tile, --by BED adds every
// interval's end and takes off its start in whichever tile holds them.  One function writes lines: format_pass().  Windows with
// records, the windows of a sequence or region without a record and BED intervals all reach the text through it, and it alone
// reserves the text buffer, launches the write kernel and advances the byte and line counts.
// ngsq_bam_depth_thresholds is the same driver with K >= 1 thresholds: beside P the reduce pass keeps C_k,
// the count of positions at or above T_k, looked up and carried as P is, and a line has K more columns.  With K = 0 nothing of
// it is reserved or launched.
#include "../../include/ngsq_depth.h"

#include "depth_run.h"
#include "depth_windows_kernels.h"

using namespace ngsq;

namespace {

constexpr uint32_t LINES_GRANULE = DEPTH_BT; // lines of a block of the format pass

// A launcher checks its arguments and returns hipErrorInvalidValue, with nothing launched, when it refuses them: the driver's own
// state is wrong.  The runtime may give the same code for a launch it refuses, so the words name both.
#define WLAUNCH(call)                                                                                                        \
    do {                                                                                                                     \
        const hipError_t e_ = (call);                                                                                        \
        if (e_ == hipErrorInvalidValue)                                                                                      \
            return ngsq_bam_fail(NGSQ_ERR_STATE, "%s: invalid value (the launcher refused its arguments, or the runtime the launch)", #call); \
        if (e_ != hipSuccess) return ngsq_bam_fail(NGSQ_ERR_DEVICE, "%s: %s", #call, hipGetErrorString(e_));                \
    } while (0)

struct WindowsRun {
    DepthRun r;
    uint32_t window = 0;         // >= 1: --by N; 0: the intervals
    uint64_t lines_per_pass = 0; // a multiple of LINES_GRANULE
    // the intervals ordered by sequence, the file's order within one: those of sequence ref are [first[ref], first[ref + 1])
    std::vector<ngsq_depth_interval> sorted;
    std::vector<uint64_t> first;
    DevArray<ngsq_depth_interval> d_iv;
    DevArray<uint64_t> d_acc;
    // the reduce pass
    DevArray<int32_t> d_bdepth;
    DevArray<long long> d_bsum;
    DevArray<uint64_t> d_bP, d_P, d_sum;
    DepthWTileArrays arr{};
    DevArray<DepthWState> d_ws;
    // thresholds (thr.k >= 1 only): the count arrays of the reduce pass, the counts of a tile's windows, of the intervals, the carries
    DepthThresholds thr{};
    DevArray<uint16_t> d_cin;
    DevArray<uint32_t> d_bcnt, d_bC, d_cnt, d_accT;
    DepthTTileArrays tarr{};
    uint64_t cnt_stride = 0; // a row of d_cnt
    DevArray<DepthTState> d_ts;
    uint64_t covered[NGSQ_DEPTH_MAX_THRESHOLDS] = {};
    // the format pass
    DevArray<uint64_t> d_off;
    ScanScratch scan;
    MappedBuf hw;
    HipEvents<2> rev;         // around the reduce kernels queued since the last wait
    bool reduce_open = false; // they bracket kernels whose time has not been read
    ngsq_depth_windows_report rep{};
    StreamDrain drain; // (behind every array the stream uses)

    DepthRun &run() { return r; }
    uint64_t n_windows(uint32_t lo, uint32_t hi) const { return lo < hi ? (uint64_t)(hi - 1) / window - lo / window + 1 : 0; }
    uint64_t n_intervals(uint32_t ref) const { return first[ref + 1] - first[ref]; }
    int begin(ngsq_bam *bam, ngsq_ctx *ctx, int fd, uint64_t longest, uint64_t most_lines);
    void reduce_time();
    int format_pass(uint32_t ref, const DepthLineSource &src, bool *more);
    int window_final(bool *more);
    int no_record(uint32_t ref, uint32_t lo, uint32_t hi, bool *more);
};

// longest: the longest window there will be; most_lines: the most lines one sequence or region has
int WindowsRun::begin(ngsq_bam *bam, ngsq_ctx *ctx, int fd, uint64_t longest, uint64_t most_lines) {
    drain.s = ctx->stream;
    const uint64_t t = std::min(r.tile, depth_round_up(std::max<uint64_t>(longest, 1), DEPTH_GRANULE));
    BHIP(d_bdepth.reserve(t / DEPTH_GRANULE));
    BHIP(d_bsum.reserve(t / DEPTH_GRANULE));
    BHIP(d_bP.reserve(t / DEPTH_GRANULE));
    BHIP(d_P.reserve(t + 1));
    arr = DepthWTileArrays{d_bdepth.p, d_bsum.p, d_bP.p, d_P.p};
    if (window) BHIP(d_sum.reserve(t / window + 2)); // the windows that end in one tile
    BHIP(d_off.reserve(std::min(lines_per_pass, depth_round_up(std::max<uint64_t>(most_lines, 1), LINES_GRANULE)) + 1));
    for (auto &e : rev.e) BHIP(hipEventCreate(&e));
    BHIP(d_ws.reserve(1));
    BHIP(hipMemset(d_ws.p, 0, sizeof(DepthWState)));
    const uint32_t host_words = thr.k ? DEPTHT_HOST_WORDS : DEPTHW_HOST_WORDS;
    BHIP(hw.reserve(host_words * sizeof(unsigned long long)));
    memset(hw.h, 0, host_words * sizeof(unsigned long long));
    if (thr.k) { // sized by K: cin K x tile x 2 bytes, bcnt / bC K x blocks, cnt K x the windows a tile can end, accT K x intervals
        BHIP(d_cin.reserve(thr.k * t));
        BHIP(d_bcnt.reserve(thr.k * (t / DEPTH_GRANULE)));
        BHIP(d_bC.reserve(thr.k * (t / DEPTH_GRANULE)));
        tarr = DepthTTileArrays{d_cin.p, d_bcnt.p, d_bC.p, t, (uint32_t)(t / DEPTH_GRANULE)};
        if (window) {
            cnt_stride = t / window + 2;
            BHIP(d_cnt.reserve(thr.k * cnt_stride));
        }
        BHIP(d_ts.reserve(1));
        BHIP(hipMemset(d_ts.p, 0, sizeof(DepthTState)));
        if (!sorted.empty()) {
            BHIP(d_accT.reserve(thr.k * sorted.size()));
            BHIP(hipMemset(d_accT.p, 0, thr.k * sorted.size() * sizeof(uint32_t)));
        }
    }
    if (!sorted.empty()) {
        BHIP(d_iv.reserve(sorted.size()));
        BHIP(d_acc.reserve(sorted.size()));
        BHIP(hipMemcpy(d_iv.p, sorted.data(), sorted.size() * sizeof(ngsq_depth_interval), hipMemcpyHostToDevice));
        BHIP(hipMemset(d_acc.p, 0, sorted.size() * sizeof(uint64_t)));
    }
    return r.begin(bam, ctx, fd, longest);
}

// (behind a wait for the stream)
void WindowsRun::reduce_time() {
    float ms = 0;
    if (reduce_open && hipEventElapsedTime(&ms, rev.e[0], rev.e[1]) == hipSuccess) rep.reduce_ms += ms;
    reduce_open = false;
}

// The lines of `src`, all of sequence ref, into the text: passes of at most lines_per_pass lines, each sized, scanned, waited for
// once and written.
int WindowsRun::format_pass(uint32_t ref, const DepthLineSource &src, bool *more) {
    const uint32_t nl = r.name_len(ref);
    const char *const name = r.name_of(ref);
    unsigned long long *const hdev = static_cast<unsigned long long *>(hw.dev);
    const unsigned long long *const h = static_cast<const unsigned long long *>(hw.h);
    // with thresholds, the counts of the source's lines: those of the tile's windows, or of the sequence's intervals
    const DepthTLineSource tsrc = src.window ? DepthTLineSource{src, thr.k, d_cnt.p, cnt_stride}
                                             : DepthTLineSource{src, thr.k, d_accT.p ? d_accT.p + first[ref] : nullptr, sorted.size()};
    for (uint64_t k0 = 0; k0 < src.count && *more; k0 += lines_per_pass) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(lines_per_pass, src.count - k0);
        if ((uint64_t)m + 1 > d_off.cap) return ngsq_bam_fail(NGSQ_ERR_STATE, "a format pass of %u lines is larger than its offsets array", m);
        BHIP(hipEventRecord(r.ev.e[4], r.st));
        if (thr.k) WLAUNCH(launch_deptht_size(tsrc, k0, m, nl, d_off.p, d_ws.p, d_ts.p, r.st));
        else WLAUNCH(launch_depthw_size(src, k0, m, nl, d_off.p, d_ws.p, r.st));
        BHIP(scan.exclusive_scan(d_off.p, (uint64_t)m + 1, r.st));
        if (thr.k) WLAUNCH(launch_deptht_total(d_off.p, m, thr.k, d_ws.p, d_ts.p, hdev, r.st));
        else WLAUNCH(launch_depthw_total(d_off.p, m, d_ws.p, hdev, r.st));
        BHIP(hipEventRecord(r.ev.e[5], r.st));
        BHIP(hipEventSynchronize(r.ev.e[5]));
        float ms = 0;
        if (hipEventElapsedTime(&ms, r.ev.e[4], r.ev.e[5]) == hipSuccess) r.format_ms += ms;
        reduce_time();
        r.add_times();
        const uint64_t bytes = h[0];
        rep.depth_sum = h[1];
        for (uint32_t k = 0; k < thr.k; k++) covered[k] = h[DEPTHW_HOST_WORDS + k];
        rep.passes++;
        if (bytes < (uint64_t)m * (nl + 10u + 2u * thr.k)) return ngsq_bam_fail(NGSQ_ERR_STATE, "the size pass gave fewer bytes than its lines need");
        if (const int rc = r.room(bytes, more)) return rc;
        if (!*more) break;
        BHIP(hipEventRecord(r.ev.e[6], r.st));
        if (thr.k) WLAUNCH(launch_deptht_write(r.d_text[r.slots.slot()].p + r.used, tsrc, k0, m, name, nl, d_off.p, r.st));
        else WLAUNCH(launch_depthw_write(r.d_text[r.slots.slot()].p + r.used, src, k0, m, name, nl, d_off.p, r.st));
        BHIP(hipEventRecord(r.ev.e[7], r.st));
        r.write_pending = true;
        r.used += bytes;
        rep.lines += m;
        if (r.used >= DEPTH_TEXT_JOB)
            if (const int rc = r.submit()) return rc;
    }
    return NGSQ_OK;
}

// The window at hand is final: tile by tile through the reduce pass; the sums that are complete go to the format pass.
int WindowsRun::window_final(bool *more) {
    const DepthWindow wn = r.win;
    r.active = false;
    r.win = DepthWindow{-1, 0, 0, nullptr};
    if (!wn.len) return NGSQ_OK;
    const uint32_t ref = (uint32_t)wn.ref, hi = wn.lo + wn.len;
    const uint64_t n_iv = window ? 0 : n_intervals(ref);
    rep.sequences++;
    BHIP(hipMemsetAsync(d_ws.p, 0, DEPTHW_CARRY_BYTES, r.st));
    if (thr.k) BHIP(hipMemsetAsync(d_ts.p, 0, DEPTHT_CARRY_BYTES, r.st));
    for (uint64_t t0 = 0; t0 < wn.len && *more; t0 += r.tile) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(r.tile, wn.len - t0);
        const uint64_t origin = (uint64_t)wn.lo + t0, tile_end = origin + n;
        if (!reduce_open) BHIP(hipEventRecord(rev.e[0], r.st));
        if (thr.k) WLAUNCH(launch_deptht_prefix(wn, t0, n, arr, tarr, thr, d_ws.p, d_ts.p, r.st));
        else WLAUNCH(launch_depthw_prefix(wn, t0, n, arr, d_ws.p, r.st));
        rep.tiles++;
        if (!window) {
            WLAUNCH(launch_depthw_interval_acc(d_iv.p + first[ref], n_iv, arr.P, t0, n, d_acc.p + first[ref], r.st));
            if (thr.k) WLAUNCH(launch_deptht_interval_acc(d_iv.p + first[ref], n_iv, tarr, thr.k, t0, n, d_accT.p + first[ref], sorted.size(), r.st));
            BHIP(hipEventRecord(rev.e[1], r.st));
            reduce_open = true;
            continue;
        }
        // the windows whose end lies in (origin, tile_end]: window kb is the first; the window's last end, hi, belongs to the last tile
        const uint64_t kb = origin / window;
        const uint64_t count = tile_end / window - kb + (tile_end == hi && hi % window ? 1 : 0);
        if (count > d_sum.cap || (thr.k && count > cnt_stride)) return ngsq_bam_fail(NGSQ_ERR_STATE, "a tile ends more windows than its sums array holds");
        if (count) WLAUNCH(launch_depthw_window_sums(arr.P, origin, n, window, kb, (uint32_t)count, hi, d_sum.p, d_ws.p, r.st));
        if (count && thr.k)
            WLAUNCH(launch_deptht_window_counts(tarr, thr.k, origin, n, window, kb, (uint32_t)count, hi, d_cnt.p, cnt_stride, d_ts.p, r.st));
        BHIP(hipEventRecord(rev.e[1], r.st));
        reduce_open = true;
        if (!count) continue;
        const DepthLineSource src{count, 0u, window, kb, wn.lo, hi, nullptr, d_sum.p};
        if (const int rc = format_pass(ref, src, more)) return rc;
    }
    if (!window && *more) {
        const DepthLineSource src{n_iv, 0u, 0u, 0, 0u, 0u, d_iv.p + first[ref], d_acc.p + first[ref]};
        if (const int rc = format_pass(ref, src, more)) return rc;
    }
    return NGSQ_OK;
}

// positions [lo, hi) of a sequence, or a region, no record was seen of: every line's sum is 0
int WindowsRun::no_record(uint32_t ref, uint32_t lo, uint32_t hi, bool *more) {
    if (lo >= hi || !*more) return NGSQ_OK;
    const DepthLineSource src = window ? DepthLineSource{n_windows(lo, hi), 1u, window, lo / window, lo, hi, nullptr, nullptr}
                                       : DepthLineSource{n_intervals(ref), 1u, 0u, 0, 0u, 0u, d_iv.p + first[ref], nullptr};
    if (!src.count) return NGSQ_OK;
    rep.sequences++;
    return format_pass(ref, src, more);
}

// Both entries: thr.k == 0 is ngsq_bam_depth_windows; covered (thr.k >= 1) receives the covered totals.
int windows_call(ngsq_bam *b, ngsq_ctx *c, int fd, uint32_t window, const ngsq_depth_interval *intervals, uint64_t n_intervals, const DepthThresholds &thr,
                 const char *query, const char *bai_path, uint32_t exclude_flags, uint32_t min_mapq, uint64_t batch_records, uint64_t coalesce_gap,
                 uint64_t tile_positions, uint64_t lines_per_pass, ngsq_depth_windows_report *out, uint64_t *covered) {
    if (!b || !c || fd < 0 || exclude_flags > 65535u || min_mapq > 255u || window > 2147483647u || (window && n_intervals) ||
        (!intervals && n_intervals) || n_intervals > 2147483647u)
        return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "null or invalid argument");
    if (out) memset(out, 0, sizeof *out);
    const double t_begin = now_ms();
    if (n_intervals && query) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "mean depth per BED interval cannot be combined with a query");
    const uint64_t n_refs = b->ref_lens.size();
    for (uint64_t i = 0; i < n_intervals; i++) {
        const ngsq_depth_interval &v = intervals[i];
        if (v.ref < 0 || (uint64_t)v.ref >= n_refs || v.start >= v.end || v.end > b->ref_lens[v.ref])
            return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "interval %llu is not one of the file's: sequence %d, start %u, end %u", (unsigned long long)i, v.ref,
                                 v.start, v.end);
    }
    if (const int rc = require_fresh_reader(b, "the depth is computed")) return rc;
    if (!ngsq_bam_sorted_by_coordinate(b)) return ngsq_bam_fail(NGSQ_ERR_UNSORTED, "the input BAM must be coordinate-sorted to compute depth");
    // ---- the query and the index, in front of the first byte and of any GPU work
    DepthRegion g;
    if (query && window)
        if (const int rc = depth_region(b, query, bai_path, &g)) return rc;
    if ((!window && !n_intervals) || (query && g.lo >= g.hi)) { // no interval (a query is not looked at), or an empty region: no line
        if (out) out->total_ms = now_ms() - t_begin;
        return NGSQ_OK;
    }
    WindowsRun p;
    DepthRun &r = p.r;
    p.window = window;
    p.thr = thr;
    r.exclude = exclude_flags;
    r.min_mapq = min_mapq;
    r.batch_records = batch_records ? batch_records : DEPTH_BATCH_RECORDS;
    r.tile = ngsq_depth_tile_positions(tile_positions);
    r.count_empty = true;
    r.seq_len = b->ref_lens;
    p.lines_per_pass = depth_round_up(std::min<uint64_t>(lines_per_pass ? lines_per_pass : r.tile, DEPTH_TILE_MAX), LINES_GRANULE);
    uint64_t longest = 0, most_lines = 0;
    if (!window) { // a stable counting sort by sequence; a sequence without an interval has no window
        p.first.assign(n_refs + 1, 0);
        for (uint64_t i = 0; i < n_intervals; i++) p.first[intervals[i].ref + 1]++;
        for (uint64_t ref = 0; ref < n_refs; ref++) {
            most_lines = std::max(most_lines, p.first[ref + 1]);
            if (!p.first[ref + 1]) r.seq_len[ref] = 0;
            p.first[ref + 1] += p.first[ref];
        }
        std::vector<uint64_t> at(p.first.begin(), p.first.end() - 1);
        p.sorted.resize(n_intervals);
        for (uint64_t i = 0; i < n_intervals; i++) p.sorted[at[intervals[i].ref]++] = intervals[i];
    }
    if (query) {
        longest = g.hi - g.lo;
        most_lines = p.n_windows(g.lo, g.hi);
    } else {
        for (const uint32_t l : r.seq_len) {
            longest = std::max<uint64_t>(longest, l);
            if (window) most_lines = std::max(most_lines, p.n_windows(0, l));
        }
    }
    BHIP(hipSetDevice(c->device));
    int rc = p.begin(b, c, fd, longest, most_lines);
    if (rc == NGSQ_OK)
        rc = query ? depth_walk_region(p, g.ref, g.start, g.end, g.lo, g.hi, g.chunks, coalesce_gap ? coalesce_gap : DEPTH_COALESCE_GAP) : depth_walk_file(p);
    rc = r.finish(rc);
    if (rc != NGSQ_OK) return rc;
    p.reduce_time();
    unsigned long long counted = 0;
    BHIP(hipMemcpy(&counted, &r.d_state.p->counted, sizeof counted, hipMemcpyDeviceToHost));
    if (out) {
        *out = p.rep;
        out->records_scanned = r.records_scanned;
        out->records_counted = counted;
        out->text_bytes = r.text_bytes;
        out->batches = r.batches;
        out->ranges = r.ranges;
        out->scan_ms = r.scan_ms;
        out->add_ms = r.add_ms;
        out->format_ms = r.format_ms;
        out->copy_ms = r.w.copy_ms;
        out->write_ms = r.w.write_ms;
        out->total_ms = now_ms() - t_begin;
    }
    for (uint32_t k = 0; k < thr.k; k++) covered[k] = p.covered[k];
    return NGSQ_OK;
}

} // namespace

extern "C" int ngsq_bam_depth_windows(ngsq_bam *b, ngsq_ctx *c, int fd, uint32_t window, const ngsq_depth_interval *intervals, uint64_t n_intervals,
                                      const char *query, const char *bai_path, uint32_t exclude_flags, uint32_t min_mapq, uint64_t batch_records,
                                      uint64_t coalesce_gap, uint64_t tile_positions, uint64_t lines_per_pass, ngsq_depth_windows_report *out) {
    return windows_call(b, c, fd, window, intervals, n_intervals, DepthThresholds{}, query, bai_path, exclude_flags, min_mapq, batch_records, coalesce_gap,
                        tile_positions, lines_per_pass, out, nullptr);
}

static_assert(offsetof(ngsq_depth_thresholds_report, covered) == sizeof(ngsq_depth_windows_report), "the windows report's fields in their order, then covered");

extern "C" int ngsq_bam_depth_thresholds(ngsq_bam *b, ngsq_ctx *c, int fd, uint32_t window, const ngsq_depth_interval *intervals, uint64_t n_intervals,
                                         const uint32_t *thresholds, uint32_t n_thresholds, const char *query, const char *bai_path,
                                         uint32_t exclude_flags, uint32_t min_mapq, uint64_t batch_records, uint64_t coalesce_gap, uint64_t tile_positions,
                                         uint64_t lines_per_pass, ngsq_depth_thresholds_report *out) {
    DepthThresholds thr{};
    bool ok = thresholds && n_thresholds >= 1 && n_thresholds <= NGSQ_DEPTH_MAX_THRESHOLDS;
    for (uint32_t k = 0; ok && k < n_thresholds; k++) {
        ok = thresholds[k] >= 1 && thresholds[k] <= 2147483647u && (!k || thresholds[k] > thresholds[k - 1]);
        thr.t[k] = thresholds[k];
    }
    if (!ok) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "null or invalid thresholds: 1 to 8 depths from 1 to 2147483647, strictly ascending");
    thr.k = n_thresholds;
    if (out) memset(out, 0, sizeof *out);
    ngsq_depth_windows_report w{};
    uint64_t covered[NGSQ_DEPTH_MAX_THRESHOLDS] = {};
    const int rc = windows_call(b, c, fd, window, intervals, n_intervals, thr, query, bai_path, exclude_flags, min_mapq, batch_records, coalesce_gap,
                                tile_positions, lines_per_pass, &w, covered);
    if (out) {
        memcpy(out, &w, sizeof w);
        memcpy(out->covered, covered, sizeof covered);
    }
    return rc;
}
