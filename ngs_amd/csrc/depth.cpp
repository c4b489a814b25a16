// depth.cpp -- ngsq_bam_depth (include/ngsq_depth.h): the file is walked once through the device ingest, or
// a region's chunks by the range walks of `ngs view`; every batch is checked for order and its first and last sequence come to
// the host in pinned words; the records of the sequence at hand are added to its difference array; a sequence is final when a
// record of a later one, or the walk's end, has been seen, and is then taken through the run path tile by tile: run starts and
// depths, line sizes, their scan, the lines.  The text collects in the two device buffers of the output stage (device_out.h) and
// goes to the file while the next tiles are made.
#include "../../include/ngsq_depth.h"

#include "depth_kernels.h"
#include "depth_run.h"

using namespace ngsq;

namespace {

// The run path on top of the shared device side (depth_run.h): its arrays, and what the walks' two hooks do.
struct RunPath {
    DepthRun r;
    DevArray<int32_t> d_bsum, d_rdepth;
    DevArray<uint32_t> d_bcnt, d_rstart;
    DevArray<uint64_t> d_off;
    ScanScratch scan;
    DepthTileArrays arr{};
    ngsq_depth_report rep{};
    StreamDrain drain; // (behind every array the stream uses)

    DepthRun &run() { return r; }
    int begin(ngsq_bam *bam, ngsq_ctx *ctx, int fd, uint64_t longest);
    int window_final(bool *more);
    int no_record(uint32_t ref, uint32_t start, uint32_t end, bool *more);
};

// the shared side, then the run path's arrays for the largest tile there will be
int RunPath::begin(ngsq_bam *bam, ngsq_ctx *ctx, int fd, uint64_t longest) {
    drain.s = ctx->stream;
    const uint64_t t = std::min(r.tile, depth_round_up(std::max<uint64_t>(longest, 1), DEPTH_GRANULE));
    BHIP(d_bsum.reserve(t / DEPTH_GRANULE));
    BHIP(d_bcnt.reserve(t / DEPTH_GRANULE));
    BHIP(d_rstart.reserve(t + 1));
    BHIP(d_rdepth.reserve(t + 1));
    BHIP(d_off.reserve(t + 2));
    arr = DepthTileArrays{d_bsum.p, d_bcnt.p, d_rstart.p, d_rdepth.p, d_off.p};
    return r.begin(bam, ctx, fd, longest);
}

// The window at hand is final: tile by tile through the run path.
int RunPath::window_final(bool *more) {
    const DepthWindow wn = r.win;
    r.active = false;
    r.win = DepthWindow{-1, 0, 0, nullptr};
    if (!wn.len) return NGSQ_OK;
    const uint32_t final_end = wn.lo + wn.len, nl = r.name_len((uint32_t)wn.ref);
    const char *const name = r.name_of((uint32_t)wn.ref);
    rep.sequences++;
    for (uint64_t t0 = 0; t0 < wn.len && *more; t0 += r.tile) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(r.tile, wn.len - t0);
        const bool final = t0 + n == wn.len;
        BHIP(hipEventRecord(r.ev.e[2], r.st));
        BHIP(launch_depth_runs(wn, t0, n, arr, r.d_state.p, r.st));
        BHIP(hipEventRecord(r.ev.e[3], r.st));
        BHIP(hipEventRecord(r.ev.e[4], r.st));
        // lines + 1 entries at most: the run held back, the window's first position, two run starts per record
        const uint64_t entries = std::min<uint64_t>((uint64_t)n + 2, 2 * r.win_records + 3);
        BHIP(launch_depth_size(entries, final, final_end, nl, arr, r.d_state.p, r.st));
        BHIP(scan.exclusive_scan(arr.off, entries, r.st));
        BHIP(launch_depth_total(final, arr, r.d_state.p, r.host_dev(), r.st));
        BHIP(hipEventRecord(r.ev.e[5], r.st));
        BHIP(hipEventSynchronize(r.ev.e[5]));
        float ms = 0;
        if (hipEventElapsedTime(&ms, r.ev.e[2], r.ev.e[3]) == hipSuccess) rep.runs_ms += ms;
        if (hipEventElapsedTime(&ms, r.ev.e[4], r.ev.e[5]) == hipSuccess) r.format_ms += ms;
        r.add_times();
        const uint64_t bytes = r.host()[0], lines = r.host()[1];
        rep.tiles++;
        if (lines + 1 > entries) return ngsq_bam_fail(NGSQ_ERR_STATE, "the run path gave more lines than the window's records allow");
        if (!lines) continue;
        if (const int rc = r.room(bytes, more)) return rc;
        if (!*more) break;
        BHIP(hipEventRecord(r.ev.e[6], r.st));
        BHIP(launch_depth_write(r.d_text[r.slots.slot()].p + r.used, (uint32_t)lines, final, final_end, name, nl, arr, r.st));
        BHIP(hipEventRecord(r.ev.e[7], r.st));
        r.write_pending = true;
        r.used += bytes;
        rep.runs += lines;
        if (r.used >= DEPTH_TEXT_JOB)
            if (const int rc = r.submit()) return rc;
    }
    return NGSQ_OK;
}

// a sequence or region no record was seen of: one line, in closed form
int RunPath::no_record(uint32_t ref, uint32_t start, uint32_t end, bool *more) {
    if (start >= end || !*more) return NGSQ_OK;
    const uint64_t bytes = r.name_len(ref) + 4u + depth_digits(start) + depth_digits(end) + 1u;
    if (const int rc = r.room(bytes, more)) return rc;
    if (!*more) return NGSQ_OK;
    BHIP(launch_depth_zero_line(r.d_text[r.slots.slot()].p + r.used, r.name_of(ref), r.name_len(ref), start, end, r.st));
    r.used += bytes;
    rep.runs++;
    rep.sequences++;
    if (r.used >= DEPTH_TEXT_JOB) return r.submit();
    return NGSQ_OK;
}

} // namespace

extern "C" uint64_t ngsq_depth_tile_positions(uint64_t requested) {
    if (!requested) return DEPTH_TILE_DEFAULT;
    return depth_round_up(std::min(requested, DEPTH_TILE_MAX), DEPTH_GRANULE);
}

extern "C" int ngsq_bam_depth(ngsq_bam *b, ngsq_ctx *c, int fd, const char *query, const char *bai_path, uint32_t exclude_flags,
                              uint32_t min_mapq, uint64_t batch_records, uint64_t coalesce_gap, uint64_t tile_positions, ngsq_depth_report *out) {
    if (!b || !c || fd < 0 || exclude_flags > 65535u || min_mapq > 255u) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "null or invalid argument");
    if (out) memset(out, 0, sizeof *out);
    const double t_begin = now_ms();
    if (const int rc = require_fresh_reader(b, "the depth is computed")) return rc;
    if (!ngsq_bam_sorted_by_coordinate(b)) return ngsq_bam_fail(NGSQ_ERR_UNSORTED, "the input BAM must be coordinate-sorted to compute depth");
    // ---- the query and the index, in front of the first byte and of any GPU work
    DepthRegion g;
    if (query) {
        if (const int rc = depth_region(b, query, bai_path, &g)) return rc;
        if (g.lo >= g.hi) { // an empty interval: no line
            if (out) out->total_ms = now_ms() - t_begin;
            return NGSQ_OK;
        }
    }
    uint64_t longest = query ? g.hi - g.lo : 0;
    if (!query)
        for (const uint32_t l : b->ref_lens) longest = std::max<uint64_t>(longest, l);
    BHIP(hipSetDevice(c->device));
    RunPath p;
    DepthRun &r = p.r;
    r.exclude = exclude_flags;
    r.min_mapq = min_mapq;
    r.batch_records = batch_records ? batch_records : DEPTH_BATCH_RECORDS;
    r.tile = ngsq_depth_tile_positions(tile_positions);
    r.seq_len = b->ref_lens;
    int rc = p.begin(b, c, fd, longest);
    if (rc == NGSQ_OK)
        rc = query ? depth_walk_region(p, g.ref, g.start, g.end, g.lo, g.hi, g.chunks, coalesce_gap ? coalesce_gap : DEPTH_COALESCE_GAP) : depth_walk_file(p);
    rc = r.finish(rc);
    if (rc != NGSQ_OK) return rc;
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
    return NGSQ_OK;
}
