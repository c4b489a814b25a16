// bai.cpp -- ngsq_bam_build_index (include/ngsq_index.h): the device ingest hands out the file's records batch by batch,
// bai_kernel.hip turns every batch into runs of (sequence, bin) and linear-index windows on the device, and the host
// writes the BAI from the run list and the windows -- it never walks the records.  DESIGN.md section 12.
#include <hip/hip_runtime_api.h>
#include <stdlib.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ngsq_index.h"
#include "bai_host.h"
#include "bai_kernels.h"
#include "bgzf.h"
#include "context.h"
#include "device_out.h"
#include "ingest_consumer.h"

using namespace ngsq;

namespace {

// The virtual position behind the header's last byte: the first record's chunk start (the header is read on the host at
// open; this walks the BGZF framing of its blocks only).  header_bytes = decompressed bytes in front of the first record.
int header_end_voffset(ngsq_bam *b, uint64_t header_bytes, uint64_t *out) {
    FILE *f = fopen(b->path.c_str(), "rb");
    if (!f) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "%s: cannot open", b->path.c_str());
    uint64_t coff = 0, total = 0;
    int rc = NGSQ_OK;
    std::vector<uint8_t> buf;
    for (;;) {
        uint8_t hd[18];
        if (fseeko(f, (off_t)coff, SEEK_SET) != 0 || fread(hd, 1, 18, f) != 18) {
            rc = ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "%s: the file ends inside the BAM header", b->path.c_str());
            break;
        }
        const uint32_t xlen = bgzf_rd16(hd + 10);
        buf.resize(12 + (size_t)xlen + 8);
        memcpy(buf.data(), hd, 18);
        if (fseeko(f, (off_t)coff, SEEK_SET) != 0 || fread(buf.data(), 1, 12 + (size_t)xlen, f) != 12 + (size_t)xlen) {
            rc = ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "%s: truncated BGZF block in the header", b->path.c_str());
            break;
        }
        // BSIZE from the extra field, then ISIZE from the block's trailer
        uint32_t bsize = 0;
        for (size_t q = 12; q + 4 <= 12 + (size_t)xlen;) {
            const uint32_t slen = bgzf_rd16(buf.data() + q + 2);
            if (buf[q] == 'B' && buf[q + 1] == 'C' && slen == 2) bsize = bgzf_rd16(buf.data() + q + 4) + 1;
            q += 4 + slen;
        }
        uint8_t tr[4];
        if (!bsize || fseeko(f, (off_t)(coff + bsize - 4), SEEK_SET) != 0 || fread(tr, 1, 4, f) != 4) {
            rc = ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "%s: corrupt BGZF block in the header", b->path.c_str());
            break;
        }
        const uint64_t isize = bgzf_rd32(tr);
        if (header_bytes > total && header_bytes <= total + isize) { // the header's last byte is in this block
            *out = header_bytes == total + isize ? (coff + bsize) << 16 : coff << 16 | (header_bytes - total);
            break;
        }
        total += isize;
        coff += bsize;
    }
    fclose(f);
    return rc;
}

void put32(std::vector<uint8_t> &v, uint32_t x) {
    for (int k = 0; k < 4; k++) v.push_back((uint8_t)(x >> (8 * k)));
}
void put64(std::vector<uint8_t> &v, uint64_t x) {
    for (int k = 0; k < 8; k++) v.push_back((uint8_t)(x >> (8 * k)));
}

constexpr uint64_t BATCH_RECORDS = (uint64_t)1 << 22;
constexpr uint32_t META_BIN = 37450;      // samtools' metadata pseudo-bin

} // namespace

std::string ngsq::bai_write_file(const char *bai_path, const BaiTables &T, const std::vector<BaiRun> &R, const std::vector<unsigned long long> &lin,
                                 uint64_t records, uint64_t final_end, BaiFileCounts *counts) {
    const uint32_t n_refs = T.n_refs;
    const uint64_t runs = R.size(), n_win = T.n_win;
    // ---- the file (SAM/BAM specification 5.2): per sequence its bins in ascending order, each with its runs in file order
    // (one chunk each: two runs of one bin are never adjacent), the pseudo-bin, the linear index; then n_no_coor
    std::vector<uint8_t> idx;
    idx.reserve(16 + runs * 20 + n_win * 8 + n_refs * 64);
    idx.insert(idx.end(), {'B', 'A', 'I', 1});
    put32(idx, n_refs);
    std::vector<uint32_t> cnt(META_BIN, 0), at(META_BIN, 0), touched, order;
    uint64_t k = 0, n_bins = 0;
    const unsigned long long *unmapped = T.unmapped(), *n_intv = T.n_intv();
    for (uint32_t r = 0; r < n_refs; r++) {
        while (k < runs && R[k].ref >= 0 && (uint32_t)R[k].ref < r) k++; // (sorted: nothing is skipped)
        const uint64_t a = k;
        while (k < runs && R[k].ref == (int32_t)r) k++;
        const uint64_t e = k;
        if (a == e) {
            put32(idx, 0);
        } else {
            touched.clear();
            for (uint64_t q = a; q < e; q++)
                if (cnt[R[q].bin]++ == 0) touched.push_back(R[q].bin);
            std::sort(touched.begin(), touched.end());
            uint32_t acc = 0;
            for (uint32_t bn : touched) {
                at[bn] = acc;
                acc += cnt[bn];
            }
            order.resize(acc);
            for (uint64_t q = a; q < e; q++) order[at[R[q].bin]++] = (uint32_t)(q - a);
            put32(idx, (uint32_t)touched.size() + 1);
            size_t o = 0;
            for (uint32_t bn : touched) {
                put32(idx, bn);
                put32(idx, cnt[bn]);
                for (uint32_t j = 0; j < cnt[bn]; j++, o++) {
                    const uint64_t q = a + order[o];
                    put64(idx, R[q].start);
                    put64(idx, q + 1 < runs ? R[q + 1].start : final_end);
                }
                cnt[bn] = 0;
            }
            n_bins += touched.size();
            const uint64_t placed = (e < runs ? R[e].rec : records) - R[a].rec;
            put32(idx, META_BIN);
            put32(idx, 2);
            put64(idx, R[a].start);
            put64(idx, e < runs ? R[e].start : final_end);
            put64(idx, placed - unmapped[r]);
            put64(idx, unmapped[r]);
        }
        const uint32_t ni = (uint32_t)n_intv[r];
        put32(idx, ni);
        for (uint32_t w = 0; w < ni; w++) put64(idx, lin[T.lin_base[r] + w]);
    }
    uint64_t n_no_coor = 0;
    if (runs && R[runs - 1].ref < 0) n_no_coor = records - R[runs - 1].rec;
    put64(idx, n_no_coor);
    // written beside its place and renamed: an error leaves nothing at bai_path
    std::string tmp = std::string(bai_path) + ".XXXXXX";
    const int fd = mkstemp(&tmp[0]);
    if (fd < 0) return "creating BAM index output file: cannot create " + tmp;
    size_t done = 0;
    while (done < idx.size()) {
        const ssize_t w = write(fd, idx.data() + done, idx.size() - done);
        if (w <= 0) break;
        done += (size_t)w;
    }
    const bool written = done == idx.size() && fchmod(fd, 0644) == 0;
    const bool ok = close(fd) == 0 && written;
    if (!ok || rename(tmp.c_str(), bai_path) != 0) {
        unlink(tmp.c_str());
        return std::string("writing BAM index: cannot write ") + bai_path;
    }
    counts->n_no_coor = n_no_coor;
    counts->bins = n_bins;
    return "";
}

extern "C" int ngsq_bam_build_index(ngsq_bam *b, ngsq_ctx *c, const char *bai_path, ngsq_index_report *out) {
    if (!b || !c || !bai_path) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    if (out) memset(out, 0, sizeof *out);
    if (const int rc = require_fresh_reader(b, "an index is built")) return rc;
    {
        const std::string m = bai_refuse_existing(bai_path);
        if (!m.empty()) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "%s", m.c_str());
    }
    if (!ngsq_bam_sorted_by_coordinate(b))
        return ngsq_bam_fail(NGSQ_ERR_UNSORTED, "the input BAM must be coordinate-sorted to be indexed");
    const double t0 = now_ms();
    uint64_t hdr_endv = 0;
    {
        const int rc = header_end_voffset(b, b->header_bytes, &hdr_endv);
        if (rc) return rc;
    }
    BHIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    // ---- device state: linear windows per sequence, unmapped counts, the carry; then the run list
    BaiTables T;
    BHIP(T.create(b->ref_lens.data(), (uint32_t)b->ref_lens.size(), hdr_endv, st));
    const uint64_t n_win = T.n_win;
    const BaiLinear &L = T.L;
    BaiState *const d_state = T.d_state;
    DevArray<uint64_t> d_flag;
    DevArray<BaiRun> d_tmp, d_runs;
    ScanScratch scan;
    const unsigned long long *const pin_h = T.pin_h;
    unsigned long long *const host_count = T.host_count, *const host_fin = T.host_fin;
    hipEvent_t ev = nullptr;
    BHIP(pool_event_get(&ev));
    struct EvPut {
        hipEvent_t e;
        ~EvPut() { pool_event_put(e); }
    } ev_put{ev};
    std::vector<BaiRun> R; // what the end copies to the host: the run list and the windows
    std::vector<unsigned long long> lin;
    // Every way out below waits for the stream first: a gather or a copy may still be queued on it when an error returns,
    // and the arrays above go back to the block cache or the heap when they leave scope (declared behind them: it runs first).
    StreamDrain drain{st};
    // ---- the scan: every batch of the device ingest, in file order
    uint64_t records = 0, runs = 0;
    uint32_t parity = 0;
    bool pending = false; // a gather has been queued whose count the host has not read yet
    for (;;) {
        ngsq_batch bt;
        BatchOrigin o;
        if (const int rc = next_batch_with_origin(b, c, BATCH_RECORDS, &bt, &o)) return rc;
        if (pending) { // (the ingest has waited for its own kernels, queued behind that gather: this returns at once)
            BHIP(hipEventSynchronize(ev));
            runs = pin_h[0];
            pending = false;
        }
        const uint64_t n = bt.n_records;
        if (!n) break;
        BHIP(d_flag.reserve(n + 1));
        BHIP(d_tmp.reserve(n));
        BHIP(d_runs.reserve_keep(runs + n, st));
        {
            KernelTimer kt(c, K_REC_INDEX, n * 16);
            BHIP(launch_bai_records(bt, o, d_state, parity, L, d_flag.p, d_tmp.p, st));
            BHIP(scan.exclusive_scan(d_flag.p, n + 1, st));
            BHIP(launch_bai_gather(d_flag.p, d_tmp.p, n, d_runs.p, runs, host_count, st));
        }
        BHIP(hipEventRecord(ev, st));
        pending = true;
        parity ^= 1u;
        records += n;
    }
    // ---- the end: linear gaps filled on the device, then the run list and the windows to the host
    BHIP(launch_bai_finish(L, d_state, parity, host_fin, st));
    R.resize(runs);
    lin.resize(n_win);
    if (runs) BHIP(hipMemcpyAsync(R.data(), d_runs.p, runs * sizeof(BaiRun), hipMemcpyDeviceToHost, st));
    if (n_win) BHIP(hipMemcpyAsync(lin.data(), T.d_lin.p, n_win * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    BHIP(hipStreamSynchronize(st));
    const unsigned long long *fin = T.fin();
    if (fin[0] != ~0ull)
        return ngsq_bam_fail(NGSQ_ERR_UNSORTED, "%s: record %llu (0-based) is out of coordinate order: the input BAM must be coordinate-sorted to be indexed",
                             b->path.c_str(), fin[0]);
    if (fin[1] != ~0ull)
        return ngsq_bam_fail(NGSQ_ERR_LIMIT, "%s: record %llu (0-based) %s", b->path.c_str(), fin[1], BAI_LIMIT_TEXT);
    const uint64_t final_end = fin[2];
    const double t1 = now_ms();
    BaiFileCounts counts;
    {
        const std::string m = bai_write_file(bai_path, T, R, lin, records, final_end, &counts);
        if (!m.empty()) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "%s", m.c_str());
    }
    if (out) {
        out->records = records;
        out->n_no_coor = counts.n_no_coor;
        out->runs = runs;
        out->bins = counts.bins;
        out->scan_ms = t1 - t0;
        out->write_ms = now_ms() - t1;
    }
    return NGSQ_OK;
}
