// sort_resident.h -- what the two drivers of `ngs convert --sort coordinate` share (DESIGN.md sections 19.2 and 20.2): samsort.cpp
// (SAM text in) and bamsort.cpp (BAM in).  A driver's phase 1 leaves the records in slabs of device memory and their addresses,
// lengths and keys in the three per-record arrays; phases 2 and 3 are here: sort_pairs_u64 orders (key, record index) pairs, the
// sorted stream is cut into pieces of piece_bytes, per piece k_sort_gather copies the records to their sorted offsets, the
// device DEFLATE encoder makes BGZF blocks of them and the output stage of device_out.h writes them, behind the header's blocks
// and in front of the EOF block.  A failure leaves its code and its message in `err`; the driver reports it through its own channel.
#pragma once

#include <cstdarg>
#include <memory>
#include <string>
#include <vector>

#include "device_out.h"
#include "samtext_kernels.h" // launch_samtext_word
#include "sort_kernels.h"

namespace ngsq {

constexpr uint64_t SORT_PIECE_DEFAULT = (uint64_t)64 << 20, SORT_PIECE_MAX = (uint64_t)1 << 30;
// Device bytes per resident record beside its own: address 8, length 4, key 8, the sort's second key array and its two index
// arrays 16, the sorted offset 8, and its share of the pass table (half a byte).
constexpr uint64_t SORT_BYTES_PER_RECORD = 48;
// What the default budget leaves free of the memory hipMemGetInfo reports: the two text buffers, a chunk's line and offset
// arrays, the piece buffer, the encoder's scratch and its two block buffers, the unused end of the last slab, and the old
// halves of the per-record arrays while they double.
constexpr uint64_t SORT_DEVICE_RESERVE = (uint64_t)4 << 30;
constexpr uint64_t SORT_SLAB_MIN = (uint64_t)1 << 20, SORT_SLAB_MAX = (uint64_t)512 << 20;

struct SortResident {
    enum Ev { EV_S0 = 0, EV_S1, EV_G0, EV_G1, EV_Z1, EV_N };
    enum HostWord : uint32_t { HW_TOTAL = 0, HW_DEFLATE, HW_WORDS = HW_DEFLATE + DEFLATE_HOST_WORDS };

    hipStream_t st = nullptr;
    // phase 1 fills these: record i of the input lies at d_addr[i], d_len[i] bytes, with the key d_key[i]
    DevArray<uint64_t> d_addr, d_key;
    DevArray<uint32_t> d_len;
    std::vector<std::unique_ptr<DevArray<uint8_t>>> slabs; // the records: a slab is filled from its front and never moved
    uint64_t slab_used = 0;
    uint64_t records = 0, rec_bytes = 0;
    // phases 2 and 3
    DevArray<uint64_t> d_soff;
    DevArray<uint8_t> d_piece;
    ScanScratch scan;
    SortScratch sort;
    BgzfEncoder enc; // d_piece's bytes become the blocks of a job
    JobSlots zslots;
    MappedBuf hw, hw_first;
    HipEvents<EV_N> ev;
    DeviceWriter w;
    uint64_t bam_bytes = 0, pieces = 0;
    double sort_ms = 0, gather_ms = 0, deflate_ms = 0;
    int code = 0;
    std::string err;
    StreamDrain drain; // (behind the arrays: it runs first)

    int fail(int code_, const char *fmt, ...) {
        char buf[1024];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code = code_;
    }
#define SRHIP(expr)                                                                                  \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) return fail(NGSQ_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

    // the stream the drivers' kernels run on, the events, the words the host reads
    int begin(hipStream_t stream) {
        st = drain.s = stream;
        SRHIP(hw.reserve(HW_WORDS * sizeof(unsigned long long)));
        memset(hw.h, 0, HW_WORDS * sizeof(unsigned long long));
        enc.h = static_cast<const unsigned long long *>(hw.h) + HW_DEFLATE;
        enc.hdev = static_cast<unsigned long long *>(hw.dev) + HW_DEFLATE;
        for (auto &e : ev.e) SRHIP(hipEventCreate(&e));
        return NGSQ_OK;
    }
    void elapsed(int a, int b, double *sum) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.e[a], ev.e[b]) == hipSuccess) *sum += ms;
    }
    int copy_failed(hipError_t e) { return fail(NGSQ_ERR_DEVICE, "copying the BGZF blocks to the host: %s", hipGetErrorString(e)); }
    int write_failed(int e) { return fail(NGSQ_ERR_INVALID_ARGUMENT, "writing BAM record: %s (os error %d)", strerror(e), e); }

    // Room for `bytes` more record bytes whose first lies at an address of residue `residue` modulo 16 (residue > 15: anywhere):
    // behind the newest slab's records, or at the front of a new slab of slab_bytes (or of what these records need).
    int place(uint64_t bytes, uint64_t slab_bytes, uint32_t residue, uint8_t **dst) {
        auto pad_at = [&](const uint8_t *p) { return residue > 15u ? 0u : (residue - (uint32_t)((uintptr_t)p & 15u)) & 15u; };
        uint32_t pad = slabs.empty() ? 0 : pad_at(slabs.back()->p + slab_used);
        if (slabs.empty() || slab_used + pad + bytes + SORT_GATHER_SLACK > slabs.back()->cap) {
            slabs.emplace_back(new DevArray<uint8_t>());
            SRHIP(slabs.back()->reserve(std::max(slab_bytes, bytes) + (residue > 15u ? 0u : 15u) + SORT_GATHER_SLACK));
            slab_used = 0;
            pad = pad_at(slabs.back()->p);
        }
        *dst = slabs.back()->p + slab_used + pad;
        slab_used += pad + bytes;
        return NGSQ_OK;
    }
    // the three per-record arrays with room for n records, their contents kept
    int reserve_records(uint64_t n) {
        SRHIP(d_addr.reserve_keep(n, st));
        SRHIP(d_len.reserve_keep(n, st));
        SRHIP(d_key.reserve_keep(n, st));
        return NGSQ_OK;
    }

    // bytes of d_piece through the encoder into its buffer of the job's slot, the blocks to the writer (as samtext.cpp's jobs)
    int compress_and_push(uint64_t bytes) {
        SRHIP(enc.launch(zslots.slot(), d_piece.p, bytes, st));
        SRHIP(hipEventRecord(ev.e[EV_Z1], st));
        SRHIP(hipEventSynchronize(ev.e[EV_Z1]));
        const char *blocks = nullptr;
        uint64_t n = 0;
        if (const char *m = enc.collect(zslots.slot(), bytes, &blocks, &n)) return fail(NGSQ_ERR_STATE, "%s", m);
        elapsed(EV_G1, EV_Z1, &deflate_ms);
        SRHIP(zslots.submit(w, blocks, n, st));
        bam_bytes += bytes;
        return NGSQ_OK;
    }

    // phases 2 and 3: the order, then the header stream hs, then the pieces, to fd
    int sort_and_write(int fd, int device, const std::string &hs, uint64_t piece_bytes) {
        unsigned long long *const hdev = static_cast<unsigned long long *>(hw.dev);
        const unsigned long long *const h = static_cast<const unsigned long long *>(hw.h);
        const uint32_t *perm = nullptr;
        uint64_t total = 0;
        const unsigned long long *first = nullptr;
        if (records) {
            SRHIP(hipEventRecord(ev.e[EV_S0], st));
            SRHIP(sort_pairs_u64(d_key.p, records, sort, st, &perm));
            // the sorted offsets, and the record every piece begins in
            SRHIP(d_soff.reserve(records + 1));
            SRHIP(launch_sort_lengths(d_len.p, perm, records, d_soff.p, st));
            SRHIP(scan.exclusive_scan(d_soff.p, records + 1, st));
            SRHIP(launch_samtext_word(d_soff.p, records, hdev + HW_TOTAL, st));
            SRHIP(hipEventRecord(ev.e[EV_S1], st));
            SRHIP(hipStreamSynchronize(st));
            elapsed(EV_S0, EV_S1, &sort_ms);
            total = h[HW_TOTAL];
            if (total != rec_bytes)
                return fail(NGSQ_ERR_STATE, "the sorted records take %llu bytes, the parsed ones %llu", (unsigned long long)total, (unsigned long long)rec_bytes);
            pieces = (total + piece_bytes - 1) / piece_bytes;
            if (pieces >= 0x7FFFFFFFull) return fail(NGSQ_ERR_LIMIT, "writing BAM record: more than 2^31 - 2 pieces of %llu bytes", (unsigned long long)piece_bytes);
            SRHIP(hw_first.reserve((pieces + 1) * sizeof(unsigned long long)));
            SRHIP(launch_sort_bisect(d_soff.p, records, piece_bytes, pieces, static_cast<unsigned long long *>(hw_first.dev), st));
            SRHIP(hipStreamSynchronize(st));
            first = static_cast<const unsigned long long *>(hw_first.h);
        }
        SRHIP(zslots.create());
        SRHIP(w.start(fd, device));
        // the header's blocks, in front of the first record (as samtools writes them)
        SRHIP(d_piece.reserve(std::max<uint64_t>(hs.size(), std::min(piece_bytes, total)) + DEFLATE_IN_SLACK));
        SRHIP(hipMemcpyAsync(d_piece.p, hs.data(), hs.size(), hipMemcpyHostToDevice, st));
        SRHIP(hipEventRecord(ev.e[EV_G1], st));
        if (const int rc = compress_and_push(hs.size())) return rc;
        for (uint64_t j = 0; j < pieces && !w.failed(); j++) {
            const uint64_t lo = j * piece_bytes, hi = std::min(lo + piece_bytes, total);
            // records first[j] .. first[j + 1]: the last of them may begin in this piece and end in the next
            const uint64_t a = first[j], b = std::min<uint64_t>(first[j + 1] + 1, records);
            if (!zslots.acquire(&w)) return copy_failed(w.herr);
            SRHIP(hipEventRecord(ev.e[EV_G0], st));
            SRHIP(launch_sort_gather(d_addr.p, perm, d_soff.p, a, b, lo, hi, d_piece.p, st));
            SRHIP(hipEventRecord(ev.e[EV_G1], st));
            if (const int rc = compress_and_push(hi - lo)) return rc;
            elapsed(EV_G0, EV_G1, &gather_ms);
        }
        SRHIP(hipStreamSynchronize(st));
        return NGSQ_OK;
    }
#undef SRHIP

    // The end of a call whose phases gave rc (a driver's own failure: this object's `err` is not set and stays so): the writer
    // ended, its errors reported when nothing failed before them, the EOF block.
    int finish(int rc, int fd) {
        const WriterEnd end = w.end();
        if (rc == NGSQ_OK && end.herr != hipSuccess) rc = copy_failed(end.herr);
        if (rc == NGSQ_OK && end.werr) rc = write_failed(end.werr);
        if (rc == NGSQ_OK) {
            if (const int e = write_bgzf_eof(fd)) rc = write_failed(e);
            enc.comp_bytes += sizeof BGZF_EOF_BLOCK;
        }
        return rc;
    }
    uint64_t resident_bytes() const { return rec_bytes + records * SORT_BYTES_PER_RECORD; }
};

} // namespace ngsq
