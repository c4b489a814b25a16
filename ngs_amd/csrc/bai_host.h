// bai_host.h -- the host side the two builders of a BAI share (DESIGN.md sections 12.2 and 21): bai.cpp (`ngs index`, positions
// from the ingest's blocks) and sort_resident.h (`ngs convert --sort coordinate --write-index`, positions from the encoder's).
// BaiTables is the device state of one build and the words the host reads of it; bai_write_file (bai.cpp) makes the file of
// the run list and the windows.  Neither walks a record.
#pragma once

#include <sys/stat.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "bai_kernels.h"
#include "mem_pool.h"

namespace ngsq {

constexpr uint32_t BAI_LIN_SLACK = 64;     // windows kept beyond @SQ LN: records may reach 1 Mbp past the sequence's end
constexpr uint32_t BAI_LIN_MAX = 1u << 15; // 2^29 / 16384: the windows of the BAI's coordinate range
constexpr const char *BAI_LIMIT_TEXT = "cannot be held by a BAI: its sequence id is out of range, or it reaches beyond position 2^29 or more than "
                                       "1 Mbp beyond its @SQ LN";

// "" or the refusal of a bai_path that exists, in the reference's words
inline std::string bai_refuse_existing(const char *bai_path) {
    struct stat sb;
    if (stat(bai_path, &sb) != 0) return "";
    return std::string("refusing to overwrite existing index file: ") + bai_path + ". Please delete and rerun if you'd like to replace it.";
}

struct BaiTables {
    uint32_t n_refs = 0;
    uint64_t n_win = 0;
    std::vector<uint64_t> lin_base; // [n_refs + 1]
    std::vector<uint32_t> lin_cap;  // [n_refs]
    std::vector<uint64_t> setup;    // [state | lin_base | lin_cap], kept while its copy may be queued
    DevArray<uint64_t> d_setup;
    DevArray<unsigned long long> d_lin, d_unm;
    BaiState *d_state = nullptr;
    BaiLinear L{};
    // results the host reads: [count of runs | state words | unmapped | n_intv] in mapped pinned memory
    MappedBuf pin;
    const unsigned long long *pin_h = nullptr;
    unsigned long long *host_count = nullptr, *host_fin = nullptr;

    // the windows of the sequences of ref_lens, empty; first_endv: the position behind the header, the first carry's endv
    hipError_t create(const uint32_t *ref_lens, uint32_t n, uint64_t first_endv, hipStream_t st) {
        n_refs = n;
        lin_base.assign((size_t)n_refs + 1, 0);
        lin_cap.assign(n_refs, 0);
        for (uint32_t r = 0; r < n_refs; r++) {
            lin_cap[r] = std::min<uint32_t>((uint32_t)(((uint64_t)ref_lens[r] + 16383) >> 14) + BAI_LIN_SLACK, BAI_LIN_MAX);
            lin_base[r + 1] = lin_base[r] + lin_cap[r];
        }
        n_win = lin_base[n_refs];
        // one upload of the setup words
        const size_t state_words = (sizeof(BaiState) + 7) / 8;
        setup.assign(state_words + n_refs + (n_refs + 1) / 2 + 1, 0);
        BaiState s0;
        memset(&s0, 0, sizeof s0);
        s0.carry[0].endv = first_endv;
        s0.bad_order = ~0ull;
        s0.bad_limit = ~0ull;
        memcpy(setup.data(), &s0, sizeof s0);
        memcpy(setup.data() + state_words, lin_base.data(), n_refs * sizeof(uint64_t));
        memcpy(setup.data() + state_words + n_refs, lin_cap.data(), n_refs * sizeof(uint32_t));
        hipError_t e = d_setup.reserve(setup.size());
        if (e == hipSuccess) e = d_lin.reserve(n_win + 1);
        if (e == hipSuccess) e = d_unm.reserve((size_t)n_refs + 1);
        if (e == hipSuccess) e = hipMemcpyAsync(d_setup.p, setup.data(), setup.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemsetAsync(d_lin.p, 0xFF, (n_win + 1) * sizeof(unsigned long long), st);
        if (e == hipSuccess) e = hipMemsetAsync(d_unm.p, 0, ((size_t)n_refs + 1) * sizeof(unsigned long long), st);
        if (e != hipSuccess) return e;
        d_state = reinterpret_cast<BaiState *>(d_setup.p);
        L.lin = d_lin.p;
        L.lin_base = d_setup.p + state_words;
        L.lin_cap = reinterpret_cast<const uint32_t *>(d_setup.p + state_words + n_refs);
        L.unmapped = d_unm.p;
        L.n_refs = n_refs;
        const size_t pin_words = 8 + BAI_HOST_STATE_WORDS + 2 * (size_t)n_refs;
        e = pin.reserve(pin_words * sizeof(unsigned long long));
        if (e != hipSuccess) return e;
        memset(pin.h, 0, pin_words * sizeof(unsigned long long));
        pin_h = static_cast<const unsigned long long *>(pin.h);
        host_count = static_cast<unsigned long long *>(pin.dev);
        host_fin = host_count + 8;
        return hipSuccess;
    }
    // what launch_bai_finish has left, once the stream has been waited for
    const unsigned long long *fin() const { return pin_h + 8; }
    const unsigned long long *unmapped() const { return fin() + BAI_HOST_STATE_WORDS; }
    const unsigned long long *n_intv() const { return unmapped() + n_refs; }
};

struct BaiFileCounts {
    uint64_t n_no_coor = 0, bins = 0;
};
// The BAI (SAM/BAM specification 5.2) of `records` records in the runs R (file order, positions virtual) and the windows lin
// (filled forward), final_end behind the last record: written beside bai_path and renamed, so that an error leaves nothing
// there.  "" or the message of the failure.
std::string bai_write_file(const char *bai_path, const BaiTables &T, const std::vector<BaiRun> &R, const std::vector<unsigned long long> &lin,
                           uint64_t records, uint64_t final_end, BaiFileCounts *counts);

} // namespace ngsq
