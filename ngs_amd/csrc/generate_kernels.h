// generate_kernels.h -- `ngs generate` on the device: the read pairs of a batch drawn, sized and written
// as FASTQ text.  Launchers only; generate_kernel.hip has the kernels, generate.cpp the driver and the two writers.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace ngsq {

// one provider on the device
struct GenProviderDev {
    uint64_t read_length, error_freq;
    int64_t inner_lower;   // the inner distance of table entry 0
    uint64_t elig_total;   // bases of its eligible sequences (len >= 2 L + 2)
    uint64_t weight_end;   // the weights up to and including this provider's
    uint32_t seq_first, n_seq; // its sequences in GenTables::seq; its cumulative eligible lengths are seq_cum[cum_first .. + n_seq]
    uint32_t cum_first;
    uint32_t tab_first, tab_n; // its inner-distance table in GenTables::inner (ngsq_generate_inner_table)
    uint32_t fname_off, fname_len; // its file name in GenTables::names
    uint32_t pad;
};
struct GenSeqDev {
    const uint8_t *bases; // one letter per base, case kept
    uint64_t len;
    uint32_t name_off, name_len;
};
struct GenTables {
    const GenProviderDev *prov;
    const GenSeqDev *seq;
    const uint64_t *seq_cum;
    const uint64_t *inner;
    const char *names;
    uint64_t total_weight;
    uint32_t n_prov;
};
// what k_gen_draw chose for a pair
struct GenPick {
    uint64_t start; // 1-based, as the name states it
    uint64_t flen;  // bases of the fragment
    uint32_t prov, seq; // seq: index in GenTables::seq
};

constexpr uint32_t GEN_ERR_BITS = 8; // bad word: pair index << GEN_ERR_BITS | code, ~0: none
enum GenError : uint32_t { GEN_OK = 0, GEN_E_ATTEMPTS };
// device words of a run: the bad word, then the attempts rejected by cause
enum GenWork : uint32_t { GW_BAD = 0, GW_REJ_START, GW_REJ_END, GW_REJ_BASE, GEN_WORK_WORDS };
// pinned words the host reads per batch: [text bytes of either file | the work words]
constexpr uint32_t GEN_HOST_WORDS = 1 + GEN_WORK_WORDS;

// One wave per pair: pick[i] and len[i] = bytes of either record of pair first + i (the two differ in one digit), len[n] = 0.
hipError_t launch_gen_draw(const GenTables &t, uint64_t seed, uint64_t first, uint64_t n, GenPick *pick, uint64_t *len, unsigned long long *work,
                           hipStream_t s);
// after the exclusive scan of len: host (pinned, device address) receives GEN_HOST_WORDS words
hipError_t launch_gen_total(const uint64_t *off, uint64_t n, const unsigned long long *work, unsigned long long *host, hipStream_t s);
// One wave per pair: its two records at one + off[i] and two + off[i].
hipError_t launch_gen_write(const GenTables &t, uint64_t seed, uint64_t first, uint64_t n, const GenPick *pick, const uint64_t *off, char *one, char *two,
                            hipStream_t s);

} // namespace ngsq
