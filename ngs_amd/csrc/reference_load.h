// reference_load.h -- the FASTA of `ngs generate` (generate.cpp): every record of a file opened by
// ngsq_fasta_open as the letters themselves on the device, one byte per base, case kept.  reference.cpp has both functions:
// they share the index, the pinned upload ring and the tiled conversion of the Edits reference (ngsq_reference_load).
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/ngsq_reference.h"
#include "kernels.h"

namespace ngsq {

// bases of every record, in file order, counted on the host through the file's mapping (a memchr per line; the file's
// reader threads share the records): what the conversion kernels will find, known before a device exists
int fasta_record_bases(ngsq_fasta *f, std::vector<uint64_t> *bases, std::string *err);

// the letters of a file on the device: record i's bases are d[off[i] .. off[i] + len[i])
struct FastaLetters {
    uint8_t *d = nullptr;
    size_t got = 0; // of the block behind d (pool_device_alloc)
    std::vector<uint64_t> off, len;
    uint64_t text_bytes = 0;
    double read_s = 0, device_s = 0;
    FastaLetters() = default;
    FastaLetters(const FastaLetters &) = delete;
    FastaLetters &operator=(const FastaLetters &) = delete;
    ~FastaLetters();
};

// Upload the text of every record (file -> pinned slots -> device) and convert it on `device`.  Returns an NGSQ_* code
// and the message in *err.
int fasta_load_letters(ngsq_fasta *f, int device, const LaunchInfo &li, FastaLetters *out, std::string *err);

} // namespace ngsq
