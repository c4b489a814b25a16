// samtext_kernels.h -- `ngs convert --gzip device <SAM> <BAM>` on the device: the lines of a chunk of SAM
// text become BAM records.  Launchers only; samtext_kernel.hip has the kernels, samtext.cpp the driver, the reader, the copies
// and the writer thread.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace ngsq {

// The reference names on the device: an open-addressing table of `slots` entries (a power of two,
// at least twice n_refs), each the reference id + 1 or 0 for an empty one; the name of sequence r is
// names[name_off[r] .. name_off[r + 1]).  A name's first slot is samtext_name_hash(name) & (slots - 1); the next one follows.
struct SamTextRefs {
    const uint32_t *table;
    const uint64_t *name_off;
    const uint8_t *names;
    uint32_t slots, n_refs;
};
uint32_t samtext_name_hash(const uint8_t *p, uint64_t n); // FNV-1a, the function the kernels use
// the kernels' float parser on the host: the bits of the f32 that p[0, n), n <= ST_FLOAT_TEXT_MAX, reads as; false: no float
bool samtext_parse_f32_host(const uint8_t *p, uint32_t n, uint32_t *bits);

// Why a line has no BAM record.  The codes follow the fields' order on the line: a line with two
// faults reports the one further left; the tags are walked in order and the walk ends at the first faulty one.
enum SamTextError : uint32_t {
    ST_OK = 0,
    ST_E_FIELDS,       // fewer than 11 fields
    ST_E_QNAME_EMPTY,  // an empty QNAME
    ST_E_QNAME_LONG,   // a QNAME longer than 254 bytes
    ST_E_FLAG,         // FLAG not decimal or above 65535
    ST_E_RNAME,        // RNAME not in the header
    ST_E_POS,          // POS not decimal or above 2^31 - 1
    ST_E_MAPQ,         // MAPQ not decimal or above 255
    ST_E_CIGAR_DIGITS, // a CIGAR operation without digits in front of it (digits without an operation behind them too)
    ST_E_CIGAR_OP,     // a CIGAR operation outside MIDNSHP=X
    ST_E_CIGAR_LEN,    // a CIGAR length of 2^28 or more
    ST_E_RNEXT,        // RNEXT not in the header
    ST_E_PNEXT,        // PNEXT not decimal or above 2^31 - 1
    ST_E_TLEN,         // TLEN not decimal or outside int32
    ST_E_SEQ,          // a SEQ letter outside =ACMGRSVTWYHKDBN (either case)
    ST_E_QUAL_NO_SEQ,  // QUAL present with SEQ *
    ST_E_QUAL_LEN,     // a QUAL length different from the SEQ length
    ST_E_QUAL_CHAR,    // a QUAL byte outside 33..126
    ST_E_TAG_FORM,     // a tag not of the form TG:T:V
    ST_E_TAG_TYPE,     // a tag type outside AifZHB
    ST_E_B_SUB,        // a B subtype outside cCsSiIf
    ST_E_NUMBER,       // a malformed number, or one outside its type's range
    ST_E_HEX,          // an H value with an odd number of digits or a byte that is no hex digit
    ST_E_FLOAT_LONG,   // a float text longer than 48 characters
    ST_E_TOO_LARGE,    // a record larger than 2^31 bytes
};
constexpr uint32_t ST_ERR_BITS = 8; // bad word: record index in the file << ST_ERR_BITS | SamTextError, ~0: none
constexpr uint32_t ST_FLOAT_TEXT_MAX = 48; // the formatter's longest output
constexpr uint32_t ST_TEXT_SLACK = 16;     // readable bytes the chunk's buffer has behind its last byte (eight-byte loads)

// The lines of a chunk that hold an f32 value: the full-occupancy kernels mark them and leave them to the kernels with the
// exact float parser, as section 13.4 does for the formatter.
struct SamTextFloats {
    uint8_t *mark;             // [n] 1: the line holds a float
    uint64_t *list;            // [n] the marked lines, in no order
    unsigned long long *count; // entries of list (zeroed by launch_samtext_size)
};

constexpr uint32_t ST_TILE = 4096; // bytes of text a workgroup counts and scatters
inline uint64_t samtext_tiles(uint64_t bytes) { return (bytes + ST_TILE - 1) / ST_TILE; }

// tile_cnt[t] = '\n' bytes of tile t of text[0, bytes), tile_cnt[tiles] = 0 (then scanned in place by the caller)
hipError_t launch_samtext_count(const uint8_t *text, uint64_t bytes, uint64_t *tile_cnt, hipStream_t s);
// host (pinned, device address) receives v[n]
hipError_t launch_samtext_word(const uint64_t *v, uint64_t n, unsigned long long *host, hipStream_t s);
// after the scan of tile_cnt: start[0] = 0 and start[k + 1] = the byte behind the k-th '\n', for k < cap (the lines beyond
// cap are dropped here).  Line k is text[start[k], start[k + 1] - 1).
hipError_t launch_samtext_scatter(const uint8_t *text, uint64_t bytes, const uint64_t *tile_off, uint64_t cap, uint64_t *start, hipStream_t s);
// Sizing pass: len[i] = bytes of line i's BAM record (block_size included), len[n] = 0; the smallest
// ((first_index + i) << 8 | code) of a line without a record goes to *bad (atomicMin).  One wave per line.
hipError_t launch_samtext_size(const uint8_t *text, const uint64_t *start, uint64_t n, uint64_t first_index, const SamTextRefs &refs, uint64_t *len,
                               unsigned long long *bad, const SamTextFloats &fl, hipStream_t s);
// after the exclusive scan of len: host receives [off[n], *bad]
hipError_t launch_samtext_total(const uint64_t *off, uint64_t n, const unsigned long long *bad, unsigned long long *host, hipStream_t s);
// Write pass: line i's record at out + off[i].
hipError_t launch_samtext_write(const uint8_t *text, const uint64_t *start, uint64_t n, const SamTextRefs &refs, const uint64_t *off, uint8_t *out,
                                const SamTextFloats &fl, hipStream_t s);

} // namespace ngsq
