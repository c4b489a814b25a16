/*
 * ngsq_depth.h -- `ngs depth <BAM> [QUERY]`: the per-base depth of a coordinate-sorted BAM file, or of one region of it, as
 * bedGraph text.  The records are read by the device ingest (one walk of the file, or the range walks of a region through the
 * BAI, ngsq_view.h), turned into a difference array of the current sequence on the GPU, and each finished sequence is scanned,
 * run-length coded and formatted there, tile by tile.  The reference has no such command: every rule
 * below is this build's own decision, and tests/depth_model.py restates it.
 *
 * Which records count.  A record counts iff ref_id >= 0, pos >= 0, (flag & exclude_flags) == 0 and mapq >= min_mapq (a mapq of
 * 255, "missing", counts as the number it is).  Its span is the reference bases of its resolved CIGAR -- M, D, N, = and X; a
 * long CIGAR's operations come from CG:B,I, as both readers resolve it -- and must be at least 1: a record without a span
 * covers nothing (the one-base rule of `ngs view` and `ngs index` is about finding records, not about covering bases).  It covers
 * the 0-based positions [pos, min(pos + span, L)), L the sequence's length in the binary reference list: alignment start to
 * alignment end, deletions and skips included (the reference's Coverage rule).  A record that starts at or
 * beyond L covers nothing.
 *
 * What is written.  Lines "<name>\t<start>\t<end>\t<depth>\n": a 0-based half-open interval in decimal, <name> the bytes of
 * the binary reference list.  The lines are the maximal runs of equal depth, zero included, and tile the axis exactly.
 * Without a query every sequence of the header appears, in header order, tiled from 0 to L; a sequence without a counted
 * record is the one line "name\t0\tL\t0"; a sequence of length 0 gives no line; a file without records tiles every sequence
 * with zeros.  With a query ("name", "name:S", "name:S-E", the grammar of ngsq_bam_query_chunks) the one interval
 * [S-1, min(E, L)) of that sequence is tiled: the first run starts at S-1, the last ends at min(E, L); an empty interval gives
 * no line and is no error.  The records of a query are those of `ngs view`'s walks: the ones whose virtual offset lies in a
 * merged chunk of the index.  The bytes depend on the file, the query and the two filters alone: not on batch_records,
 * tile_positions, coalesce_gap or the grid.
 *
 * Order.  The header must say SO:coordinate (ngsq_bam_sorted_by_coordinate), else NGSQ_ERR_UNSORTED, "the input BAM must be
 * coordinate-sorted to compute depth", before any GPU work.  A record out of order met on the walk -- the key of `ngs index`:
 * (sequence, position), records without a sequence or a position last -- gives NGSQ_ERR_UNSORTED, "reading BAM record: record N
 * (0-based) is out of coordinate order: the input BAM must be coordinate-sorted to compute depth".  N is the record's index
 * in the file; with a query it counts within the range walk that met it (a walk numbers its records from its own beginning,
 * and its first record is compared with none).  What has been written by then is unspecified.
 *
 * Limits.  A depth is held in 32 bits: more than 2^31 - 1 counted records over one position are outside the contract.
 */
#ifndef NGSQ_DEPTH_H
#define NGSQ_DEPTH_H

#include "ngsq.h"
#include "ngsq_bam.h"
#include "ngsq_view.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the default of --exclude-flags: unmapped, secondary, QC-fail, duplicate (0x4 | 0x100 | 0x200 | 0x400), as `samtools depth` */
#define NGSQ_DEPTH_EXCLUDE_FLAGS 1796u

/* What one call did. */
typedef struct ngsq_depth_report {
    uint64_t records_scanned; /* records the device ingest handed out */
    uint64_t records_counted; /* records that count (the filters above) and, with a query, belong to the region's walks and
                                 meet [S-1, min(E, L)); a counted record may still cover nothing (no span, a start at or beyond L) */
    uint64_t runs;            /* lines written */
    uint64_t text_bytes;      /* bytes written */
    uint64_t sequences;       /* sequences (or the one region) with at least one line */
    uint64_t tiles;           /* tiles of tile_positions the run path took */
    uint64_t batches;         /* batches of the device ingest */
    uint64_t ranges;          /* range walks (0 without a query: one walk of the whole file) */
    double scan_ms;           /* host time inside the device ingest's calls */
    double add_ms;            /* GPU time of the order check and of the kernel that adds the records to the difference array */
    double runs_ms;           /* GPU time of the run kernels: sums, run starts, depths */
    double format_ms;         /* GPU time of the size pass, its scan and the write pass */
    double copy_ms;           /* GPU time of the device-to-host copies of the text */
    double write_ms;          /* the writer thread's time inside write(2) */
    double total_ms;          /* wall clock of the call */
} ngsq_depth_report;

/* The tile size in force for a request: 0 asks for the default; any request of at least 1 is accepted and rounded up to the
 * kernels' granule (a block's positions).  Pure; needs no GPU. */
uint64_t ngsq_depth_tile_positions(uint64_t requested);

/* Write the depth of `bam` (opened by ngsq_bam_open, no batch read yet) to the file descriptor fd, as described above.
 * query NULL: the whole file, no index needed.  Otherwise the region, through the index bai_path (NULL: "<path of bam>.bai");
 * the query and the index are looked at before the first byte is written, and their errors are those of ngsq_bam_query_chunks.
 * exclude_flags <= 65535, min_mapq <= 255.  batch_records: records per ingest batch (0: the default).  coalesce_gap: as in
 * ngsq_bam_view.  tile_positions: positions of a sequence the run path takes at a time (ngsq_depth_tile_positions).
 * Errors through ngsq_bam_last_error(): those above; "writing depth to stream: <strerror> (os error N)" for a failing write.
 * out (optional) receives the report. */
int ngsq_bam_depth(ngsq_bam *bam, ngsq_ctx *ctx, int fd, const char *query, const char *bai_path, uint32_t exclude_flags,
                   uint32_t min_mapq, uint64_t batch_records, uint64_t coalesce_gap, uint64_t tile_positions, ngsq_depth_report *out);

/* ---- `ngs depth --by <N|BED>`: the mean depth per window or per interval of a BED file ---- */

/* One interval: positions [start, end) of sequence ref (an index into the binary reference list), 0-based half-open,
 * start < end <= the sequence's length. */
typedef struct ngsq_depth_interval {
    int32_t ref;
    uint32_t start, end;
} ngsq_depth_interval;

/* Read the BED file `path` against the reference list of `bam` (opened by ngsq_bam_open): *intervals receives *n intervals in
 * the file's order (NULL when there is none), to be released with ngsq_depth_free_intervals.  Host code; needs no GPU.
 * Lines end in "\n", a trailing "\r" is dropped; empty lines and lines that begin with "#", "track" or "browser" are skipped.
 * Fields are separated by tabs: name, start, end; further fields are ignored.  start and end are decimal digits without a sign,
 * at most 2^31 - 1; end is clipped to the sequence's length L.  Intervals may overlap, nest, repeat and be unsorted.  A file
 * without an interval is accepted.
 * Errors (NGSQ_ERR_INVALID_ARGUMENT, ngsq_bam_last_error()): "opening BED file: <strerror> (os error N)", and, N the 1-based
 * line number, checked in this order, "reading BED file: line N: " followed by
 *   "expected at least 3 tab-separated fields, found K"
 *   "invalid start '<text>': expected a decimal number of at most 2147483647"   (likewise "invalid end")
 *   "start S is not below end E"
 *   "sequence '<name>' is not in the header"
 *   "start S lies at or beyond the end of '<name>' (L positions)"
 *   "more than 2147483647 intervals"
 * tests/depth_windows_model.py restates the reader. */
int ngsq_depth_read_bed(const ngsq_bam *bam, const char *path, ngsq_depth_interval **intervals, uint64_t *n);
void ngsq_depth_free_intervals(ngsq_depth_interval *intervals);

/* What one call of ngsq_bam_depth_windows did. */
typedef struct ngsq_depth_windows_report {
    uint64_t records_scanned; /* records the device ingest handed out */
    uint64_t records_counted; /* records that count, as in ngsq_depth_report; with intervals: of the whole file, whether or not
                                 their sequence has an interval */
    uint64_t lines;           /* lines written */
    uint64_t text_bytes;      /* bytes written */
    uint64_t sequences;       /* sequences (or the one region) with at least one line */
    uint64_t depth_sum;       /* sum of all interval sums, modulo 2^64 */
    uint64_t tiles;           /* tiles of tile_positions the reduce pass took */
    uint64_t passes;          /* format passes: each sizes, scans and writes at most lines_per_pass lines and waits once */
    uint64_t batches;         /* batches of the device ingest */
    uint64_t ranges;          /* range walks (0 without a query) */
    double scan_ms;           /* host time inside the device ingest's calls */
    double add_ms;            /* GPU time of the order check and of the kernels that add or count the records */
    double reduce_ms;         /* GPU time of the reduce pass: block sums, offsets, prefix sums, window or interval sums */
    double format_ms;         /* GPU time of the size pass, its scan and the write pass */
    double copy_ms;           /* GPU time of the device-to-host copies of the text */
    double write_ms;          /* the writer thread's time inside write(2) */
    double total_ms;          /* wall clock of the call */
} ngsq_depth_windows_report;

/* Write the mean depth of `bam` (opened by ngsq_bam_open, no batch read yet) per interval to fd, one line
 * "<name>\t<start>\t<end>\t<mean>\n" each.  The depth of a position, the records that count, query, bai_path, exclude_flags,
 * min_mapq, batch_records, coalesce_gap, tile_positions and the order rules are ngsq_bam_depth's.
 * window >= 1 (at most 2^31 - 1): the windows [kN, min((k + 1)N, L)) of every sequence in header order, all of them also where
 * no record counts ("0.00"); a sequence of length 0 gives no line.  With a query the windows stay aligned to position 0 and are
 * clipped to [S-1, min(E, L)); an empty region gives no line and is no error.
 * window == 0: the n_intervals intervals (NULL only with n_intervals == 0), each as ngsq_depth_read_bed gives it (ref in the
 * reference list, start < end <= L): sequences in header order, within one the order given; a sequence without an interval
 * gives no line, and its records are still counted.  Not with a query ("mean depth per BED interval cannot be combined with a
 * query").  No interval at all: nothing is written, no record is read, every count is 0, and a query is not looked at (the header must
 * still be sorted and the reader fresh).
 * The mean is the sum of the interval's depths over its length with exactly two decimals, rounded half up, in integers:
 * w = sum / len, r = sum % len, f = (100 r + len / 2) / len, and f == 100 carries into w.
 * lines_per_pass: lines the format pass takes at a time (0: the default; rounded up to a block's 256 lines).  The bytes do not
 * depend on it, nor on batch_records, tile_positions or coalesce_gap.
 * Errors as ngsq_bam_depth; bad arguments, window and intervals together and intervals outside the file's sequences are
 * NGSQ_ERR_INVALID_ARGUMENT before the header is looked at.  tests/depth_windows_model.py restates the bytes and the counts. */
int ngsq_bam_depth_windows(ngsq_bam *bam, ngsq_ctx *ctx, int fd, uint32_t window, const ngsq_depth_interval *intervals, uint64_t n_intervals,
                           const char *query, const char *bai_path, uint32_t exclude_flags, uint32_t min_mapq, uint64_t batch_records,
                           uint64_t coalesce_gap, uint64_t tile_positions, uint64_t lines_per_pass, ngsq_depth_windows_report *out);

/* ---- `ngs depth --by <N|BED> --thresholds <T[,T...]>`: positions at or above each depth, per interval ---- */

/* The most thresholds one call takes. */
#define NGSQ_DEPTH_MAX_THRESHOLDS 8

/* What one call of ngsq_bam_depth_thresholds did: the fields of ngsq_depth_windows_report in their order, then the covered totals. */
typedef struct ngsq_depth_thresholds_report {
    uint64_t records_scanned;
    uint64_t records_counted;
    uint64_t lines;
    uint64_t text_bytes;
    uint64_t sequences;
    uint64_t depth_sum;
    uint64_t tiles;
    uint64_t passes;
    uint64_t batches;
    uint64_t ranges;
    double scan_ms;
    double add_ms;
    double reduce_ms;         /* with the count kernels: block counts, their offsets, window or interval counts */
    double format_ms;
    double copy_ms;
    double write_ms;
    double total_ms;
    uint64_t covered[NGSQ_DEPTH_MAX_THRESHOLDS]; /* covered[k]: the sum of n_k over all lines written (below 2^62: a count is below
                                                    2^31 and a source has fewer than 2^31 lines); entries from n_thresholds upward are 0 */
} ngsq_depth_thresholds_report;

/* ngsq_bam_depth_windows with K = n_thresholds more columns a line: "<name>\t<start>\t<end>\t<mean>\t<n_1>\t...\t<n_K>\n".  The
 * first four columns are ngsq_bam_depth_windows' of the same call: the same intervals, the same order, the same mean.  n_k is
 * the number of positions of the interval whose depth is at least thresholds[k], in decimal; the depth of a position is
 * ngsq_bam_depth's, unchanged (the same filters, the same span, the same clip at L).  A sequence, region or interval without a
 * counted record gives "0.00" and K zeros.  There is no header line.  Every rule of ngsq_bam_depth_windows about windows,
 * regions and intervals holds word for word: windows aligned to position 0 and clipped to the region, intervals not with a
 * query, the empty interval list and the empty region answered with zero counts.  The bytes follow from the file, the filters,
 * the query, the window or the intervals and the thresholds alone: not from batch_records, tile_positions, lines_per_pass,
 * coalesce_gap or the grid.
 * thresholds: n_thresholds (1 to NGSQ_DEPTH_MAX_THRESHOLDS) depths, each from 1 to 2^31 - 1, strictly ascending.  A null list,
 * a count of 0 or above 8, an element of 0 or above 2^31 - 1 and a list that is not strictly ascending are
 * NGSQ_ERR_INVALID_ARGUMENT before the header is looked at, as is everything ngsq_bam_depth_windows refuses there; all other
 * errors are ngsq_bam_depth_windows'.  ngsq_bam_depth_windows itself, its bytes and the kernels it launches do not change.
 * tests/depth_thresholds_model.py restates the bytes and the counts. */
int ngsq_bam_depth_thresholds(ngsq_bam *bam, ngsq_ctx *ctx, int fd, uint32_t window, const ngsq_depth_interval *intervals, uint64_t n_intervals,
                              const uint32_t *thresholds, uint32_t n_thresholds, const char *query, const char *bai_path, uint32_t exclude_flags,
                              uint32_t min_mapq, uint64_t batch_records, uint64_t coalesce_gap, uint64_t tile_positions, uint64_t lines_per_pass,
                              ngsq_depth_thresholds_report *out);

#ifdef __cplusplus
}
#endif
#endif
