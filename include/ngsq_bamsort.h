/*
 * ngsq_bamsort.h -- `ngs convert --gzip device --sort coordinate <BAM> <BAM>`: a BAM in any record order
 * becomes a coordinate-sorted BAM that `ngs index` accepts.  The device ingest (ngsq_bam.h) inflates the file and finds its
 * records on the GPU, the records stay in device memory until their order is known, and the device DEFLATE encoder (ngsq_bgzf.h)
 * writes the BGZF.  The counterpart of ngsq_sam_write_sorted_bam (ngsq_samtext.h) for the file an aligner pipeline keeps.
 *
 * Messages: ngsq_bam_last_error().
 */
#ifndef NGSQ_BAMSORT_H
#define NGSQ_BAMSORT_H

#include "ngsq.h"
#include "ngsq_bam.h"
#include "ngsq_index.h"
#include "ngsq_sort.h" /* ngsq_sort_survey_bytes_per_record, ngsq_sort_resident_bytes_per_record */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ngsq_bamsort_report {
    uint64_t records;          /* records written */
    uint64_t header_bytes;     /* the header text as written (ngsq_sam_sorted_header of the input's) */
    uint64_t bam_bytes;        /* the decompressed stream: header, reference list and records */
    uint64_t compressed_bytes; /* the file: every block and the EOF block */
    uint64_t batches;          /* batches of the device ingest */
    uint64_t slabs;            /* blocks of device memory that hold the records */
    uint64_t pieces;           /* pieces of the sorted stream that were gathered and compressed */
    uint64_t blocks, stored_blocks; /* BGZF blocks (without the EOF block), and those of them with a stored payload */
    uint64_t resident_bytes;   /* what the budget was held against: the record bytes and 48 bytes per record */
    uint32_t passes_run, passes_skipped; /* of the sort's eight digits */
    double scan_ms, keep_ms, sort_ms, gather_ms, deflate_ms, d2h_ms, write_ms; /* ingest (wall clock of its calls), copies into the slabs, keys to sorted offsets, gather, encoder, copies down, file writes */
    double total_ms;           /* wall clock */
} ngsq_bamsort_report;

/* The records of `bam`, a reader no record has been read from, in coordinate order, written as a BAM to the descriptor fd.
 * Key, ties and unplaced records are ngsq_sam_write_sorted_bam's: key = (refID < 0 || pos < 0 ? 0xFFFFFFFF : refID) << 32 |
 * (pos + 1), ascending, equal keys in input order.  A record is the input's bytes, block_size included, moved whole.  The header
 * text is ngsq_sam_sorted_header of the input's (trailing NULs dropped, as the reader drops them); n_ref and the reference
 * entries are the input's bytes.  ctx: a context on the device that sorts.  max_records: the first max_records records of the
 * input are sorted (0: all).  batch_records: records per ingest batch (0: 4 Mi).  piece_bytes: sorted record bytes gathered and
 * compressed at a time (0: 64 MiB).  max_resident_bytes: what the record bytes and 48 bytes per record may take of device memory
 * (0: what hipMemGetInfo reports free once the ingest has its buffers, less 4 GiB); beyond it the call fails with NGSQ_ERR_LIMIT.
 * At most 2^32 - 1 records.  What the ingest refuses (a truncated file, a bad block, a malformed record) is reported with its
 * message behind "reading BAM record: ", and every such fault before anything is written to fd.  The decompressed stream
 * depends on the input and max_records alone; the compressed bytes also on piece_bytes. */
int ngsq_bam_write_sorted_bam(ngsq_bam *bam, ngsq_ctx *ctx, int fd, uint64_t max_records, uint64_t batch_records, uint64_t piece_bytes,
                              uint64_t max_resident_bytes, ngsq_bamsort_report *out);

/* ngsq_bam_write_sorted_bam, and the BAI of what it writes at bai_path (`ngs convert --write-index`): byte
 * for byte the file ngsq_bam_build_index writes for the finished BAM, built from the records while they are resident and from the
 * encoder's block offsets, without reading the output back.  The bytes written to fd are those of the unindexed call.
 * index_tile_records: sorted records per launch of the index pass (0: 4 Mi).  index_out (optional): records, n_no_coor, runs and
 * bins as ngsq_bam_build_index reports them, scan_ms = the device time the index added (index pass, block table, translation),
 * write_ms = the BAI file.  Refused before any GPU work: an existing bai_path (NGSQ_ERR_INVALID_ARGUMENT, "refusing to overwrite
 * existing index file: ...").  A record the BAI cannot hold (position beyond 2^29, or reaching more than 1 Mbp beyond the
 * reference length of the input's binary header): NGSQ_ERR_LIMIT before anything is written to fd, "reading BAM record: record N
 * (0-based) of the sorted output cannot be held by a BAI: ...".  The index is written beside bai_path and renamed once the EOF
 * block is out; a failing call leaves nothing there. */
int ngsq_bam_write_sorted_bam_indexed(ngsq_bam *bam, ngsq_ctx *ctx, int fd, uint64_t max_records, uint64_t batch_records, uint64_t piece_bytes,
                                      uint64_t max_resident_bytes, ngsq_bamsort_report *out, const char *bai_path, uint64_t index_tile_records,
                                      ngsq_index_report *index_out);

/* How ngsq_bam_write_sorted_bam_rounds went about a file. */
typedef struct ngsq_bamsort_rounds {
    uint64_t rounds;         /* ranges of the sorted order that were resident in turn (1: the records fitted the budget) */
    uint64_t walks;          /* walks of the input begun: 1, or the attempt that overflowed, the survey and one per round */
    uint64_t survey_records; /* records the survey walk saw (0: no survey) */
    uint64_t survey_bytes;   /* what the survey's arrays were counted as: ngsq_sort_survey_bytes_per_record() per record */
    uint64_t budget;         /* the budget in force: max_resident_bytes, or the default */
    double survey_ms;        /* wall clock of the survey: its walk, its sort and the plan */
} ngsq_bamsort_rounds;

/* ngsq_bam_write_sorted_bam (bai_path null) or ngsq_bam_write_sorted_bam_indexed without the limit of max_resident_bytes: `ngs
 * convert --gzip device --sort coordinate [--sort-memory <SIZE>] <BAM> <BAM>`.  Records that fit the budget:
 * exactly the call above, one walk of the input, rounds = 1.  Records that do not: the attempt is dropped and the input walked
 * again from its beginning -- a survey walk that keeps a key and a length per record (ngsq_sort_survey_bytes_per_record() bytes
 * each, counted against the budget), sorts them and cuts the sorted order greedily into consecutive ranges of records whose bytes
 * and ngsq_sort_resident_bytes_per_record() bytes each fit the budget; then one walk per range ("round") that keeps that range's
 * records, sorts them and continues the file's stream of pieces.  The bytes written to fd, and to bai_path, are those of the calls
 * above at a budget that fits, for the same input, max_records and piece_bytes.  NGSQ_ERR_LIMIT, before anything is written to
 * fd: "reading BAM record: --sort coordinate in rounds holds a key per record in device memory: N bytes needed, M allowed" (the
 * survey alone does not fit), "reading BAM record: record N (0-based) of the sorted output alone takes B bytes of device memory,
 * M allowed" (one record does not), and with bai_path a record the BAI cannot hold, in the words and with the number of the call
 * above.  NGSQ_ERR_STATE, "the input changed between walks: ...", when a round finds other records than the survey planned: the
 * file was rewritten underneath the call, and what has been written to fd by then is no BAM.  `out` as above, with batches =
 * the survey walk's, slabs and resident_bytes = the largest round's, passes_run and passes_skipped = the survey sort's, and
 * the times summed over the walks and rounds.  rounds_out (optional) as above. */
int ngsq_bam_write_sorted_bam_rounds(ngsq_bam *bam, ngsq_ctx *ctx, int fd, uint64_t max_records, uint64_t batch_records, uint64_t piece_bytes,
                                     uint64_t max_resident_bytes, ngsq_bamsort_report *out, const char *bai_path, uint64_t index_tile_records,
                                     ngsq_index_report *index_out, ngsq_bamsort_rounds *rounds_out);
/* The device time the last indexed call on this thread (this one or ngsq_sam_write_sorted_bam_indexed) spent on its index, in
 * ms: the index pass, the appends to the block table, the translation to virtual positions.  Null pointers are skipped. */
void ngsq_sort_index_split(double *pass_ms, double *blocks_ms, double *translate_ms);

#ifdef __cplusplus
}
#endif
#endif
