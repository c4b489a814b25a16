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

/* The device time the last indexed call on this thread (this one or ngsq_sam_write_sorted_bam_indexed) spent on its index, in
 * ms: the index pass, the appends to the block table, the translation to virtual positions.  Null pointers are skipped. */
void ngsq_sort_index_split(double *pass_ms, double *blocks_ms, double *translate_ms);

#ifdef __cplusplus
}
#endif
#endif
