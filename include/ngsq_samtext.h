/*
 * ngsq_samtext.h -- `ngs convert --gzip device <SAM> <BAM>`: SAM text parsed on the GPU, the BAM records
 * compressed there by the device DEFLATE encoder (ngsq_bgzf.h), so that text goes up over PCIe and only BGZF comes back.
 * The counterpart of ngsq_bam_write_sam (ngsq_sam.h).
 *
 * Messages: ngsq_last_error(ctx); ngsq_sam_check_header writes its own.
 */
#ifndef NGSQ_SAMTEXT_H
#define NGSQ_SAMTEXT_H

#include "ngsq.h"
#include "ngsq_index.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ngsq_samtext_report {
    uint64_t records;          /* records written */
    uint64_t header_bytes;     /* the header text (the leading lines that start with '@') */
    uint64_t text_bytes;       /* the lines of the records written, their newlines included */
    uint64_t bam_bytes;        /* the decompressed stream: header, reference list and records */
    uint64_t compressed_bytes; /* the file: every block and the EOF block */
    uint64_t chunks;           /* chunks of text that went to the device */
    uint64_t blocks, stored_blocks; /* BGZF blocks (without the EOF block), and those of them with a stored payload */
    double read_ms, h2d_ms, parse_ms, deflate_ms, d2h_ms, write_ms; /* file reads, copies up, line starts and both passes, encoder, copies down, file writes */
    double total_ms;           /* wall clock */
} ngsq_samtext_report;

/* Host only, no GPU: opens sam_path and reads its header as ngsq_sam_write_bam does.  NGSQ_OK, or an error whose message
 * (with its context "opening SAM input file: ") is written to why[why_cap].  n_refs (optional): the @SQ lines. */
int ngsq_sam_check_header(const char *sam_path, uint32_t *n_refs, char *why, size_t why_cap);

/* The BAM of the SAM text at sam_path, written to the descriptor fd: the header text unchanged, the reference list of its
 * @SQ lines, one record per line, BGZF blocks of 65280 bytes written by the device encoder, the EOF block.  ctx: a context
 * without facets and references (facets 0, n_refs 0).  max_records: at most this many records (0: all).  chunk_bytes: text
 * bytes that go to the device at a time (0: 64 MiB).  A line of up to chunk_bytes bytes fits, its newline not counted, so a
 * chunk holds up to chunk_bytes + 1 bytes (and the newline added to a last line that has none).  The decompressed stream depends on the input alone;
 * the compressed bytes also depend on chunk_bytes.  After a failure the content written to fd is not specified. */
int ngsq_sam_write_bam(ngsq_ctx *ctx, const char *sam_path, int fd, uint64_t max_records, uint64_t chunk_bytes, ngsq_samtext_report *out);

/* ---- `--sort coordinate`: the records stay in device memory until their order is known ---- */

typedef struct ngsq_samsort_report {
    uint64_t records;          /* records written */
    uint64_t header_bytes;     /* the header text as written (ngsq_sam_sorted_header) */
    uint64_t text_bytes;       /* the lines of the records written, their newlines included */
    uint64_t bam_bytes;        /* the decompressed stream: header, reference list and records */
    uint64_t compressed_bytes; /* the file: every block and the EOF block */
    uint64_t chunks;           /* chunks of text that went to the device */
    uint64_t pieces;           /* pieces of the sorted stream that were gathered and compressed */
    uint64_t blocks, stored_blocks; /* BGZF blocks (without the EOF block), and those of them with a stored payload */
    uint64_t resident_bytes;   /* what the budget was held against: the record bytes and 48 bytes per record */
    uint32_t passes_run, passes_skipped; /* of the sort's eight digits */
    double read_ms, h2d_ms, parse_ms, sort_ms, gather_ms, deflate_ms, d2h_ms, write_ms; /* as ngsq_samtext_report; sort: keys to sorted offsets */
    double total_ms;           /* wall clock */
} ngsq_samsort_report;

/* ngsq_sam_write_bam with the records in coordinate order: key = (refID < 0 || pos < 0 ? 0xFFFFFFFF : refID) << 32 | (pos + 1),
 * ascending, equal keys in input order, so that records without a sequence or a position come last and `ngs index` accepts
 * the file.  The header text is ngsq_sam_sorted_header's.  max_records: the first max_records records of the text are sorted
 * (0: all).  piece_bytes: sorted record bytes gathered and compressed at a time (0: 64 MiB).  max_resident_bytes: what the
 * record bytes and 48 bytes per record may take of device memory (0: what hipMemGetInfo reports free, less 4 GiB for the
 * call's other buffers); beyond it the call fails with NGSQ_ERR_LIMIT as soon as the running total shows it.  At most 2^32 - 1
 * records.  Every fault of the text is reported before anything is written to fd.  The decompressed stream depends on the
 * input and max_records alone; the compressed bytes also on piece_bytes. */
int ngsq_sam_write_sorted_bam(ngsq_ctx *ctx, const char *sam_path, int fd, uint64_t max_records, uint64_t chunk_bytes, uint64_t piece_bytes,
                              uint64_t max_resident_bytes, ngsq_samsort_report *out);

/* ngsq_sam_write_sorted_bam, and the BAI of what it writes at bai_path: the counterpart of ngsq_bam_write_sorted_bam_indexed
 * (ngsq_bamsort.h), with its arguments, refusals and report; the sequences' lengths are the @SQ LN of the text's header, and
 * the messages of the index begin "reading SAM record: ". */
int ngsq_sam_write_sorted_bam_indexed(ngsq_ctx *ctx, const char *sam_path, int fd, uint64_t max_records, uint64_t chunk_bytes, uint64_t piece_bytes,
                                      uint64_t max_resident_bytes, ngsq_samsort_report *out, const char *bai_path, uint64_t index_tile_records,
                                      ngsq_index_report *index_out);

/* Host only, no GPU: the header text of a coordinate-sorted file made from text[n].  The first SO: field of the @HD line
 * (the line ngsq_bam_sorted_by_coordinate reads) becomes SO:coordinate, or is appended to that line; its SS: fields whose
 * value does not start with "coordinate:" are dropped; without an @HD line "@HD\tVN:1.6\tSO:coordinate\n" is put in front.
 * *out_n = the bytes of the result, also when cap is too small: that case returns NGSQ_ERR_BUFFER_TOO_SMALL and writes nothing. */
int ngsq_sam_sorted_header(const char *text, size_t n, char *out, size_t cap, size_t *out_n);

/* The bits of the f32 an `f` value reads as (Rust's f32::from_str: DESIGN.md section 18.1) -- the function the kernels use,
 * on the host.  NGSQ_OK, or NGSQ_ERR_INVALID_ARGUMENT for a text that is no float or is longer than 48 characters. */
int ngsq_sam_parse_f32(const char *text, uint32_t len, uint32_t *bits);

#ifdef __cplusplus
}
#endif
#endif
