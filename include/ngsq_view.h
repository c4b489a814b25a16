/*
 * ngsq_view.h -- `ngs view <BAM> [QUERY]`: the SAM text of a BAM file or of one region of it.  A region's records are found
 * through the file's BAI (the chunk query below, on the host), read by range walks of the device ingest (ngsq_bam_range_begin,
 * ngsq_bam.h), selected on the GPU and formatted there by the kernels of `ngs convert` (ngsq_sam.h).  DESIGN.md section 15 has
 * the rules; they follow the reference's src/view/command.rs and src/view/bam.rs, and where those lean on crates this project
 * cannot read (the region grammar, the index query) they are this build's own decisions, written down there.
 */
#ifndef NGSQ_VIEW_H
#define NGSQ_VIEW_H

#include "ngsq.h"
#include "ngsq_bam.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NGSQ_VIEW_FULL 0u         /* the header text, then the records */
#define NGSQ_VIEW_HEADER_ONLY 1u  /* the header text; needs no GPU (ctx may be NULL) */
#define NGSQ_VIEW_RECORDS_ONLY 2u /* the records */

/* the end of an interval without one ("chr1", "chr1:5"): the coordinate range of the binning scheme, 2^29 */
#define NGSQ_VIEW_END_MAX ((uint64_t)1 << 29)

/* virtual offsets [begin, end) of the file that may hold records of a region */
typedef struct ngsq_view_chunk {
    uint64_t begin, end;
} ngsq_view_chunk;

/* What one view did. */
typedef struct ngsq_view_report {
    uint64_t records_scanned; /* records the device ingest handed out */
    uint64_t records_written; /* records selected and written */
    uint64_t header_bytes;    /* bytes of the header text written */
    uint64_t text_bytes;      /* bytes of the record lines written */
    uint64_t chunks;          /* merged chunks of the query (0 without one) */
    uint64_t ranges;          /* range walks of the device ingest (0 without a query: one walk of the whole file) */
    uint64_t batches;         /* batches of the device ingest */
    double scan_ms;           /* host time inside the device ingest's calls */
    double select_ms;         /* GPU time of the selection kernel */
    double format_ms;         /* GPU time of the formatter kernels */
    double copy_ms;           /* GPU time of the device-to-host copies of the text */
    double write_ms;          /* the writer thread's time inside write(2) */
    double total_ms;          /* wall clock of the call */
} ngsq_view_report;

/* Parse `query` ("name", "name:S" or "name:S-E", 1-based inclusive; split at the last ':') against the reference sequences
 * of `bam` and return the chunks of the index bai_path (NULL: "<path of bam>.bai") that may hold its records: the bins of
 * reg2bins over [S-1, min(E, 2^29)) without the pseudo-bin 37450, chunks that end at or in front of the linear index's entry
 * for S dropped, the rest sorted by begin and merged where they touch or overlap.  *ref_id, *start, *end: the region
 * (*end = NGSQ_VIEW_END_MAX for an interval without an end).  chunks[0, min(*n, cap)) are filled; *n is the number there are
 * (chunks may be NULL with cap 0).  Host only, needs no GPU.
 * Errors, NGSQ_ERR_INVALID_ARGUMENT with ngsq_bam_last_error(): "parsing query: ..." (an empty query), "querying BAM file: ..."
 * (no such sequence), "reading BAM index: ..." (a missing or unparsable index, or one with fewer sequences than the region's id). */
int ngsq_bam_query_chunks(const ngsq_bam *bam, const char *bai_path, const char *query, uint32_t *ref_id, uint64_t *start,
                          uint64_t *end, ngsq_view_chunk *chunks, uint64_t cap, uint64_t *n);

/* Write the view of `bam` (opened by ngsq_bam_open, no batch read yet) to the file descriptor fd.
 * mode: NGSQ_VIEW_FULL / HEADER_ONLY / RECORDS_ONLY.  The header text is written exactly as the file holds it (no newline
 * added).  query NULL: every record, in file order, as ngsq_bam_write_sam writes them.  Otherwise the records of the region
 * (DESIGN.md section 15): those whose virtual offset lies in a merged chunk of ngsq_bam_query_chunks, whose sequence is the
 * region's, whose pos >= 0 and whose span [pos+1, pos+max(reference span, 1)] meets [S, E]; in file order.  A record that is not
 * selected is not examined for SAM text.  The query and the index are looked at before the first byte is written.
 * batch_records: records per ingest batch (0: the default).  coalesce_gap: merged chunks whose compressed-offset gap is below
 * this many bytes are read by one range walk (0: the default, 64 MiB; 1: a walk per merged chunk); the output does not
 * depend on it.
 * Errors: those of ngsq_bam_query_chunks; "writing BAM header to stream: <strerror> (os error N)"; "writing record to stream:
 * record <i>: <what>" (i: the record's 0-based index in the file) for a selected record without SAM text (section 13.3);
 * "writing record to stream: <strerror> (os error N)" for a failing write.  out (optional) receives the report. */
int ngsq_bam_view(ngsq_bam *bam, ngsq_ctx *ctx, int fd, const char *query, const char *bai_path, uint32_t mode,
                  uint64_t batch_records, uint64_t coalesce_gap, ngsq_view_report *out);

#ifdef __cplusplus
}
#endif
#endif
