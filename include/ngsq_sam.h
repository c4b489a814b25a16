/*
 * ngsq_sam.h -- `ngs convert <BAM> <SAM>`: the SAM text of a BAM file, formatted on the GPU from the batches of the device
 * ingest (ngsq_bam.h).  DESIGN.md section 13 has the rules; they follow the reference's src/convert/bam.rs:24-70
 * (to_sam_async) and the SAM writer of noodles-sam as this project reads it.
 */
#ifndef NGSQ_SAM_H
#define NGSQ_SAM_H

#include "ngsq.h"
#include "ngsq_bam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What one conversion did. */
typedef struct ngsq_sam_report {
    uint64_t records;      /* records written */
    uint64_t header_bytes; /* bytes of the header text written */
    uint64_t text_bytes;   /* bytes of the record lines written */
    uint64_t batches;      /* batches of the device ingest */
    double scan_ms;        /* host time inside the device ingest's calls (ngsq_bam_next_batch_device) */
    double format_ms;      /* GPU time of the formatter kernels (sizing pass, scan, write pass) */
    double copy_ms;        /* GPU time of the device-to-host copies of the text */
    double write_ms;       /* the writer thread's time inside write(2) */
    double total_ms;       /* wall clock of the call */
} ngsq_sam_report;

/* Write the SAM text of `bam` (opened by ngsq_bam_open, no batch read yet) to the file descriptor fd: the header text as
 * the file holds it (a final newline added when it lacks one, nothing for an empty text), then one line per record in file
 * order.  The records are scanned by the device ingest on ctx's device (ctx may be created with facets 0); the text is
 * formatted there, copied to a pinned ring on a second stream and written by a writer thread in order.
 * max_records: write at most this many records (0: all).  batch_records: records per ingest batch (0: the default).
 * A record that has no SAM text ends the call with NGSQ_ERR_INVALID_ARGUMENT and the message
 * "writing SAM record: record <i>: <what>" (i: its 0-based index in the file); what fd holds then is not specified.
 * A failing write: NGSQ_ERR_INVALID_ARGUMENT, "writing SAM record: <strerror> (os error N)".  Messages: ngsq_bam_last_error().
 * out (optional) receives the report. */
int ngsq_bam_write_sam(ngsq_bam *bam, ngsq_ctx *ctx, int fd, uint64_t max_records, uint64_t batch_records, ngsq_sam_report *out);

#ifdef __cplusplus
}
#endif
#endif
