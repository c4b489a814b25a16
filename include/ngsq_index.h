/*
 * ngsq_index.h -- `ngs index` for BAM: the BAI of a coordinate-sorted file, built on the GPU from the batches of the
 * device ingest (ngsq_bam.h).  DESIGN.md section 12 has the rules; they follow the reference's src/index/bam.rs:39-109
 * and the index writers of samtools (SAM/BAM specification 5.2 and 5.3).
 */
#ifndef NGSQ_INDEX_H
#define NGSQ_INDEX_H

#include "ngsq.h"
#include "ngsq_bam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What one index build did. */
typedef struct ngsq_index_report {
    uint64_t records;   /* records of the file */
    uint64_t n_no_coor; /* records without a reference sequence or position (the BAI's n_no_coor) */
    uint64_t runs;      /* runs of records of one (sequence, bin): the chunks of the index */
    uint64_t bins;      /* bins written over all sequences, the metadata pseudo-bin 37450 not counted */
    double scan_ms;     /* device ingest and the index kernels, up to the index on the host */
    double write_ms;    /* the file written from it */
} ngsq_index_report;

/* Scan the whole file of `bam` (opened by ngsq_bam_open, no batch read yet) through the device ingest on ctx's device and
 * write its BAI to bai_path (the reference: "<BAM>.bai").  ctx may be created with facets 0: nothing of the qc state is used.
 * Refused before the scan: an existing bai_path (NGSQ_ERR_INVALID_ARGUMENT, "refusing to overwrite existing index file: ..."),
 * a header whose @HD lacks SO:coordinate (NGSQ_ERR_UNSORTED, "the input BAM must be coordinate-sorted to be indexed").
 * A record whose (sequence, position) goes backwards, or a placed record behind an unplaced one: NGSQ_ERR_UNSORTED, the
 * message names the record's index in the file.  A record the BAI cannot hold (position beyond 2^29, or reaching more than
 * 1 Mbp beyond its @SQ LN): NGSQ_ERR_LIMIT.  On any error no file is left at bai_path.  Messages: ngsq_bam_last_error().
 * out (optional) receives the report. */
int ngsq_bam_build_index(ngsq_bam *bam, ngsq_ctx *ctx, const char *bai_path, ngsq_index_report *out);

#ifdef __cplusplus
}
#endif
#endif
