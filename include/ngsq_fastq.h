/*
 * ngsq_fastq.h -- `ngs fastq <BAM> <READ_ONES_FILE> [<READ_TWOS_FILE>]`: the reads of a BAM file as FASTQ text.  The records
 * are read by the device ingest (one walk of the file, ngsq_bam.h), and every kept record's four lines are sized, placed
 * and written on the GPU, one device buffer per output; the output stage carries each buffer to its file descriptor, as text
 * or -- compressed there by the device DEFLATE encoder -- as BGZF.  The reference has no such command:
 * every rule below is this build's own decision, and tests/fastq_model.py restates it.
 *
 * Which records are kept.  A record is kept iff (flag & exclude_flags) == 0, (flag & require_flags) == require_flags and
 * l_seq >= 1.  A record that passes the two flag tests and has l_seq == 0 has no read to give: it is skipped and counted
 * (no_sequence).  A record that fails a flag test is counted as excluded, whatever its l_seq.
 *
 * Where a kept record goes.  Its class comes from the flag: a read one has 0x40 set and 0x80 clear, a read two has 0x80 set and
 * 0x40 clear, any other record (neither bit, or both) is an "other".  In one-file mode (fd_two < 0) every kept record goes to
 * fd_one.  In two-file mode read ones go to fd_one, read twos to fd_two, and others to fd_other, or, with fd_other < 0, nowhere:
 * they are dropped and counted (dropped_other).  The order within every output is file order.  Nothing is paired or collated:
 * the two files of a name-grouped BAM correspond line by line, those of a coordinate-sorted BAM hold the same reads in
 * different orders.  `ngs fastq --collate` (ngsq_collate.h) pairs the mates by name on the GPU, whatever the order of the file.
 *
 * What is written for a kept record: four lines,
 *
 *     @<name>[/1|/2]\n<SEQ>\n+\n<QUAL>\n
 *
 * <name>: the l_read_name - 1 bytes in front of the name's NUL, as they are (an empty name gives "@" alone).  With name_suffix,
 * "/1" behind the name of a read one and "/2" behind that of a read two, in either mode; an other gets none.
 * <SEQ>: the l_seq bases through "=ACMGRSVTWYHKDBN".  With flag 0x10 the read is reverse-complemented: the bases in reverse
 * order, each 4-bit code replaced by its four bits reversed (A<->T, C<->G, M<->K, R<->Y, V<->B, H<->D; S, W, N and = stay).
 * <QUAL>: every score + 33; with flag 0x10 in reverse order.  QUAL is missing when its first byte is 0xFF: the line then is
 * l_seq copies of default_quality + 33.
 * The record takes l_read_name - 1 + 2 l_seq + 6 bytes, and 2 more with a suffix.
 *
 * A kept record whose QUAL is present and holds a score above 93 ends the call: NGSQ_ERR_INVALID_ARGUMENT, "writing FASTQ
 * record: record <i>: quality score above 93", <i> the record's 0-based index in the file, the smallest index of such a
 * record.  Records that are not kept are not checked.  What the outputs hold after
 * this error is unspecified.
 *
 * The decompressed bytes of every output depend on the file and the options alone: not on batch_records, the grid, or where
 * a compressed output is compressed.  An output that receives no record is empty: no byte as text, the 28-byte EOF block alone
 * as BGZF.
 */
#ifndef NGSQ_FASTQ_H
#define NGSQ_FASTQ_H

#include "ngsq.h"
#include "ngsq_bam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the default of --exclude-flags: secondary, supplementary (0x100 | 0x800), as `samtools fastq` */
#define NGSQ_FASTQ_EXCLUDE_FLAGS 2304u
#define NGSQ_FASTQ_DEFAULT_QUALITY 1u
#define NGSQ_FASTQ_MAX_QUALITY 93u

/* the outputs, as the report's arrays and bgzf_mask's bits number them */
#define NGSQ_FASTQ_ONE 0
#define NGSQ_FASTQ_TWO 1
#define NGSQ_FASTQ_OTHER 2

typedef struct ngsq_fastq_options {
    uint32_t struct_size;     /* sizeof(ngsq_fastq_options) */
    uint32_t require_flags;   /* <= 65535 */
    uint32_t exclude_flags;   /* <= 65535 */
    uint32_t default_quality; /* <= 93: the score of every base of a record without QUAL */
    uint32_t name_suffix;     /* 0 or 1 */
    uint32_t bgzf_mask;       /* bit 0 / 1 / 2: fd_one / fd_two / fd_other receives BGZF from the device encoder (at the context's
                                 effort, ngsq_bgzf_set_effort) and the EOF block at the end; a bit of an output that is not given
                                 is refused */
    uint64_t max_records;     /* examine only the first max_records records of the file, kept or not (0: all) */
    uint64_t batch_records;   /* records per ingest batch (0: the default) */
} ngsq_fastq_options;

/* What one call did.  Arrays: [NGSQ_FASTQ_ONE], [NGSQ_FASTQ_TWO], [NGSQ_FASTQ_OTHER]. */
typedef struct ngsq_fastq_report {
    uint64_t records_scanned;     /* records the device ingest handed out */
    uint64_t excluded;            /* records that failed exclude_flags or require_flags */
    uint64_t no_sequence;         /* records that passed them with l_seq == 0 */
    uint64_t reads_one;           /* kept records by class (in one-file mode all three go to fd_one) */
    uint64_t reads_two;
    uint64_t reads_other;         /* kept others, written or dropped */
    uint64_t dropped_other;       /* kept others that had no output (two-file mode, fd_other < 0) */
    uint64_t batches;             /* batches of the device ingest that were formatted */
    uint64_t text_bytes[3];       /* FASTQ text per output, before compression */
    uint64_t compressed_bytes[3]; /* bytes written to a BGZF output, its EOF block included (0 for a text output) */
    uint64_t blocks;              /* BGZF blocks of all outputs, the EOF blocks aside */
    uint64_t stored_blocks;       /* ... of which stored */
    double scan_ms;               /* host time inside the device ingest's calls */
    double format_ms;             /* GPU time of the size/classify pass, the scans and the write pass */
    double deflate_ms;            /* GPU time of the encoder */
    double copy_ms;               /* GPU time of the device-to-host copies, all outputs */
    double write_ms;              /* the writer threads' time inside write(2), all outputs */
    double total_ms;              /* wall clock of the call */
} ngsq_fastq_report;

/* Write the reads of `bam` (opened by ngsq_bam_open, no batch read yet: NGSQ_ERR_STATE otherwise) to the file descriptors, as
 * described above.  fd_one >= 0.  fd_two < 0: one-file mode; fd_other must be < 0 then.  fd_other < 0 in two-file mode: others
 * are dropped.  The records are scanned by the device ingest on ctx's device (ctx may be created with facets 0).
 * A null argument, a struct_size other than the structure's, a flag word above 65535, default_quality above 93, name_suffix
 * above 1, a bgzf_mask bit without its output, or a descriptor combination other than those above: NGSQ_ERR_INVALID_ARGUMENT,
 * before the header is looked at and before anything is written.
 * A failing write: NGSQ_ERR_INVALID_ARGUMENT, "could not write record to read one file: <strerror> (os error N)", and
 * "... read two file", "... other reads file".  Messages: ngsq_bam_last_error().  out (optional) receives the report. */
int ngsq_bam_write_fastq(ngsq_bam *bam, ngsq_ctx *ctx, int fd_one, int fd_two, int fd_other, const ngsq_fastq_options *opt,
                         ngsq_fastq_report *out);

#ifdef __cplusplus
}
#endif
#endif
