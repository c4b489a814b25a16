/*
 * ngsq_collate.h -- `ngs fastq --collate [--singletons <FILE>] <BAM> <READ_ONES_FILE> [<READ_TWOS_FILE>]`: the reads of a BAM
 * file as FASTQ text with the mates paired by name, whatever the order of the file.  `ngs fastq`
 * (ngsq_fastq.h) writes read ones and read twos in file order, which pairs them only in a name-grouped file; from a
 * coordinate-sorted BAM this call gives the two files an aligner takes.  The kept records are held in device memory, their names
 * are hashed, sorted and compared on the GPU, and the text is written there in pair order.  The reference has no such command:
 * every rule below is this build's own decision, and tests/fastq_collate_model.py restates it.
 *
 * Kept, class and text are ngsq_fastq.h's, exactly: a record is kept iff (flag & exclude_flags) == 0,
 * (flag & require_flags) == require_flags and l_seq >= 1 (else it is counted as excluded or no_sequence); it is a read one
 * (0x40 without 0x80), a read two (0x80 without 0x40) or an other; its four lines are those of ngsq_fastq.h, with the
 * reverse-complement on 0x10, the missing QUAL, name_suffix and default_quality.  max_records examines the first records only.
 *
 * Name.  The l_read_name - 1 bytes in front of the name's NUL, compared exactly; nothing is stripped, so "x/1" and "x/2" are
 * two names.  A name group is the kept read ones and read twos of equal name.  Others never take part.
 * Pair.  A group with exactly one read one and exactly one read two is a pair.
 * Singletons.  Every other kept read one or read two is a singleton.  If its group holds more than one read one, or more than
 * one read two, it is also counted as ambiguous.
 * Pair order.  Pairs are written in the order of the file index of their earlier record: for a coordinate-sorted BAM the order
 * of the leftmost mate.
 *
 * Two-file mode (fd_two >= 0).  Pair p's read one is record p of fd_one and its read two is record p of fd_two: the two files
 * correspond line by line, always.  Singletons, ones and twos together, go to fd_single in file order, or, with fd_single < 0,
 * nowhere: they are dropped and counted (dropped_singletons).  Others go to fd_other in file order or are dropped and counted
 * (dropped_other).
 * One-file mode (fd_two < 0).  fd_one is interleaved: pair p's read one, then its read two.  fd_single as above.  fd_other must
 * be < 0: others are dropped and counted.
 *
 * Quality error.  Every kept record -- also one that ends up dropped -- is checked for a present score above 93:
 * NGSQ_ERR_INVALID_ARGUMENT, "writing FASTQ record: record <i>: quality score above 93", the smallest file index.  The check
 * is made during the walk, before any output receives a byte: on this error a text output is 0 bytes long.
 *
 * Residence.  The kept records lie in device memory (records that are not kept are never stored), with
 * ngsq_collate_bytes_per_record() bytes of arrays each.  Beyond memory_budget the call is refused: NGSQ_ERR_LIMIT, "fastq
 * --collate holds the kept records in device memory: N bytes needed, M allowed"; more than 2^32 - 1 kept records likewise.
 * Collation in rounds is not built.  Outside the budget, as for `ngs convert --sort coordinate`: the arrays' spare capacity
 * (they double as they grow, so up to as much again for three of them, 20 bytes a record), and the text of the pieces, two
 * buffers of piece_records entries per output -- 0.7 GB each at the default for pairs of 150 bases, what the default budget's
 * reserve leaves room for.  A piece is cut by entries, not by bytes: a file of very long reads wants a smaller piece_records,
 * and a piece whose text cannot be allocated ends the call with NGSQ_ERR_DEVICE, "allocating N bytes for a piece's FASTQ text".
 *
 * Run limit.  The mate search compares a record with the records that share its sorted key, which is quadratic in the run.
 * If more than NGSQ_COLLATE_MAX_RUN read ones and twos share one key, the call is refused before the search is launched:
 * NGSQ_ERR_LIMIT, "fastq --collate: more than 1024 reads share a name or a name hash".  Exactly 1024 reads of one name are
 * accepted: singletons, and ambiguous.
 *
 * Independence.  The decompressed bytes of every output and every count follow from the file and the options above alone: not
 * from the hash function, hash_bits, batch_records, piece_records, the budget, or where an output is compressed.
 */
#ifndef NGSQ_COLLATE_H
#define NGSQ_COLLATE_H

#include "ngsq.h"
#include "ngsq_bam.h"
#include "ngsq_fastq.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NGSQ_COLLATE_MAX_RUN 1024u

/* the fourth output, as the report's arrays and bgzf_mask's bits number it (0 to 2: NGSQ_FASTQ_ONE / _TWO / _OTHER) */
#define NGSQ_FASTQ_SINGLE 3

typedef struct ngsq_collate_options {
    uint32_t struct_size;     /* sizeof(ngsq_collate_options) */
    uint32_t require_flags;   /* <= 65535 */
    uint32_t exclude_flags;   /* <= 65535 */
    uint32_t default_quality; /* <= 93 */
    uint32_t name_suffix;     /* 0 or 1 */
    uint32_t bgzf_mask;       /* bit 0 / 1 / 2 / 3: fd_one / fd_two / fd_other / fd_single receives BGZF from the device encoder and
                                 the EOF block at the end; a bit of an output that is not given is refused */
    uint32_t hash_bits;       /* 0: the whole name hash; 1 to 63: only that many low bits of it, so that unlike names meet in
                                 one run (for tests: the outputs do not depend on it) */
    uint32_t reserved;        /* 0 */
    uint64_t max_records;     /* examine only the first max_records records of the file, kept or not (0: all) */
    uint64_t batch_records;   /* records per ingest batch (0: the default) */
    uint64_t piece_records;   /* pairs (of the pair outputs) or records (of the others' and the singletons') per write piece
                                 (0: the default) */
    uint64_t memory_budget;   /* what the resident records and their arrays may take of device memory (0: what is free, less the
                                 reserve of `ngs convert --sort coordinate`) */
} ngsq_collate_options;

/* What one call did.  Arrays: [NGSQ_FASTQ_ONE], [NGSQ_FASTQ_TWO], [NGSQ_FASTQ_OTHER], [NGSQ_FASTQ_SINGLE]. */
typedef struct ngsq_collate_report {
    uint64_t records_scanned;     /* as ngsq_fastq_report's, these seven */
    uint64_t excluded;
    uint64_t no_sequence;
    uint64_t reads_one;
    uint64_t reads_two;
    uint64_t reads_other;
    uint64_t dropped_other;
    uint64_t pairs;               /* name groups of exactly one read one and one read two */
    uint64_t singletons;          /* kept read ones and twos outside a pair, written or dropped */
    uint64_t ambiguous;           /* ... of which in a group with more than one read one or more than one read two */
    uint64_t dropped_singletons;  /* singletons that had no output (fd_single < 0) */
    uint64_t name_collisions;     /* read ones and twos that met a record of another name in the run of their key */
    uint64_t batches;             /* batches of the device ingest */
    uint64_t resident_records;    /* kept records */
    uint64_t resident_bytes;      /* their bytes and ngsq_collate_bytes_per_record() each: what memory_budget is held against */
    uint64_t sort_passes;         /* radix passes that ran (of 8) */
    uint64_t pieces;              /* write pieces, all lists */
    uint64_t text_bytes[4];       /* FASTQ text per output, before compression */
    uint64_t compressed_bytes[4]; /* bytes written to a BGZF output, its EOF block included (0 for a text output) */
    uint64_t blocks;              /* BGZF blocks of all outputs, the EOF blocks aside */
    uint64_t stored_blocks;       /* ... of which stored */
    double scan_ms;               /* host time inside the device ingest's calls */
    double walk_ms;               /* wall clock of the walk: the ingest, the flag pass, the keep and the score check of every batch */
    double match_ms;              /* stream time from the name hash to the last list: the kernels of the hash, the sort, the run check,
                                     the mate search and the lists, and the waits between them (the sort's histogram, the run
                                     check's word and the three lists' lengths come to the host) */
    double format_ms;             /* stream time of the pieces' size passes and scans, and of their write passes */
    double deflate_ms;            /* GPU time of the encoder */
    double copy_ms;               /* GPU time of the device-to-host copies, all outputs */
    double write_ms;              /* the writer threads' time inside write(2), all outputs */
    double total_ms;              /* wall clock of the call */
} ngsq_collate_report;

/* device bytes per resident record beside the record's own */
uint64_t ngsq_collate_bytes_per_record(void);

/* Write the reads of `bam` (opened by ngsq_bam_open, no batch read yet: NGSQ_ERR_STATE otherwise) to the file descriptors, as
 * described above.  fd_one >= 0.  fd_two < 0: one-file mode; fd_other must be < 0 then.  fd_other < 0: others are dropped.
 * fd_single < 0: singletons are dropped.
 * A null argument, a struct_size other than the structure's, a flag word above 65535, default_quality above 93, name_suffix
 * above 1, hash_bits above 63, reserved other than 0, a bgzf_mask bit without its output, or a descriptor combination other than those above:
 * NGSQ_ERR_INVALID_ARGUMENT, before the header is looked at and before anything is written.
 * A failing write: NGSQ_ERR_INVALID_ARGUMENT, "could not write record to read one file: <strerror> (os error N)", and
 * "... read two file", "... other reads file", "... singletons file".  Messages: ngsq_bam_last_error().  out (optional)
 * receives the report. */
int ngsq_bam_write_fastq_collated(ngsq_bam *bam, ngsq_ctx *ctx, int fd_one, int fd_two, int fd_other, int fd_single,
                                  const ngsq_collate_options *opt, ngsq_collate_report *out);

#ifdef __cplusplus
}
#endif
#endif
