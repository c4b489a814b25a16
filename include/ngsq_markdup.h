/*
 * ngsq_markdup.h -- `ngs markdup [--remove] [--metrics <FILE>] <BAM> <OUT_BAM>`: the duplicate reads of a BAM file marked
 * with flag 0x400, or left out, on the GPU.  The records are held in device memory, their unclipped 5'
 * ends and quality scores are computed there, mates are found by name as `ngs fastq --collate` finds them (ngsq_collate.h),
 * pairs and fragments of equal ends are grouped by the project's radix sort, and the file is written by the device encoder.
 * The reference has no such command: every rule below is this build's own decision, and tests/markdup_model.py restates it.
 *
 * Output.  The input's header text (the NUL padding at its end aside), its reference list and its records, in input order and
 * byte for byte, as BGZF from the device encoder.  Byte 19 of a record (counted from its block_size) holds flag bit 0x400, and
 * only that byte may differ: an existing 0x400 is cleared on every record, then set on the duplicates.  With `remove` the
 * duplicates are left out instead; 0x400 is still cleared on the records that stay.  The decompressed stream depends on the
 * file, max_records and remove alone: not on batch_records, piece_bytes, hash_bits, the budget or the encoder's effort.
 *
 * Candidate.  A record is a candidate iff none of 0x4, 0x100 and 0x800 is set and refID >= 0 and pos >= 0.  All other records
 * are never marked (secondary and supplementary records do not follow their primary).
 * End of a candidate, (ref, u, s).  s = flag & 0x10.  Forward: u = pos - (the sum of the leading run of S and H operations).
 * Reverse: u = pos + (the reference length of M, D, N, = and X) - 1 + (the sum of the trailing run of S and H operations).  I
 * and P take no part.  A CIGAR of zero operations gives u = pos either way.  The CIGAR is the record's own field: a CG tag is
 * not looked at.  u is computed in 64 bits; a candidate with u outside [-2^30, 2^31 - 2^30) is refused before anything is
 * written: NGSQ_ERR_LIMIT, "reading BAM record: record N (0-based): unclipped end outside what markdup can hold", the
 * smallest N.  The packed end is ref << 33 | (u + 2^30) << 1 | s.
 * Score.  The sum of the QUAL bytes that are >= 15; a missing QUAL (first byte 0xFF) scores 0.  The score is 32 bits wide and is
 * not capped: it is the sum modulo 2^32, and a pair's score the sum of its two scores modulo 2^32.
 * Pair.  A candidate is a pair candidate iff it has 0x1, has 0x8 clear, and has exactly one of 0x40 and 0x80.  Names are
 * compared exactly, as in ngsq_collate.h.  A name whose pair candidates are exactly one read one and one read two is a pair.
 * Every other candidate is a fragment: an unpaired read, a read whose mate is unmapped, absent or cut off by max_records, a read
 * whose name is ambiguous (more than one read one or more than one read two among its pair candidates; these are counted).
 * Read groups and libraries are ignored: the file is one library.  Optical duplicates are not told apart.
 * Run limit.  More than NGSQ_COLLATE_MAX_RUN (1024) pair candidates of one name, or of one name hash, are refused before the mate
 * search: NGSQ_ERR_LIMIT, "markdup: more than 1024 reads share a name or a name hash".  Exactly 1024 are accepted.  The limit
 * is the mate search's; runs of equal ends have none.
 * Pair duplicates.  A pair's key is its two packed ends in ascending order, 128 bits.  Among pairs of equal key the one with the
 * largest score survives, ties going to the pair whose earlier record has the smaller file index; both records of every other
 * pair of the group are duplicates.
 * Fragment duplicates.  All candidates, pair members and fragments, are grouped by packed end.  If any pair member has that end,
 * every fragment with it is a duplicate; otherwise the fragment of the largest score survives (ties to the smaller file index)
 * and the others are duplicates.  A pair member is never made a duplicate by this rule.
 *
 * Residence.  Every record of the file lies in device memory with ngsq_markdup_bytes_per_record() bytes of arrays each.  Beyond
 * memory_budget the call is refused: NGSQ_ERR_LIMIT, "markdup holds the records in device memory: N bytes needed, M allowed";
 * more than 2^32 - 1 records likewise.  Marking in rounds is not built.
 * Errors.  Every refusal above, and every fault of the input, is known before the first byte is written: the descriptor has
 * received nothing.  A failing write (NGSQ_ERR_INVALID_ARGUMENT, "writing BAM record: <strerror> (os error N)") leaves a partial
 * file.  The command line refuses an output that exists, so the file is its own: it removes it after every error.
 */
#ifndef NGSQ_MARKDUP_H
#define NGSQ_MARKDUP_H

#include "ngsq.h"
#include "ngsq_bam.h"
#include "ngsq_collate.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ngsq_markdup_options {
    uint32_t struct_size;   /* sizeof(ngsq_markdup_options) */
    uint32_t remove;        /* 0: duplicates are marked; 1: they are left out */
    uint32_t hash_bits;     /* 0: the whole name hash; 1 to 63: only that many low bits of it (for tests, as ngsq_collate_options') */
    uint32_t reserved;      /* 0 */
    uint64_t max_records;   /* examine, and write, only the first max_records records of the file (0: all) */
    uint64_t batch_records; /* records per ingest batch (0: the default) */
    uint64_t piece_bytes;   /* bytes of the record stream per write piece (0: the default of `ngs convert --sort coordinate`) */
    uint64_t memory_budget; /* what the resident records and their arrays may take of device memory (0: what is free, less the
                               reserve of `ngs convert --sort coordinate`) */
} ngsq_markdup_options;

typedef struct ngsq_markdup_report {
    uint64_t records;             /* records examined */
    uint64_t candidates;
    uint64_t pairs;
    uint64_t fragments;           /* candidates - 2 pairs */
    uint64_t duplicate_pairs;
    uint64_t duplicate_fragments;
    uint64_t duplicate_records;   /* duplicate_fragments + 2 duplicate_pairs: the records marked, or left out */
    uint64_t cleared;             /* records that came in with 0x400 */
    uint64_t ambiguous;           /* pair candidates whose name has more than one read one or more than one read two */
    uint64_t name_collisions;     /* pair candidates that met a record of another name in the run of their key */
    double duplication;           /* (duplicate_fragments + 2 duplicate_pairs) / (fragments + 2 pairs); 0 when the divisor is 0 */
    uint64_t batches;             /* batches of the device ingest */
    uint64_t resident_bytes;      /* the records' bytes and ngsq_markdup_bytes_per_record() each: what memory_budget is held against */
    uint64_t sort_passes;         /* radix passes that ran, all four sorts (the names, the pairs' two words, the fragments) */
    uint64_t pieces;              /* write pieces */
    uint64_t blocks;              /* BGZF blocks, the EOF block aside */
    uint64_t stored_blocks;       /* ... of which stored */
    uint64_t bam_bytes;           /* the header and the records written, before compression */
    uint64_t compressed_bytes;    /* bytes written, the EOF block included */
    double scan_ms;               /* host time inside the device ingest's calls */
    double walk_ms;               /* wall clock of the walk: the ingest and the keep of every batch */
    double ends_ms;               /* stream time of the ends-and-scores pass */
    double match_ms;              /* stream time from the name hash to the mates, with the waits between */
    double mark_ms;               /* stream time of the pair mark, the fragment mark and the flag bytes */
    double gather_ms;             /* stream time of the pieces' gathers */
    double deflate_ms;            /* GPU time of the encoder */
    double d2h_ms;                /* GPU time of the device-to-host copies */
    double write_ms;              /* the writer thread's time inside write(2) */
    double total_ms;              /* wall clock of the call */
} ngsq_markdup_report;

/* device bytes per resident record beside the record's own */
uint64_t ngsq_markdup_bytes_per_record(void);

/* Write the records of `bam` (opened by ngsq_bam_open, no batch read yet: NGSQ_ERR_STATE otherwise) to fd as a BAM file with
 * the duplicates marked or removed, as described above.  A null argument, fd < 0, a struct_size other than the structure's,
 * remove above 1, hash_bits above 63 or reserved other than 0: NGSQ_ERR_INVALID_ARGUMENT, before the header is looked at.
 * Messages: ngsq_bam_last_error().  out (optional) receives the report. */
int ngsq_bam_mark_duplicates(ngsq_bam *bam, ngsq_ctx *ctx, int fd, const ngsq_markdup_options *opt, ngsq_markdup_report *out);

#ifdef __cplusplus
}
#endif
#endif
