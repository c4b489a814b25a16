/*
 * ngsq_derive.h -- `ngs derive instrument` for BAM: the distinct instrument ids and flowcell ids of the read names,
 * collected on the GPU from the batches of the device ingest (ngsq_bam.h), and the sequencer predicted from them on the host.
 * DESIGN.md section 14 has the rules; they follow the reference's src/derive/command/instrument.rs:53-110,
 * src/derive/instrument/reads.rs:35-64 and src/derive/instrument/compute.rs:103-283.
 */
#ifndef NGSQ_DERIVE_H
#define NGSQ_DERIVE_H

#include <stddef.h>

#include "ngsq.h"
#include "ngsq_bam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The two sets of one scan: byte strings (any byte, possibly empty), each once, ascending by bytes. */
typedef struct ngsq_derive_names ngsq_derive_names;

#define NGSQ_DERIVE_INSTRUMENTS 0
#define NGSQ_DERIVE_FLOWCELLS 1

/* Capacity of one scan on the device.  Every string the kernel could not find in its table is appended to a string arena
 * and to an entry list, duplicates included; a file that needs more of either ends the scan with
 * NGSQ_ERR_LIMIT.  A file with up to NGSQ_DERIVE_TABLE_SLOTS / 2 distinct names per set appends each about once. */
#define NGSQ_DERIVE_ARENA_BYTES (32u << 20)
#define NGSQ_DERIVE_MAX_ENTRIES (2u << 20)
#define NGSQ_DERIVE_TABLE_SLOTS (1u << 16) /* per set; the default of table_slots */

/* What one scan did. */
typedef struct ngsq_derive_report {
    uint64_t records;     /* records examined */
    uint64_t skipped;     /* of them: records whose name is absent ("*") */
    uint64_t instruments; /* distinct instrument ids */
    uint64_t flowcells;   /* distinct flowcell ids */
    uint64_t entries;     /* strings the device appended: the distinct ones and the candidates */
    uint64_t candidates;  /* of them: appended without a table slot, left to the host to de-duplicate */
    uint64_t batches;     /* batches of the device ingest */
    double scan_ms;       /* host time inside the device ingest's calls (ngsq_bam_next_batch_device) */
    double kernel_ms;     /* GPU time of the name kernel */
    double total_ms;      /* wall clock of the call */
} ngsq_derive_report;

/* Scan the records of `bam` (opened by ngsq_bam_open, no batch read yet) through the device ingest on ctx's device (ctx
 * may be created with facets 0) and return the distinct instrument ids and flowcell ids of their names in *out (release
 * it with ngsq_derive_names_free).  A name is the stored name without its NUL; "*" is skipped; any other name is split
 * at every ':' -- 5 segments: the instrument is segment 0; 7 segments: the instrument is segment 0, the flowcell segment 2.
 * Any other count ends the call with NGSQ_ERR_INVALID_ARGUMENT and the message
 * "Could not parse Illumina-formatted query names for read: <name>", naming the first such record in file order.
 * max_records: examine at most this many records (0: all).  batch_records: records per ingest batch (0: the default).
 * table_slots: slots of each set's table on the device, a power of two (0: NGSQ_DERIVE_TABLE_SLOTS); the result does not
 * depend on it.  Messages: ngsq_bam_last_error().  rep (optional) receives the report. */
int ngsq_bam_derive_instrument(ngsq_bam *bam, ngsq_ctx *ctx, uint64_t max_records, uint64_t batch_records, uint32_t table_slots,
                               ngsq_derive_names **out, ngsq_derive_report *rep);
/* which: NGSQ_DERIVE_INSTRUMENTS or NGSQ_DERIVE_FLOWCELLS */
uint64_t ngsq_derive_names_count(const ngsq_derive_names *names, int which);
/* string i of the set (not NUL-terminated inside its length; *len receives the length); NULL: no such string */
const char *ngsq_derive_names_get(const ngsq_derive_names *names, int which, uint64_t i, uint32_t *len);
void ngsq_derive_names_free(ngsq_derive_names *names);

/* Host only.  The machines whose pattern `query` (len bytes) matches in the instrument table (which =
 * NGSQ_DERIVE_INSTRUMENTS) or the flowcell table (NGSQ_DERIVE_FLOWCELLS): their names ascending by bytes, each followed
 * by '\n', then a NUL, written to out[0, cap).  *need (optional) receives the bytes that takes, the NUL included; a smaller
 * cap writes nothing and returns NGSQ_ERR_BUFFER_TOO_SMALL. */
int ngsq_derive_lookup(int which, const char *query, uint32_t len, char *out, size_t cap, size_t *need);

/* Host only.  The document `ngs derive instrument` prints for these instrument ids and flowcell ids (each a set: a string
 * given twice counts once): keys succeeded, instruments, confidence, evidence, comment, two spaces of indent, `instruments`
 * ascending by bytes, no final newline; NUL-terminated in json[0, cap).  *need (optional) receives the bytes that takes, the
 * NUL included; a smaller cap writes nothing and returns NGSQ_ERR_BUFFER_TOO_SMALL. */
int ngsq_derive_predict(const char *const *instruments, const uint32_t *instrument_lens, uint64_t n_instruments,
                        const char *const *flowcells, const uint32_t *flowcell_lens, uint64_t n_flowcells, char *json, size_t cap,
                        size_t *need);

#ifdef __cplusplus
}
#endif
#endif
