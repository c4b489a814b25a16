/*
 * ngsq_generate.h -- `ngs generate`: paired FASTQ reads sampled from one or more reference FASTAs, drawn and written as text
 * on the GPU.  DESIGN.md section 16 has the rules; they follow the reference's src/generate/command.rs:30-131,
 * src/generate/providers/reference_provider.rs:89-173,197-260,284-394, src/generate/providers.rs:29-48,
 * src/generate/utils.rs:96-127 and src/utils/formats/fastq.rs:16-44.  The reference draws from ThreadRng; this build's
 * draws are a pure function of (seed, pair index, purpose, attempt or base index), so a seed names its two files.
 *
 * Messages: ngsq_generate_last_error() (per thread).
 */
#ifndef NGSQ_GENERATE_H
#define NGSQ_GENERATE_H

#include <stddef.h>

#include "ngsq.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ngsq_generate ngsq_generate;
typedef struct ngsq_gzip_pipe ngsq_gzip_pipe;

/* One reference provider: PATH:ERROR_FREQ:MU:SIGMA:READ_LENGTH:WEIGHT */
typedef struct ngsq_generate_provider {
    const char *path;     /* the reference FASTA */
    uint64_t error_freq;  /* one base in error_freq is substituted */
    double mu, sigma;     /* the normal distribution of the inner distance */
    uint64_t read_length; /* bases per read */
    uint64_t weight;      /* how often this provider is chosen, against the others' weights */
} ngsq_generate_provider;

#define NGSQ_GENERATE_MAX_TABLE (1u << 20)   /* most entries of an inner-distance table */
#define NGSQ_GENERATE_MAX_ATTEMPTS 1024u     /* attempts per pair before the call gives up */
#define NGSQ_GENERATE_MAX_READ_LENGTH (1u << 24)

const char *ngsq_generate_last_error(void);

/* ---- plain functions over caller memory (no file, no GPU; generate_args.cpp) ---------------------------------------------- */

/* Split `s` at every ':' into the six parts of a provider (reference_provider.rs:197-260, whose seven messages err receives
 * verbatim).  path receives PATH (out->path points at it).  Numbers parse as Rust's usize / f64 do: decimal digits with an
 * optional '+' for the integers; "nan", "inf", "infinity" in any case among the floats.  NGSQ_ERR_INVALID_ARGUMENT, or
 * NGSQ_ERR_LIMIT when path_cap is too small. */
int ngsq_generate_parse_provider(const char *s, char *path, size_t path_cap, ngsq_generate_provider *out, char *err, size_t err_cap);

/* What this build refuses up front of what the reference panics on, or spins on, later: error_freq 0 or above
 * 2^32 - 1, a non-finite mu, a non-finite or negative sigma, read_length 0 or above NGSQ_GENERATE_MAX_READ_LENGTH, an inner
 * distance whose lower bound makes a fragment shorter than a read, a table above the limit.  `name` names the provider. */
int ngsq_generate_check_provider(const ngsq_generate_provider *p, const char *name, char *err, size_t err_cap);

/* The inner distance of (mu, sigma): the integers lower .. lower + *n - 1 with
 *   lower = trunc(mu - floor(3 sigma)), upper = trunc(mu + ceil(3 sigma))            (reference_provider.rs:321-326)
 * and table[j] = floor(2^64 * P(round(X) clamped to [lower, upper] <= lower + j)) for X ~ N(mu, sigma), from erf in double,
 * non-decreasing, the last entry 2^64 - 1.  A 64-bit draw u selects lower + #{j < *n - 1 : table[j] <= u}.
 * table[0, min(*n, cap)) are filled; *n counts all.  NGSQ_ERR_LIMIT: more than NGSQ_GENERATE_MAX_TABLE entries, or bounds
 * beyond +-2^40. */
int ngsq_generate_inner_table(double mu, double sigma, int64_t *lower, uint64_t *table, uint64_t cap, uint64_t *n, char *err, size_t err_cap);

/* The 64-bit draw of (seed, pair, purpose, index); pure. */
uint64_t ngsq_generate_draw(uint64_t seed, uint64_t pair, uint32_t purpose, uint32_t index);

/* ---- the generator ---------------------------------------------------------------------------------------------------------- */

/* Host only: check the providers (ngsq_generate_check_provider; all weights 0), open every FASTA (ngsq_fasta_open: its
 * errors), count the bases of every record, refuse a file with a duplicate sequence name and a provider without a sequence
 * of at least 2 * read_length + 2 bases.  Touches no HIP. */
int ngsq_generate_open(const ngsq_generate_provider *providers, uint32_t n_providers, ngsq_generate **out);
void ngsq_generate_close(ngsq_generate *g);
/* coverage * (total bases of the FIRST provider / its read length), reference_provider.rs:171-173; saturates */
uint64_t ngsq_generate_reads_for_coverage(const ngsq_generate *g, uint64_t coverage);
/* sequences of provider p, their names and lengths in bases, in file order */
uint32_t ngsq_generate_n_sequences(const ngsq_generate *g, uint32_t p);
const char *ngsq_generate_sequence_name(const ngsq_generate *g, uint32_t p, uint32_t s);
uint64_t ngsq_generate_sequence_length(const ngsq_generate *g, uint32_t p, uint32_t s);

/* Bring the providers to ctx's device (a context created with facets 0 serves): the FASTA text crosses PCIe and is turned
 * into one letter per base there, case kept; the tables follow.  Once per generator. */
int ngsq_generate_load(ngsq_generate *g, ngsq_ctx *ctx);

/* What one call did. */
typedef struct ngsq_generate_report {
    uint64_t pairs;            /* pairs written to each file */
    uint64_t rejected_start;   /* attempts rejected: start == 0 */
    uint64_t rejected_end;     /* ... the fragment runs past the sequence's end */
    uint64_t rejected_base;    /* ... the fragment holds a byte outside ACGTacgt */
    uint64_t text_bytes_one;   /* bytes of text written to fd_one */
    uint64_t text_bytes_two;   /* ... to fd_two */
    uint64_t batches;
    double draw_ms;            /* GPU time of k_gen_draw and the scan */
    double format_ms;          /* GPU time of k_gen_write */
    double copy_ms;            /* GPU time of the device-to-host copies, both files */
    double write_ms;           /* the writer threads' time inside write(2), both files */
    double total_ms;           /* wall clock of the call */
} ngsq_generate_report;

/* Write pairs first_pair .. first_pair + n_pairs - 1 (named first_pair + 1 ...): read ones to fd_one, read twos to fd_two.
 * batch_pairs: pairs per launch (0: the default).  The bytes depend on (providers, seed, pair index) alone.
 * A pair without a fragment after NGSQ_GENERATE_MAX_ATTEMPTS attempts ends the call with NGSQ_ERR_INVALID_ARGUMENT and
 * "no read pair could be drawn from <file name> ..." (the smallest such pair's index in it); what the descriptors hold then
 * is not specified.  A failing write: "could not write record to read one file: <strerror> (os error N)" / "... two ...". */
int ngsq_generate_write(ngsq_generate *g, int fd_one, int fd_two, uint64_t seed, uint64_t first_pair, uint64_t n_pairs,
                        uint64_t batch_pairs, ngsq_generate_report *out);

/* ---- BGZF written on the device ------------------------------------------------------------------------- */

#define NGSQ_GENERATE_PLAIN_ONE 1u /* flags: fd_one receives plain text, as from ngsq_generate_write */
#define NGSQ_GENERATE_PLAIN_TWO 2u /* ... fd_two */

typedef struct ngsq_generate_bgzf_report {
    ngsq_generate_report text;     /* what ngsq_generate_write reports; copy_ms and write_ms are of the bytes that crossed */
    uint64_t compressed_bytes_one; /* bytes of BGZF written to fd_one, the EOF block among them (0: plain) */
    uint64_t compressed_bytes_two;
    uint64_t blocks, stored_blocks; /* BGZF blocks of both files without the EOF blocks; those left stored */
    double deflate_ms;              /* GPU time of the encoder, its CRC and its pack */
} ngsq_generate_bgzf_report;

/* ngsq_generate_write with each batch's text compressed on the device (ngsq_bgzf.h) behind the kernel that writes it: only
 * BGZF blocks cross to the host, and each descriptor receives the 28-byte EOF block after its last batch.  n_pairs == 0
 * writes the EOF block alone (and needs no ngsq_generate_load).  The DECOMPRESSED bytes depend on (providers, seed, pair
 * index) alone, as ngsq_generate_write's do; the compressed bytes also depend on batch_pairs, because every batch ends its
 * last block.  flags: 0, or NGSQ_GENERATE_PLAIN_* for a file that is to stay plain text.  Errors as ngsq_generate_write. */
int ngsq_generate_write_bgzf(ngsq_generate *g, int fd_one, int fd_two, uint64_t seed, uint64_t first_pair, uint64_t n_pairs,
                             uint64_t batch_pairs, uint32_t flags, ngsq_generate_bgzf_report *out);

/* ---- gzipped FASTQ ------------------------------------------------------------------------------------------------------------ */

/* A pipe whose read end is compressed (zlib level 6, one gzip member per piece of at most 1 MiB) by n_threads threads
 * (0: 8) and written to out_fd in order.  *write_fd: hand it to ngsq_generate_write and close it afterwards; then
 * ngsq_gzip_pipe_close waits for the last member (an input of no bytes gives one empty member) and reports a failed write. */
int ngsq_gzip_pipe_open(int out_fd, int n_threads, ngsq_gzip_pipe **out, int *write_fd);
int ngsq_gzip_pipe_close(ngsq_gzip_pipe *p);

#ifdef __cplusplus
}
#endif
#endif
