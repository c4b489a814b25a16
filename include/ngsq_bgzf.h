/*
 * ngsq_bgzf.h -- BGZF written on the GPU: the device DEFLATE encoder, the counterpart of
 * ngsq_bgzf_inflate_device (ngsq_bam.h).  The input is cut into blocks of NGSQ_BGZF_BLOCK_INPUT bytes; each becomes one
 * complete BGZF block (SAM/BAM specification 4.1) with a dynamic-Huffman DEFLATE payload, or a stored one when that is not
 * smaller.  The output bytes depend on the input bytes and the context's effort (below) alone.
 *
 * Messages: ngsq_last_error(ctx).
 */
#ifndef NGSQ_BGZF_H
#define NGSQ_BGZF_H

#include "ngsq.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NGSQ_BGZF_BLOCK_INPUT 65280u /* input bytes per block (htslib's): a stored block always fits BSIZE */
#define NGSQ_BGZF_EOF 1u             /* flags: append the 28-byte EOF block */

/* Most bytes ngsq_bgzf_deflate_device writes for in_len input bytes: every block stored (31 bytes around its input), and
 * the EOF block with NGSQ_BGZF_EOF.  Host, pure. */
uint64_t ngsq_bgzf_deflate_bound(uint64_t in_len, uint32_t flags);

typedef struct ngsq_bgzf_deflate_report {
    uint64_t blocks, stored_blocks, in_bytes, out_bytes, tokens, matches; /* tokens, matches: of the dynamic blocks */
    double deflate_ms, crc_ms, pack_ms, copy_ms, total_ms; /* GPU time of the encoder, the CRC, scan and pack, the two copies; wall clock */
} ngsq_bgzf_deflate_report;

/* Host memory in, host memory out.  *out_len = the bytes of the BGZF stream, also when out_cap is too small: that case
 * returns NGSQ_ERR_LIMIT and writes nothing to out.  in_len == 0 with NGSQ_BGZF_EOF gives the EOF block alone (no GPU
 * work); without the flag, nothing.  rep may be NULL. */
int ngsq_bgzf_deflate_device(ngsq_ctx *ctx, const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                             uint32_t flags, ngsq_bgzf_deflate_report *rep);

/* The encoder's effort, a property of the context: every encoder launch made for the context reads it -- the call above, the BAM
 * writers of ngsq_samtext.h and ngsq_bamsort.h, and ngsq_generate_write_bgzf through the context given to ngsq_generate_load.
 * NORMAL is the encoder of a context that was never told.  HIGH searches harder for matches (candidates inside a position's own
 * tile, several candidates per position, a lazy parse) and costs encoder time; no block is larger than at NORMAL.  The output
 * bytes depend on the input bytes and the effort alone. */
#define NGSQ_BGZF_EFFORT_NORMAL 0u
#define NGSQ_BGZF_EFFORT_HIGH 1u
/* NGSQ_ERR_INVALID_ARGUMENT, with a message, for another value or a null context. */
int ngsq_bgzf_set_effort(ngsq_ctx *ctx, uint32_t effort);
uint32_t ngsq_bgzf_effort(const ngsq_ctx *ctx); /* (a null context: NORMAL) */
/* Match candidates a position looks at beside the one at distance 1: 1 at NORMAL, the length of the hash chain walked at HIGH;
 * 0 for another value.  Host, pure. */
uint32_t ngsq_bgzf_effort_candidates(uint32_t effort);

#ifdef __cplusplus
}
#endif
#endif
