/*
 * ngsq_bgzf.h -- BGZF written on the GPU: the device DEFLATE encoder, the counterpart of
 * ngsq_bgzf_inflate_device (ngsq_bam.h).  The input is cut into blocks of NGSQ_BGZF_BLOCK_INPUT bytes; each becomes one
 * complete BGZF block (SAM/BAM specification 4.1) with a dynamic-Huffman DEFLATE payload, or a stored one when that is not
 * smaller.  The output bytes depend on the input bytes alone.
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

#ifdef __cplusplus
}
#endif
#endif
