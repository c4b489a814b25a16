/* view_query.h -- the host side of a `ngs view` query: the region grammar and the chunk query over
 * the bytes of a BAI.  Plain functions over caller memory, no file, no GPU, no other part of the library: view.cpp wraps them
 * into ngsq_bam_query_chunks, and tests/c/view_query_drive.c feeds them hostile input under the sanitizers. */
#ifndef NGSQ_VIEW_QUERY_H
#define NGSQ_VIEW_QUERY_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/ngsq_view.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { NGSQ_VQ_OK = 0, NGSQ_VQ_PARSE = 1, NGSQ_VQ_NAME = 2, NGSQ_VQ_INDEX = 3 };

/* "name", "name:S", "name:S-E": split at the last ':'; when what follows parses as S or S-E (decimal digits only, at most
 * 18 of them, S >= 1, E >= S) the name is what stands in front, otherwise the whole string.  NGSQ_VQ_PARSE: an empty query;
 * NGSQ_VQ_NAME: the name is none of names[0, n_refs).  err receives the message (always NUL-terminated when err_cap > 0). */
int ngsq_vq_parse(const char *query, const char *const *names, uint32_t n_refs, uint32_t *ref_id, uint64_t *start, uint64_t *end,
                  char *err, size_t err_cap);

/* The merged chunks of sequence ref_id for the 1-based interval [start, end] in the index bai[0, bai_len): the whole index is
 * walked and must be well-formed (SAM specification 5.2).  chunks[0, min(*n, cap)) are filled, *n counts all of them. */
int ngsq_vq_chunks(const uint8_t *bai, size_t bai_len, uint32_t ref_id, uint64_t start, uint64_t end, ngsq_view_chunk *chunks,
                   uint64_t cap, uint64_t *n, char *err, size_t err_cap);

#ifdef __cplusplus
}
#endif
#endif
