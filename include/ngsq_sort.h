/*
 * ngsq_sort.h -- the sort of `ngs convert --sort coordinate` alone: a stable LSD radix sort of 64-bit
 * keys on the GPU, 8-bit digits, host memory in and out.  A pass whose digit is the same in every key is skipped.
 *
 * Messages: ngsq_sort_last_error() (per thread).
 */
#ifndef NGSQ_SORT_H
#define NGSQ_SORT_H

#include "ngsq.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ngsq_sort_report {
    uint32_t passes_run, passes_skipped; /* of the eight digits */
    double sort_ms;                      /* GPU time: histogram, passes, the identity when no pass runs (copies not counted) */
    double total_ms;                     /* wall clock */
} ngsq_sort_report;

/* perm[i] = the input index of the i-th key in ascending order; equal keys keep input order.  n from 0 to 2^32 - 1, more is
 * NGSQ_ERR_LIMIT.  n == 0 needs no device.  rep may be NULL. */
int ngsq_sort_u64_device(int device, const uint64_t *keys, uint64_t n, uint32_t *perm, ngsq_sort_report *rep);
/* keys one workgroup ranks at a time: tests place their edges by it */
uint32_t ngsq_sort_tile_keys(void);
/* Device bytes `ngs convert --sort coordinate` counts per record against its budget (ngsq_bamsort.h): beside a resident record's
 * own bytes (address, length, key, the sort's arrays, the sorted offset: 48), and per record of the survey of a file sorted in
 * rounds (key, length, the sort's arrays, its share of the pass table).  Tests and models read them here. */
uint64_t ngsq_sort_resident_bytes_per_record(void);
uint64_t ngsq_sort_survey_bytes_per_record(void);
const char *ngsq_sort_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
