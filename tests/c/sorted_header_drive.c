/* sorted_header_drive.c -- ngsq_sam_sorted_header (include/ngsq_samtext.h, ngs_amd/csrc/samsort_header.cpp) on hostile input.
 * Stand-alone: tests/test_sam_sort.py compiles this file and samsort_header.cpp with -fsanitize=address,undefined, links the two
 * and runs the program; a sanitizer report or a failed check ends it non-zero.  Every text is handed over in a heap block of its
 * exact size, without a NUL behind it, and every output buffer has exactly `cap` bytes, so that one byte read or written past
 * an end is seen. */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/ngsq_samtext.h"

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #x); \
            exit(1);                                                    \
        }                                                               \
    } while (0)

/* the rewrite of text[0, n) into a block of exactly the size it takes; *out_n = that size */
static char *rewrite(const char *text, size_t n, size_t *out_n) {
    char *in = (char *)malloc(n ? n : 1);
    CHECK(in);
    memcpy(in, text, n);
    size_t need = 0;
    CHECK(ngsq_sam_sorted_header(n ? in : NULL, n, NULL, 0, &need) == (need ? NGSQ_ERR_BUFFER_TOO_SMALL : NGSQ_OK));
    char *out = (char *)malloc(need ? need : 1);
    CHECK(out);
    if (need > 1) { /* one byte short: refused, the size reported again */
        size_t again = 0;
        CHECK(ngsq_sam_sorted_header(in, n, out, need - 1, &again) == NGSQ_ERR_BUFFER_TOO_SMALL && again == need);
    }
    CHECK(ngsq_sam_sorted_header(n ? in : NULL, n, out, need, out_n) == NGSQ_OK && *out_n == need);
    free(in);
    return out;
}

static void expect(const char *text, const char *want) {
    size_t n = 0;
    char *got = rewrite(text, strlen(text), &n);
    if (n != strlen(want) || memcmp(got, want, n)) {
        fprintf(stderr, "rewrite of [%s]: got [%.*s], want [%s]\n", text, (int)n, got, want);
        exit(1);
    }
    free(got);
}

int main(void) {
    expect("", "@HD\tVN:1.6\tSO:coordinate\n");
    expect("@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:a\tLN:5\n", "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:a\tLN:5\n");
    expect("@HD\tVN:1.6\tSO:queryname\tSS:queryname:natural\n", "@HD\tVN:1.6\tSO:coordinate\n");
    expect("@HD\tVN:1.6\tSO:coordinate\tSS:coordinate:x\n", "@HD\tVN:1.6\tSO:coordinate\tSS:coordinate:x\n");
    expect("@HD\tVN:1.6\n", "@HD\tVN:1.6\tSO:coordinate\n");
    expect("@SQ\tSN:a\tLN:5\n@HD\tVN:1.5\tSO:unsorted\n", "@SQ\tSN:a\tLN:5\n@HD\tVN:1.5\tSO:coordinate\n");
    expect("@SQ\tSN:a\tLN:5\n", "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:a\tLN:5\n");
    /* fields cut short at the end of the text: nothing is read behind it */
    expect("@HD", "@HD\tSO:coordinate");
    expect("@HD\t", "@HD\t\tSO:coordinate");
    expect("@HD\tSO", "@HD\tSO\tSO:coordinate");
    expect("@HD\tSO:", "@HD\tSO:coordinate");
    expect("@HD\tSS", "@HD\tSS\tSO:coordinate");
    expect("@HD\tSS:", "@HD\tSO:coordinate");
    expect("@HD\tSS:coordinate", "@HD\tSO:coordinate");
    expect("@HD\tSS:coordinate:", "@HD\tSS:coordinate:\tSO:coordinate");
    expect("@CO\tx\n@HD", "@CO\tx\n@HD\tSO:coordinate");
    printf("cases ok\n");
    /* every prefix of a longer header, and every tail */
    const char *full = "@CO\tfirst\n@HD\tVN:1.6\tGO:none\tSS:unsorted:x\tSO:unknown\tSS:coordinate:y\tSO:again\n@SQ\tSN:chr1\tLN:1000\n@PG\tID:p\tSO:no\n";
    const size_t len = strlen(full);
    for (size_t k = 0; k <= len; k++) {
        size_t n = 0;
        char *a = rewrite(full, k, &n);
        CHECK(n + 40 >= k); /* (at most its two SS fields go) */
        free(a);
        char *b = rewrite(full + k, len - k, &n);
        CHECK(n + 40 >= len - k);
        free(b);
    }
    printf("prefixes ok\n");
    /* bytes that are no text */
    unsigned state = 12345;
    char junk[512];
    for (int round = 0; round < 2000; round++) {
        const size_t n = (size_t)(round % 512);
        for (size_t k = 0; k < n; k++) {
            state = state * 1103515245u + 12345u;
            const unsigned r = (state >> 16) & 15;
            junk[k] = r < 3 ? '\t' : r < 5 ? '\n' : r < 7 ? '@' : r < 8 ? 'H' : r < 9 ? 'D' : r < 10 ? 'S' : r < 11 ? 'O' : r < 12 ? ':' : (char)(state >> 8);
        }
        size_t got = 0;
        char *a = rewrite(junk, n, &got);
        free(a);
    }
    printf("hostile ok\n");
    return 0;
}
