/* view_query_drive.c -- hostile input for the host side of a `ngs view` query (ngs_amd/csrc/view_query.h): the region grammar
 * and the chunk query over the bytes of a BAI.  Stand-alone: tests/test_view.py compiles this file and view_query.cpp with
 * -fsanitize=address,undefined, links the two and runs the program; a sanitizer report or a failed check ends it non-zero.
 * Every index is handed over in a heap block of its exact size, so that one byte read past its end is seen. */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../ngs_amd/csrc/view_query.h"

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #x); \
            exit(1);                                                    \
        }                                                               \
    } while (0)

static unsigned char buf[1 << 16];
static size_t len;

static void p32(uint32_t v) {
    for (int k = 0; k < 4; k++) buf[len++] = (unsigned char)(v >> (8 * k));
}
static void p64(uint64_t v) {
    p32((uint32_t)v);
    p32((uint32_t)(v >> 32));
}

/* the chunk query on an exact-size copy of buf[0, n) */
static int chunks_of(size_t n, uint32_t ref, uint64_t s, uint64_t e, ngsq_view_chunk *out, uint64_t cap, uint64_t *got) {
    char err[64]; /* (shorter than some messages: they must be cut, not overrun) */
    unsigned char *copy = (unsigned char *)malloc(n ? n : 1);
    CHECK(copy);
    memcpy(copy, buf, n);
    const int rc = ngsq_vq_chunks(n ? copy : NULL, n, ref, s, e, out, cap, got, err, sizeof err);
    free(copy);
    if (rc != NGSQ_VQ_OK) CHECK(rc == NGSQ_VQ_INDEX && !strncmp(err, "reading BAM index: ", 19));
    return rc;
}

static void grammar(void) {
    static const char *const names[] = {"chr1", "HLA-A*01:01", "HLA-A*01", "", "chr1:0"};
    static const struct {
        const char *q;
        int rc;
        uint32_t ref;
        uint64_t s, e;
    } T[] = {
        {"chr1", NGSQ_VQ_OK, 0, 1, NGSQ_VIEW_END_MAX},
        {"chr1:5", NGSQ_VQ_OK, 0, 5, NGSQ_VIEW_END_MAX},
        {"chr1:5-9", NGSQ_VQ_OK, 0, 5, 9},
        {"chr1:0", NGSQ_VQ_OK, 4, 1, NGSQ_VIEW_END_MAX}, /* 0 is no start: the whole string is the name (a sequence of this table) */
        {"chr1:9-5", NGSQ_VQ_NAME, 0, 0, 0},
        {"HLA-A*01:01", NGSQ_VQ_OK, 2, 1, NGSQ_VIEW_END_MAX}, /* "01" reads as a start */
        {"HLA-A*01:01:5-9", NGSQ_VQ_OK, 1, 5, 9},
        {"", NGSQ_VQ_PARSE, 0, 0, 0},
        {":7", NGSQ_VQ_OK, 3, 7, NGSQ_VIEW_END_MAX}, /* the empty name, when the header has it */
        {":", NGSQ_VQ_NAME, 0, 0, 0},
        {"chr1:", NGSQ_VQ_NAME, 0, 0, 0},
        {"chr1:-5", NGSQ_VQ_NAME, 0, 0, 0},
        {"chr1:5-", NGSQ_VQ_NAME, 0, 0, 0},
        {"chr1:5-9-11", NGSQ_VQ_NAME, 0, 0, 0},
        {"chr1:+5", NGSQ_VQ_NAME, 0, 0, 0},
        {"chr1:1,000", NGSQ_VQ_NAME, 0, 0, 0},
        {"chr1:999999999999999999", NGSQ_VQ_OK, 0, 999999999999999999ull, NGSQ_VIEW_END_MAX},
        {"chr1:1000000000000000000", NGSQ_VQ_NAME, 0, 0, 0}, /* nineteen digits: no number of this grammar */
        {"chr1:99999999999999999999999999999999999999", NGSQ_VQ_NAME, 0, 0, 0},
        {"chr2", NGSQ_VQ_NAME, 0, 0, 0},
    };
    for (size_t k = 0; k < sizeof T / sizeof T[0]; k++) {
        uint32_t ref = 77;
        uint64_t s = 77, e = 77;
        char err[40] = "";
        char *q = strdup(T[k].q); /* exact size on the heap */
        CHECK(q);
        const int rc = ngsq_vq_parse(q, names, 5, &ref, &s, &e, err, sizeof err);
        free(q);
        if (rc != T[k].rc) fprintf(stderr, "query \"%s\": %d, want %d\n", T[k].q, rc, T[k].rc);
        CHECK(rc == T[k].rc);
        if (rc == NGSQ_VQ_OK) CHECK(ref == T[k].ref && s == T[k].s && e == T[k].e);
        else CHECK(strlen(err) > 0 && strlen(err) < sizeof err);
    }
    /* a name longer than any message buffer, no names at all, no message buffer */
    char *big = (char *)malloc(100001);
    CHECK(big);
    memset(big, 'x', 100000);
    big[100000] = 0;
    uint32_t ref;
    uint64_t s, e;
    char err[16];
    CHECK(ngsq_vq_parse(big, names, 5, &ref, &s, &e, err, sizeof err) == NGSQ_VQ_NAME && strlen(err) == 15);
    CHECK(ngsq_vq_parse("chr1", NULL, 0, &ref, &s, &e, NULL, 0) == NGSQ_VQ_NAME);
    free(big);
    printf("grammar ok\n");
}

/* two sequences: the first with four bins (one of them without chunks, one the pseudo-bin) and a linear index of two
 * windows, the second with nothing */
static void build_index(void) {
    len = 0;
    memcpy(buf, "BAI\1", 4);
    len = 4;
    p32(2);
    p32(4);
    p32(4681), p32(2), p64(0x10000), p64(0x20000), p64(0x20000), p64(0x28000); /* window 0: two chunks that touch */
    p32(4682), p32(0);                                                         /* window 1: a bin with zero chunks */
    p32(0), p32(2), p64(0x90000), p64(0xA0000), p64(0x30000), p64(0x30000);    /* bin 0: out of order, one empty */
    p32(37450), p32(2), p64(1), p64(2), p64(3), p64(4);
    p32(2), p64(0x10000), p64(0x28000);
    p32(0), p32(0);
    p64(5);
}

static void index_cases(void) {
    ngsq_view_chunk c[8];
    uint64_t n = 0;
    build_index();
    const size_t full = len;
    /* the whole sequence: the touching chunks merge, bin 0's chunk follows, the empty chunk and the pseudo-bin are dropped */
    CHECK(chunks_of(full, 0, 1, NGSQ_VIEW_END_MAX, c, 8, &n) == NGSQ_VQ_OK && n == 2);
    CHECK(c[0].begin == 0x10000 && c[0].end == 0x28000 && c[1].begin == 0x90000 && c[1].end == 0xA0000);
    /* window 1: the linear entry 0x28000 drops the chunks of window 0 -- they are not its bins anyway; bin 0 stays */
    CHECK(chunks_of(full, 0, 16385, 16385, c, 8, &n) == NGSQ_VQ_OK && n == 1 && c[0].begin == 0x90000);
    /* a window past the linear index: min_offset 0 */
    CHECK(chunks_of(full, 0, 5 * 16384 + 1, 6 * 16384, c, 8, &n) == NGSQ_VQ_OK && n == 1);
    /* nothing: the second sequence, an interval past 2^29, an inverted one */
    CHECK(chunks_of(full, 1, 1, NGSQ_VIEW_END_MAX, c, 8, &n) == NGSQ_VQ_OK && n == 0);
    CHECK(chunks_of(full, 0, NGSQ_VIEW_END_MAX + 1, ~(uint64_t)0, c, 8, &n) == NGSQ_VQ_OK && n == 0);
    CHECK(chunks_of(full, 0, 9, 5, c, 8, &n) == NGSQ_VQ_OK && n == 0);
    CHECK(chunks_of(full, 0, 0, 0, c, 8, &n) == NGSQ_VQ_OK && n == 0);
    /* a sequence the index does not have */
    CHECK(chunks_of(full, 2, 1, 10, c, 8, &n) == NGSQ_VQ_INDEX);
    CHECK(chunks_of(full, 0xFFFFFFFFu, 1, 10, c, 8, &n) == NGSQ_VQ_INDEX);
    /* fewer places than chunks: the count is whole, nothing is written behind cap */
    c[1].begin = 42;
    CHECK(chunks_of(full, 0, 1, NGSQ_VIEW_END_MAX, c, 1, &n) == NGSQ_VQ_OK && n == 2 && c[1].begin == 42);
    CHECK(chunks_of(full, 0, 1, NGSQ_VIEW_END_MAX, NULL, 0, &n) == NGSQ_VQ_OK && n == 2);
    /* without n_no_coor; with trailing bytes */
    CHECK(chunks_of(full - 8, 0, 1, 100, c, 8, &n) == NGSQ_VQ_OK && n == 2);
    CHECK(chunks_of(full - 4, 0, 1, 100, c, 8, &n) == NGSQ_VQ_INDEX);
    /* truncated at every length */
    for (size_t k = 0; k < full - 8; k++) CHECK(chunks_of(k, 0, 1, NGSQ_VIEW_END_MAX, c, 8, &n) == NGSQ_VQ_INDEX);
    printf("index ok\n");
    /* counts that promise more than the bytes hold */
    static const size_t AT[] = {4, 8, 16, 12 + 8 + 32 + 4};
    for (size_t k = 0; k < sizeof AT / sizeof AT[0]; k++)
        for (int v = 0; v < 3; v++) {
            build_index();
            const uint32_t lie = v == 0 ? 0xFFFFFFFFu : v == 1 ? 0x7FFFFFFFu : 0x10000000u;
            for (int j = 0; j < 4; j++) buf[AT[k] + j] = (unsigned char)(lie >> (8 * j));
            CHECK(chunks_of(len, 0, 1, NGSQ_VIEW_END_MAX, c, 8, &n) == NGSQ_VQ_INDEX);
        }
    /* n_intv that lies about the linear index */
    build_index();
    {
        const size_t at = 8 + 4 + (8 + 32) + 8 + (8 + 32) + (8 + 32);
        CHECK(buf[at] == 2);
        buf[at] = 3;
        CHECK(chunks_of(len, 0, 40000, 40001, c, 8, &n) == NGSQ_VQ_INDEX);
        buf[at] = 0xFF, buf[at + 3] = 0xFF;
        CHECK(chunks_of(len, 0, 40000, 40001, c, 8, &n) == NGSQ_VQ_INDEX);
    }
    /* bytes of every value behind a good magic */
    srand(7);
    for (int t = 0; t < 2000; t++) {
        len = 8 + (size_t)(rand() % 200);
        for (size_t k = 4; k < len; k++) buf[k] = (unsigned char)(rand() % 3 ? rand() % 4 : rand());
        memcpy(buf, "BAI\1", 4);
        buf[4] = (unsigned char)(rand() % 3), buf[5] = buf[6] = buf[7] = 0;
        (void)chunks_of(len, (uint32_t)(rand() % 2), 1 + (uint64_t)(rand() % 100000), 1 + (uint64_t)(rand() % 200000), c, 8, &n);
    }
    len = 0;
    CHECK(chunks_of(0, 0, 1, 2, c, 8, &n) == NGSQ_VQ_INDEX);
    printf("hostile ok\n");
}

int main(void) {
    grammar();
    index_cases();
    return 0;
}
