/* generate_args_drive.c -- the provider-string parser, the up-front checks and the inner-distance table builder of `ngs generate`
 * (ngs_amd/csrc/generate_args.cpp) on hostile input, linked with them into one program under -fsanitize=address,undefined and
 * run on the CPU by tests/test_generate.py.  Prints "parse ok", "check ok", "table ok"; any other output is a failure. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/ngsq_generate.h"

static int failures = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            failures++;                                               \
        }                                                             \
    } while (0)

static int parse(const char *s, ngsq_generate_provider *p, char *err, size_t err_cap) {
    /* the path buffer is exactly as long as the string needs at most: an overrun is the sanitizer's to find */
    char *path = malloc(strlen(s) + 1);
    const int rc = ngsq_generate_parse_provider(s, path, strlen(s) + 1, p, err, err_cap);
    if (rc == 0) EXPECT(p->path == path && strlen(path) <= strlen(s));
    free(path);
    return rc;
}

static void test_parse(void) {
    ngsq_generate_provider p;
    char err[600];
    static const struct { const char *s, *starts; } bad[] = {
        {"", "invalid format for reference genome sequence provider, please check the wiki for the correct format."},
        {"a.fa:1:2:3:4", "invalid format"},
        {"a.fa:1:2:3:4:5:6", "invalid format"},
        {":::::", "could not parse the error frequency for reference provider: :::::."},
        {"a.fa::2:3:4:5", "could not parse the error frequency"},
        {"a.fa:-1:2:3:4:5", "could not parse the error frequency"},
        {"a.fa:1.5:2:3:4:5", "could not parse the error frequency"},
        {"a.fa:18446744073709551616:2:3:4:5", "could not parse the error frequency"},
        {"a.fa:99999999999999999999999999999999:2:3:4:5", "could not parse the error frequency"},
        {"a.fa:1::3:4:5", "could not parse the mean for inner distance distribution for reference provider: a.fa:1::3:4:5."},
        {"a.fa:1:0x10:3:4:5", "could not parse the mean"},
        {"a.fa:1: 2:3:4:5", "could not parse the mean"},
        {"a.fa:1:2e:3:4:5", "could not parse the mean"},
        {"a.fa:1:.:3:4:5", "could not parse the mean"},
        {"a.fa:1:2:x:4:5", "could not parse the std deviation for inner distance distribution for reference provider: a.fa:1:2:x:4:5."},
        {"a.fa:1:2:3:4.0:5", "could not parse the read length for reference provider: a.fa:1:2:3:4.0:5."},
        {"a.fa:1:2:3::5", "could not parse the read length"},
        {"a.fa:1:2:3:4:", "could not parse the weight for reference provider: a.fa:1:2:3:4:."},
        {"a.fa:1:2:3:4:18446744073709551616", "could not parse the weight"},
    };
    for (size_t k = 0; k < sizeof bad / sizeof bad[0]; k++) {
        err[0] = 0;
        EXPECT(parse(bad[k].s, &p, err, sizeof err) != 0);
        if (strncmp(err, bad[k].starts, strlen(bad[k].starts)) != 0) {
            printf("FAILED: '%s' gave '%s'\n", bad[k].s, err);
            failures++;
        }
    }
    EXPECT(parse("dir/a.fa:+100:-2.5e1:inf:150:18446744073709551615", &p, err, sizeof err) == 0);
    EXPECT(p.error_freq == 100 && p.mu == -25.0 && isinf(p.sigma) && p.read_length == 150 && p.weight == UINT64_MAX);
    EXPECT(parse("a.fa:1:NaN:-Infinity:1:0", &p, err, sizeof err) == 0 && isnan(p.mu) && p.sigma < 0 && isinf(p.sigma));
    EXPECT(parse(":1:5.:.5:1:1", &p, err, sizeof err) == 0 && p.mu == 5.0 && p.sigma == 0.5); /* an empty path parses; opening it fails */
    /* a message longer than its buffer is cut, and the buffer stays terminated; no buffer at all is taken too */
    char tiny[8];
    memset(tiny, 'x', sizeof tiny);
    EXPECT(parse("a.fa:zzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzz:2:3:4:5", &p, tiny, sizeof tiny) != 0 && strlen(tiny) == sizeof tiny - 1);
    EXPECT(parse("a.fa:z:2:3:4:5", &p, NULL, 0) != 0);
    /* a path buffer that is too small is refused, not overrun */
    char small[4];
    EXPECT(ngsq_generate_parse_provider("long/path.fa:1:2:3:4:5", small, sizeof small, &p, err, sizeof err) != 0);
    /* a long string of colons and one of digits */
    char *many = malloc(100001);
    memset(many, ':', 100000);
    many[100000] = 0;
    EXPECT(parse(many, &p, err, sizeof err) != 0);
    memset(many, '9', 100000);
    many[4] = ':';
    EXPECT(parse(many, &p, err, sizeof err) != 0);
    free(many);
    puts(failures ? "parse FAILED" : "parse ok");
}

static int check(uint64_t ef, double mu, double sigma, uint64_t L, char *err, size_t cap) {
    ngsq_generate_provider p = {"x.fa", ef, mu, sigma, L, 1};
    return ngsq_generate_check_provider(&p, "x.fa", err, cap);
}

static void test_check(void) {
    const int before = failures;
    char err[1024];
    EXPECT(check(100, 0, 0, 150, err, sizeof err) == 0);
    EXPECT(check(0, 0, 0, 150, err, sizeof err) != 0 && strstr(err, "error frequency"));
    EXPECT(check(4294967296ull, 0, 0, 150, err, sizeof err) != 0);
    EXPECT(check(4294967295ull, 0, 0, 150, err, sizeof err) == 0);
    EXPECT(check(1, 0, 0, 0, err, sizeof err) != 0 && strstr(err, "read length"));
    EXPECT(check(1, 0, 0, UINT64_MAX, err, sizeof err) != 0);
    EXPECT(check(1, NAN, 1, 150, err, sizeof err) != 0);
    EXPECT(check(1, INFINITY, 1, 150, err, sizeof err) != 0);
    EXPECT(check(1, 0, NAN, 150, err, sizeof err) != 0 && strstr(err, "std deviation"));
    EXPECT(check(1, 0, INFINITY, 150, err, sizeof err) != 0);
    EXPECT(check(1, 0, -1, 150, err, sizeof err) != 0);
    EXPECT(check(1, 0, -0.0, 150, err, sizeof err) == 0);
    EXPECT(check(1, 0, 1e300, 150, err, sizeof err) == NGSQ_ERR_LIMIT);
    EXPECT(check(1, 1e300, 1, 150, err, sizeof err) == NGSQ_ERR_LIMIT);
    EXPECT(check(1, -1e300, 1, 150, err, sizeof err) == NGSQ_ERR_LIMIT);
    EXPECT(check(1, 0, 1e6, 150, err, sizeof err) == NGSQ_ERR_LIMIT);
    /* the lower bound: 2 L + lower >= L */
    EXPECT(check(1, -150, 0, 150, err, sizeof err) == 0);
    EXPECT(check(1, -151, 0, 150, err, sizeof err) != 0 && strstr(err, "fragment is too short for the specified read length"));
    EXPECT(check(1, -140, 4, 150, err, sizeof err) != 0); /* -140 - 12 */
    EXPECT(check(1, -140, 3, 150, err, sizeof err) == 0); /* -140 - 9 */
    char tiny[4];
    EXPECT(check(0, 0, 0, 150, tiny, sizeof tiny) != 0 && strlen(tiny) == 3);
    EXPECT(ngsq_generate_check_provider(NULL, "x", err, sizeof err) != 0);
    puts(failures == before ? "check ok" : "check FAILED");
}

static void test_table(void) {
    const int before = failures;
    char err[512];
    int64_t lower = 0;
    uint64_t n = 0;
    /* the size alone, then a table of exactly that size; one too small is filled as far as it goes */
    EXPECT(ngsq_generate_inner_table(10.3, 2.2, &lower, NULL, 0, &n, err, sizeof err) == 0 && lower == 4 && n == 14);
    uint64_t *t = malloc(14 * sizeof *t);
    EXPECT(ngsq_generate_inner_table(10.3, 2.2, &lower, t, 14, &n, err, sizeof err) == 0 && t[13] == UINT64_MAX);
    for (int k = 1; k < 14; k++) EXPECT(t[k] >= t[k - 1]);
    free(t);
    t = malloc(3 * sizeof *t);
    EXPECT(ngsq_generate_inner_table(10.3, 2.2, &lower, t, 3, &n, err, sizeof err) == 0 && n == 14 && t[2] < UINT64_MAX);
    free(t);
    /* sigma 0: one entry, trunc(mu) */
    uint64_t one = 0;
    EXPECT(ngsq_generate_inner_table(-2.7, 0, &lower, &one, 1, &n, err, sizeof err) == 0 && lower == -2 && n == 1 && one == UINT64_MAX);
    /* a table at the limit, one past it, and what cannot be one */
    const double at_limit = (NGSQ_GENERATE_MAX_TABLE - 1) / 6.0; /* floor(3 s) + ceil(3 s) + 1 entries around an integer mean */
    EXPECT(ngsq_generate_inner_table(0, floor(at_limit), &lower, NULL, 0, &n, err, sizeof err) == 0 && n <= NGSQ_GENERATE_MAX_TABLE);
    t = malloc(n * sizeof *t);
    const uint64_t cap = n;
    EXPECT(ngsq_generate_inner_table(0, floor(at_limit), &lower, t, cap, &n, err, sizeof err) == 0 && n == cap && t[n - 1] == UINT64_MAX);
    for (uint64_t k = 1; k < n; k++)
        if (t[k] < t[k - 1]) {
            EXPECT(!"the table decreases");
            break;
        }
    free(t);
    EXPECT(ngsq_generate_inner_table(0, 200000, &lower, NULL, 0, &n, err, sizeof err) == NGSQ_ERR_LIMIT);
    EXPECT(ngsq_generate_inner_table(0, 1e308, &lower, NULL, 0, &n, err, sizeof err) == NGSQ_ERR_LIMIT);
    EXPECT(ngsq_generate_inner_table(1e19, 1, &lower, NULL, 0, &n, err, sizeof err) == NGSQ_ERR_LIMIT);
    EXPECT(ngsq_generate_inner_table(NAN, 1, &lower, NULL, 0, &n, err, sizeof err) != 0);
    EXPECT(ngsq_generate_inner_table(0, NAN, &lower, NULL, 0, &n, err, sizeof err) != 0);
    EXPECT(ngsq_generate_inner_table(0, INFINITY, &lower, NULL, 0, &n, err, sizeof err) != 0);
    EXPECT(ngsq_generate_inner_table(0, -1, &lower, NULL, 0, &n, NULL, 0) != 0);
    EXPECT(ngsq_generate_inner_table(0, 1, NULL, NULL, 0, &n, err, sizeof err) != 0);
    /* a tiny sigma far from the edges: every threshold is 0 or the maximum, and the order holds */
    uint64_t few[8];
    EXPECT(ngsq_generate_inner_table(0.2, 1e-9, &lower, few, 8, &n, err, sizeof err) == 0 && n == 2 && lower == 0);
    /* the draw is a pure function */
    EXPECT(ngsq_generate_draw(1, 2, 3, 4) == ngsq_generate_draw(1, 2, 3, 4) && ngsq_generate_draw(1, 2, 3, 4) != ngsq_generate_draw(1, 2, 3, 5));
    puts(failures == before ? "table ok" : "table FAILED");
}

int main(void) {
    test_parse();
    test_check();
    test_table();
    return failures ? 1 : 0;
}
