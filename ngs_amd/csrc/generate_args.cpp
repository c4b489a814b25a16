// generate_args.cpp -- the host side of `ngs generate` that needs neither a file nor a GPU (include/ngsq_generate.h; DESIGN.md
// section 16): the provider string, the up-front refusals, the inner-distance table, the draw function.  Plain functions over
// caller memory and no other part of the library: tests/c/generate_args_drive.c feeds them hostile input under the sanitizers.
#include <errno.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/ngsq_generate.h"
#include "generate_draw.h"

namespace {

int say(int code, char *err, size_t cap, const char *fmt, ...) {
    if (err && cap) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, cap, fmt, ap);
        va_end(ap);
    }
    return code;
}

// str::parse::<usize>: an optional '+', then decimal digits only; no overflow
bool parse_usize(const std::string &t, uint64_t *out) {
    size_t i = !t.empty() && t[0] == '+' ? 1 : 0;
    if (i >= t.size()) return false;
    uint64_t v = 0;
    for (; i < t.size(); i++) {
        if (t[i] < '0' || t[i] > '9') return false;
        const uint64_t d = (uint64_t)(t[i] - '0');
        if (v > (UINT64_MAX - d) / 10) return false;
        v = v * 10 + d;
    }
    *out = v;
    return true;
}

bool word_is(const std::string &t, size_t at, const char *w) {
    const size_t n = strlen(w);
    if (t.size() - at != n) return false;
    for (size_t k = 0; k < n; k++)
        if (tolower((unsigned char)t[at + k]) != w[k]) return false;
    return true;
}

// str::parse::<f64>: [+-] (inf | infinity | nan | digits [. digits] | . digits) [e [+-] digits]; nothing around it
bool parse_f64(const std::string &t, double *out) {
    size_t i = !t.empty() && (t[0] == '+' || t[0] == '-') ? 1 : 0;
    if (i >= t.size()) return false;
    if (word_is(t, i, "inf") || word_is(t, i, "infinity")) {
        *out = t[0] == '-' ? -INFINITY : INFINITY;
        return true;
    }
    if (word_is(t, i, "nan")) {
        *out = NAN;
        return true;
    }
    size_t digits = 0;
    while (i < t.size() && t[i] >= '0' && t[i] <= '9') i++, digits++;
    if (i < t.size() && t[i] == '.') {
        i++;
        while (i < t.size() && t[i] >= '0' && t[i] <= '9') i++, digits++;
    }
    if (!digits) return false;
    if (i < t.size() && (t[i] == 'e' || t[i] == 'E')) {
        i++;
        if (i < t.size() && (t[i] == '+' || t[i] == '-')) i++;
        size_t ed = 0;
        while (i < t.size() && t[i] >= '0' && t[i] <= '9') i++, ed++;
        if (!ed) return false;
    }
    if (i != t.size()) return false;
    *out = strtod(t.c_str(), nullptr); // (the grammar above is a subset of strtod's: the whole string is consumed)
    return true;
}

constexpr double BOUND_LIMIT = 1099511627776.0; // 2^40

// lower and upper of reference_provider.rs:321-326, as doubles (`as i64` truncates)
void inner_bounds(double mu, double sigma, double *lo, double *hi) {
    *lo = trunc(mu - floor(3.0 * sigma));
    *hi = trunc(mu + ceil(3.0 * sigma));
}

int check_distribution(double mu, double sigma, double *lo, double *hi, char *err, size_t cap) {
    if (!isfinite(mu)) return say(NGSQ_ERR_INVALID_ARGUMENT, err, cap, "the mean of the inner distance distribution must be finite");
    if (!isfinite(sigma) || sigma < 0)
        return say(NGSQ_ERR_INVALID_ARGUMENT, err, cap, "the std deviation of the inner distance distribution must be finite and not negative");
    inner_bounds(mu, sigma, lo, hi);
    if (!(fabs(*lo) <= BOUND_LIMIT) || !(fabs(*hi) <= BOUND_LIMIT))
        return say(NGSQ_ERR_LIMIT, err, cap, "the inner distance distribution reaches beyond +-2^40");
    if (*hi - *lo + 1 > (double)NGSQ_GENERATE_MAX_TABLE)
        return say(NGSQ_ERR_LIMIT, err, cap, "the inner distance distribution spans %.0f integers; this build takes %u", *hi - *lo + 1,
                   NGSQ_GENERATE_MAX_TABLE);
    return NGSQ_OK;
}

} // namespace

extern "C" {

uint64_t ngsq_generate_draw(uint64_t seed, uint64_t pair, uint32_t purpose, uint32_t index) {
    return ngsq::gen_draw(ngsq::gen_pair_key(seed, pair), purpose, index);
}

int ngsq_generate_parse_provider(const char *s, char *path, size_t path_cap, ngsq_generate_provider *out, char *err, size_t err_cap) {
    if (!s || !path || !out) return say(NGSQ_ERR_INVALID_ARGUMENT, err, err_cap, "null argument");
    std::vector<std::string> parts(1);
    for (const char *p = s; *p; p++) {
        if (*p == ':') parts.emplace_back();
        else parts.back() += *p;
    }
    if (parts.size() != 6)
        return say(NGSQ_ERR_INVALID_ARGUMENT, err, err_cap,
                   "invalid format for reference genome sequence provider, please check the wiki for the correct format.");
    ngsq_generate_provider p{};
    if (!parse_usize(parts[1], &p.error_freq))
        return say(NGSQ_ERR_INVALID_ARGUMENT, err, err_cap, "could not parse the error frequency for reference provider: %s.", s);
    if (!parse_f64(parts[2], &p.mu))
        return say(NGSQ_ERR_INVALID_ARGUMENT, err, err_cap, "could not parse the mean for inner distance distribution for reference provider: %s.", s);
    if (!parse_f64(parts[3], &p.sigma))
        return say(NGSQ_ERR_INVALID_ARGUMENT, err, err_cap, "could not parse the std deviation for inner distance distribution for reference provider: %s.", s);
    if (!parse_usize(parts[4], &p.read_length))
        return say(NGSQ_ERR_INVALID_ARGUMENT, err, err_cap, "could not parse the read length for reference provider: %s.", s);
    if (!parse_usize(parts[5], &p.weight))
        return say(NGSQ_ERR_INVALID_ARGUMENT, err, err_cap, "could not parse the weight for reference provider: %s.", s);
    if (parts[0].size() + 1 > path_cap) return say(NGSQ_ERR_LIMIT, err, err_cap, "the path of the reference provider is longer than %zu bytes", path_cap);
    memcpy(path, parts[0].c_str(), parts[0].size() + 1);
    p.path = path;
    *out = p;
    return NGSQ_OK;
}

int ngsq_generate_check_provider(const ngsq_generate_provider *p, const char *name, char *err, size_t err_cap) {
    if (!p) return say(NGSQ_ERR_INVALID_ARGUMENT, err, err_cap, "null argument");
    if (!name) name = "";
    if (p->error_freq == 0)
        return say(NGSQ_ERR_INVALID_ARGUMENT, err, err_cap, "reference provider %s: the error frequency must be at least 1 (one base in N is substituted)", name);
    if (p->error_freq > 0xFFFFFFFFull)
        return say(NGSQ_ERR_INVALID_ARGUMENT, err, err_cap, "reference provider %s: the error frequency must be below 2^32", name);
    if (p->read_length == 0) return say(NGSQ_ERR_INVALID_ARGUMENT, err, err_cap, "reference provider %s: the read length must be at least 1", name);
    if (p->read_length > NGSQ_GENERATE_MAX_READ_LENGTH)
        return say(NGSQ_ERR_LIMIT, err, err_cap, "reference provider %s: this build takes read lengths up to %u", name, NGSQ_GENERATE_MAX_READ_LENGTH);
    double lo, hi;
    char why[256];
    if (const int rc = check_distribution(p->mu, p->sigma, &lo, &hi, why, sizeof why)) return say(rc, err, err_cap, "reference provider %s: %s", name, why);
    // a fragment of 2 L + lower bases must hold a read (reference_provider.rs:366-384 panics with this sentence when one is drawn)
    if (2.0 * (double)p->read_length + lo < (double)p->read_length)
        return say(NGSQ_ERR_INVALID_ARGUMENT, err, err_cap,
                   "reference provider %s: an inner distance of %.0f can be drawn, and with it a fragment is too short for the specified read length. "
                   "This usually means you need to increase the specified inner distance or reduce the standard deviation for genome %s such that "
                   "fragments this short cannot be generated.",
                   name, lo, name);
    return NGSQ_OK;
}

int ngsq_generate_inner_table(double mu, double sigma, int64_t *lower, uint64_t *table, uint64_t cap, uint64_t *n, char *err, size_t err_cap) {
    if (!lower || !n) return say(NGSQ_ERR_INVALID_ARGUMENT, err, err_cap, "null argument");
    double lo, hi;
    if (const int rc = check_distribution(mu, sigma, &lo, &hi, err, err_cap)) return rc;
    const uint64_t cnt = (uint64_t)(hi - lo) + 1;
    *lower = (int64_t)lo;
    *n = cnt;
    if (!table) return NGSQ_OK;
    uint64_t prev = 0;
    for (uint64_t j = 0; j < cnt && j < cap; j++) {
        uint64_t t = UINT64_MAX;
        if (j + 1 < cnt) {
            // P(round(X) <= lower + j) = P(X < lower + j + 0.5): the lower tail folds onto entry 0, the upper one onto the last
            const double edge = lo + (double)j + 0.5;
            double cdf;
            if (sigma > 0) cdf = 0.5 * (1.0 + erf((edge - mu) / (sigma * 1.4142135623730951)));
            else cdf = mu < edge ? 1.0 : 0.0; // (sigma == 0 has one entry; kept for a caller's own bounds)
            const double scaled = cdf * 18446744073709551616.0;
            t = scaled >= 18446744073709551615.0 ? UINT64_MAX : scaled <= 0 ? 0 : (uint64_t)scaled;
            if (t < prev) t = prev;
        }
        table[j] = t;
        prev = t;
    }
    return NGSQ_OK;
}

} // extern "C"
