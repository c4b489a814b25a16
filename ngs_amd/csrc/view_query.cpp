// view_query.cpp -- the region grammar and the chunk query of `ngs view` (view_query.h).  Host only.
#include "view_query.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace {

int vq_fail(int code, char *err, size_t cap, const char *fmt, ...) __attribute__((format(printf, 4, 5)));
int vq_fail(int code, char *err, size_t cap, const char *fmt, ...) {
    if (err && cap) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, cap, fmt, ap);
        va_end(ap);
    }
    return code;
}

// decimal digits only, 1 to 18 of them
bool parse_number(const char *p, size_t n, uint64_t *out) {
    if (n < 1 || n > 18) return false;
    uint64_t v = 0;
    for (size_t k = 0; k < n; k++) {
        if (p[k] < '0' || p[k] > '9') return false;
        v = v * 10 + (uint64_t)(p[k] - '0');
    }
    *out = v;
    return true;
}

// "S" or "S-E"
bool parse_interval(const char *p, size_t n, uint64_t *start, uint64_t *end) {
    const char *dash = static_cast<const char *>(memchr(p, '-', n));
    uint64_t s = 0, e = NGSQ_VIEW_END_MAX;
    if (dash) {
        if (!parse_number(p, (size_t)(dash - p), &s) || !parse_number(dash + 1, n - (size_t)(dash - p) - 1, &e)) return false;
        if (e < s) return false;
    } else if (!parse_number(p, n, &s)) {
        return false;
    }
    if (s < 1) return false;
    *start = s;
    *end = e;
    return true;
}

uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
uint64_t rd64(const uint8_t *p) { return (uint64_t)rd32(p) | (uint64_t)rd32(p + 4) << 32; }

} // namespace

extern "C" int ngsq_vq_parse(const char *query, const char *const *names, uint32_t n_refs, uint32_t *ref_id, uint64_t *start,
                             uint64_t *end, char *err, size_t err_cap) {
    if (!query || !ref_id || !start || !end || (n_refs && !names)) return vq_fail(NGSQ_VQ_PARSE, err, err_cap, "parsing query: null argument");
    const size_t len = strlen(query);
    if (!len) return vq_fail(NGSQ_VQ_PARSE, err, err_cap, "parsing query: empty input");
    size_t name_len = len;
    uint64_t s = 1, e = NGSQ_VIEW_END_MAX;
    if (const char *colon = strrchr(query, ':')) {
        const size_t at = (size_t)(colon - query);
        if (parse_interval(colon + 1, len - at - 1, &s, &e)) name_len = at;
        else s = 1, e = NGSQ_VIEW_END_MAX;
    }
    for (uint32_t r = 0; r < n_refs; r++)
        if (names[r] && strlen(names[r]) == name_len && memcmp(names[r], query, name_len) == 0) {
            *ref_id = r;
            *start = s;
            *end = e;
            return NGSQ_VQ_OK;
        }
    return vq_fail(NGSQ_VQ_NAME, err, err_cap, "querying BAM file: the region's reference sequence \"%.*s\" is not in the header",
                   (int)std::min<size_t>(name_len, 200), query);
}

extern "C" int ngsq_vq_chunks(const uint8_t *bai, size_t bai_len, uint32_t ref_id, uint64_t start, uint64_t end, ngsq_view_chunk *chunks,
                              uint64_t cap, uint64_t *n, char *err, size_t err_cap) {
    if (!n || (bai_len && !bai) || (cap && !chunks)) return vq_fail(NGSQ_VQ_INDEX, err, err_cap, "reading BAM index: null argument");
    *n = 0;
    // the 0-based interval [beg, lim) and its bins: per level the first and last bin it meets (reg2bins, SAM specification 5.3)
    const uint64_t beg = start ? start - 1 : 0, lim = std::min<uint64_t>(end, NGSQ_VIEW_END_MAX);
    const bool any = beg < lim;
    static const struct { uint32_t shift, first; } LEVEL[5] = {{26, 1}, {23, 9}, {20, 73}, {17, 585}, {14, 4681}};
    auto wanted = [&](uint32_t bin) {
        if (!any) return false;
        if (bin == 0) return true;
        for (const auto &lv : LEVEL) {
            const uint64_t lo = lv.first + (beg >> lv.shift), hi = lv.first + ((lim - 1) >> lv.shift);
            if (bin >= lo && bin <= hi) return true;
        }
        return false; // (37450 and anything else outside the scheme)
    };
    size_t q = 0;
    auto need = [&](uint64_t k) { return k <= bai_len - q; }; // (q <= bai_len throughout)
    if (bai_len < 8 || memcmp(bai, "BAI\1", 4) != 0) return vq_fail(NGSQ_VQ_INDEX, err, err_cap, "reading BAM index: invalid BAI magic");
    const uint32_t n_ref = rd32(bai + 4);
    q = 8;
    if (ref_id >= n_ref)
        return vq_fail(NGSQ_VQ_INDEX, err, err_cap, "reading BAM index: the index holds %u reference sequences, the region's is number %u", n_ref, ref_id);
    std::vector<ngsq_view_chunk> found;
    uint64_t min_offset = 0;
    for (uint32_t r = 0; r < n_ref; r++) {
        if (!need(4)) return vq_fail(NGSQ_VQ_INDEX, err, err_cap, "reading BAM index: truncated (bins of reference %u)", r);
        const uint32_t n_bin = rd32(bai + q);
        q += 4;
        for (uint32_t k = 0; k < n_bin; k++) {
            if (!need(8)) return vq_fail(NGSQ_VQ_INDEX, err, err_cap, "reading BAM index: truncated bin");
            const uint32_t bin = rd32(bai + q), n_chunk = rd32(bai + q + 4);
            q += 8;
            if (!need((uint64_t)n_chunk * 16)) return vq_fail(NGSQ_VQ_INDEX, err, err_cap, "reading BAM index: truncated chunks");
            if (r == ref_id && wanted(bin))
                for (uint32_t c = 0; c < n_chunk; c++) found.push_back(ngsq_view_chunk{rd64(bai + q + (size_t)c * 16), rd64(bai + q + (size_t)c * 16 + 8)});
            q += (size_t)n_chunk * 16;
        }
        if (!need(4)) return vq_fail(NGSQ_VQ_INDEX, err, err_cap, "reading BAM index: truncated (intervals)");
        const uint32_t n_intv = rd32(bai + q);
        q += 4;
        if (!need((uint64_t)n_intv * 8)) return vq_fail(NGSQ_VQ_INDEX, err, err_cap, "reading BAM index: truncated linear index");
        if (r == ref_id && (beg >> 14) < n_intv) min_offset = rd64(bai + q + (size_t)(beg >> 14) * 8);
        q += (size_t)n_intv * 8;
    }
    if (q != bai_len && bai_len - q != 8) return vq_fail(NGSQ_VQ_INDEX, err, err_cap, "reading BAM index: trailing bytes");
    // chunks that end at or in front of the linear index's entry hold nothing of the region; neither does an empty chunk
    found.erase(std::remove_if(found.begin(), found.end(), [&](const ngsq_view_chunk &c) { return c.end <= min_offset || c.end <= c.begin; }),
                found.end());
    std::sort(found.begin(), found.end(), [](const ngsq_view_chunk &a, const ngsq_view_chunk &b) { return a.begin != b.begin ? a.begin < b.begin : a.end < b.end; });
    uint64_t m = 0;
    ngsq_view_chunk cur{};
    auto emit = [&]() {
        if (m < cap) chunks[m] = cur;
        m++;
    };
    for (size_t k = 0; k < found.size(); k++) {
        if (k && found[k].begin <= cur.end) {
            cur.end = std::max(cur.end, found[k].end);
            continue;
        }
        if (k) emit();
        cur = found[k];
    }
    if (!found.empty()) emit();
    *n = m;
    return NGSQ_VQ_OK;
}
