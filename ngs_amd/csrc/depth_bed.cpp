// depth_bed.cpp -- ngsq_depth_read_bed (include/ngsq_depth.h): the intervals of a BED file, read against
// the reference list of an open reader, for the mean depth per interval.  Host code only: it needs no GPU.
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ngsq_depth.h"
#include "bam_reader.h"

namespace {

constexpr uint64_t BED_MAX = 0x7FFFFFFFull; // the largest coordinate, and the most intervals

// decimal digits without a sign, at most BED_MAX
bool bed_number(const std::string &t, uint64_t *v) {
    if (t.empty()) return false;
    uint64_t x = 0;
    for (const char ch : t) {
        if (ch < '0' || ch > '9') return false;
        x = x * 10 + (uint64_t)(ch - '0');
        if (x > BED_MAX) return false;
    }
    *v = x;
    return true;
}

bool begins(const std::string &s, const char *prefix) { return s.compare(0, strlen(prefix), prefix) == 0; }

} // namespace

extern "C" int ngsq_depth_read_bed(const ngsq_bam *b, const char *path, ngsq_depth_interval **intervals, uint64_t *n) {
    if (!b || !path || !intervals || !n) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "null or invalid argument");
    *intervals = nullptr;
    *n = 0;
    FILE *f = fopen(path, "rb");
    if (!f) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "opening BED file: %s (os error %d)", strerror(errno), errno);
    std::unordered_map<std::string, uint32_t> by_name;
    for (size_t r = b->ref_names.size(); r-- > 0;) by_name[b->ref_names[r]] = (uint32_t)r; // (a repeated name: its first sequence)
    std::vector<ngsq_depth_interval> out;
    std::string line, why;
    unsigned long long line_no = 0;
    char *buf = nullptr;
    size_t cap = 0;
    ssize_t got;
    while (why.empty() && (got = getline(&buf, &cap, f)) >= 0) {
        line_no++;
        line.assign(buf, (size_t)got);
        if (!line.empty() && line.back() == '\n') line.pop_back();
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#' || begins(line, "track") || begins(line, "browser")) continue;
        std::vector<std::string> fields;
        for (size_t at = 0;;) {
            const size_t tab = line.find('\t', at);
            fields.push_back(line.substr(at, tab == std::string::npos ? std::string::npos : tab - at));
            if (tab == std::string::npos) break;
            at = tab + 1;
        }
        uint64_t start = 0, end = 0;
        if (fields.size() < 3) {
            why = "expected at least 3 tab-separated fields, found " + std::to_string(fields.size());
        } else if (!bed_number(fields[1], &start)) {
            why = "invalid start '" + fields[1] + "': expected a decimal number of at most 2147483647";
        } else if (!bed_number(fields[2], &end)) {
            why = "invalid end '" + fields[2] + "': expected a decimal number of at most 2147483647";
        } else if (start >= end) {
            why = "start " + std::to_string(start) + " is not below end " + std::to_string(end);
        } else {
            const auto it = by_name.find(fields[0]);
            if (it == by_name.end()) {
                why = "sequence '" + fields[0] + "' is not in the header";
            } else if (start >= b->ref_lens[it->second]) {
                why = "start " + std::to_string(start) + " lies at or beyond the end of '" + fields[0] + "' (" + std::to_string(b->ref_lens[it->second]) + " positions)";
            } else if (out.size() >= BED_MAX) {
                why = "more than 2147483647 intervals";
            } else {
                out.push_back(ngsq_depth_interval{(int32_t)it->second, (uint32_t)start, (uint32_t)std::min<uint64_t>(end, b->ref_lens[it->second])});
            }
        }
    }
    const bool read_failed = why.empty() && ferror(f);
    const int read_errno = errno;
    free(buf);
    fclose(f);
    if (read_failed) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "reading BED file: %s (os error %d)", strerror(read_errno), read_errno);
    if (!why.empty()) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "reading BED file: line %llu: %s", line_no, why.c_str());
    if (out.empty()) return NGSQ_OK;
    ngsq_depth_interval *p = static_cast<ngsq_depth_interval *>(malloc(out.size() * sizeof(ngsq_depth_interval)));
    if (!p) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "reading BED file: out of memory for %zu intervals", out.size());
    memcpy(p, out.data(), out.size() * sizeof(ngsq_depth_interval));
    *intervals = p;
    *n = out.size();
    return NGSQ_OK;
}

extern "C" void ngsq_depth_free_intervals(ngsq_depth_interval *intervals) { free(intervals); }
