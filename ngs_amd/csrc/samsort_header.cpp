// samsort_header.cpp -- the header text of a coordinate-sorted file: ngsq_sam_sorted_header of
// include/ngsq_samtext.h and the function behind it, which the driver (samsort.cpp) calls.  Host only and free of HIP, so that
// tests/c/sorted_header_drive.c links it alone under the sanitizers.
#include <cstring>
#include <string>

#include "../../include/ngsq_samtext.h"

namespace ngsq {

std::string sorted_header_text(const char *text, size_t n) {
    const std::string t(text, n);
    const size_t hd = t.rfind("@HD", 0) == 0 ? 0 : t.find("\n@HD"); // (as ngsq_bam_sorted_by_coordinate looks for the line)
    if (hd == std::string::npos) return "@HD\tVN:1.6\tSO:coordinate\n" + t;
    const size_t beg = hd == 0 ? 0 : hd + 1;
    size_t eol = t.find('\n', beg);
    if (eol == std::string::npos) eol = t.size();
    std::string line;
    bool has_so = false;
    for (size_t f = beg; f <= eol;) {
        size_t fe = t.find('\t', f);
        if (fe == std::string::npos || fe > eol) fe = eol;
        const bool first = f == beg;
        if (!first && !has_so && t.compare(f, 3, "SO:") == 0) {
            line += "\tSO:coordinate";
            has_so = true;
        } else if (!first && t.compare(f, 3, "SS:") == 0 && t.compare(f + 3, 11, "coordinate:") != 0) {
            // (a sub-sort of another order says nothing about this file)
        } else {
            if (!first) line += '\t';
            line.append(t, f, fe - f);
        }
        f = fe + 1;
    }
    if (!has_so) line += "\tSO:coordinate";
    return t.substr(0, beg) + line + t.substr(eol);
}

} // namespace ngsq

extern "C" {

int ngsq_sam_sorted_header(const char *text, size_t n, char *out, size_t cap, size_t *out_n) {
    if ((n && !text) || !out_n || (cap && !out)) return NGSQ_ERR_INVALID_ARGUMENT;
    const std::string s = ngsq::sorted_header_text(n ? text : "", n);
    *out_n = s.size();
    if (s.size() > cap) return NGSQ_ERR_BUFFER_TOO_SMALL;
    memcpy(out, s.data(), s.size());
    return NGSQ_OK;
}

} // extern "C"
