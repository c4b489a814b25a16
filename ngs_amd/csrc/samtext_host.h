// samtext_host.h -- the host-only pieces of SAM to BAM, which samtext_run.h puts together into the
// chunk pipeline and the drivers (samtext.cpp, samsort.cpp; bamsort.cpp for the header text) use beside it: the header and its
// reference list, the header stream, the reference table for the device, the reader that cuts the text into chunks, the words
// of the messages.
#pragma once

#include <fcntl.h>

#include <cstdarg>
#include <string>
#include <unordered_set>
#include <vector>

#include "device_out.h"
#include "samtext_kernels.h"

namespace ngsq {

constexpr uint64_t ST_CHUNK_DEFAULT = (uint64_t)64 << 20, ST_CHUNK_MAX = (uint64_t)1 << 30; // (a line's record stays under 2^31 bytes)
constexpr const char *ST_OPEN_CTX = "opening SAM input file: ";

inline int sfail(ngsq_ctx *c, int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

inline const char *samtext_error_text(uint32_t code) {
    switch (code) {
    case ST_E_FIELDS: return "fewer than 11 fields";
    case ST_E_QNAME_EMPTY: return "empty read name";
    case ST_E_QNAME_LONG: return "read name longer than 254 bytes";
    case ST_E_FLAG: return "invalid FLAG";
    case ST_E_RNAME: return "reference sequence name not in the header";
    case ST_E_POS: return "invalid POS";
    case ST_E_MAPQ: return "invalid MAPQ";
    case ST_E_CIGAR_DIGITS: return "CIGAR operation without a length";
    case ST_E_CIGAR_OP: return "invalid CIGAR operation";
    case ST_E_CIGAR_LEN: return "CIGAR operation length of 2^28 or more";
    case ST_E_RNEXT: return "mate reference sequence name not in the header";
    case ST_E_PNEXT: return "invalid PNEXT";
    case ST_E_TLEN: return "invalid TLEN";
    case ST_E_SEQ: return "invalid SEQ base";
    case ST_E_QUAL_NO_SEQ: return "QUAL without SEQ";
    case ST_E_QUAL_LEN: return "QUAL length differs from SEQ length";
    case ST_E_QUAL_CHAR: return "QUAL byte outside 33..126";
    case ST_E_TAG_FORM: return "tag not of the form TG:T:V";
    case ST_E_TAG_TYPE: return "invalid tag value type";
    case ST_E_B_SUB: return "invalid B array subtype";
    case ST_E_NUMBER: return "malformed number";
    case ST_E_HEX: return "invalid H value";
    case ST_E_FLOAT_LONG: return "float text longer than 48 characters";
    case ST_E_TOO_LARGE: return "record larger than 2^31 bytes";
    default: return "invalid record";
    }
}

struct Fd {
    int fd = -1;
    ~Fd() {
        if (fd >= 0) close(fd);
    }
};

struct SamHeader {
    std::string text;               // the leading '@' lines, unchanged
    std::vector<std::string> names; // @SQ SN, file order
    std::vector<uint32_t> lens;     // @SQ LN
    uint64_t body_at = 0;           // file offset of the first record line
};

// pread until n bytes or the end of the file; the bytes read, or -errno
inline ssize_t pread_full(int fd, char *p, size_t n, uint64_t at) {
    size_t got = 0;
    while (got < n) {
        const ssize_t r = pread(fd, p + got, n - got, (off_t)(at + got));
        if (r < 0) {
            if (errno == EINTR) continue;
            return -errno;
        }
        if (r == 0) break;
        got += (size_t)r;
    }
    return (ssize_t)got;
}

// The header of the SAM file fd; "" or why it is refused (without the context).
inline std::string read_header(int fd, SamHeader *h) {
    std::vector<char> buf((size_t)1 << 20);
    uint64_t at = 0;
    bool line_start = true, done = false;
    while (!done) {
        const ssize_t n = pread_full(fd, buf.data(), buf.size(), at);
        if (n < 0) return std::string(strerror((int)-n)) + " (os error " + std::to_string(-n) + ")";
        if (n == 0) break;
        ssize_t i = 0;
        for (; i < n; i++) {
            if (line_start && buf[(size_t)i] != '@') {
                done = true;
                break;
            }
            line_start = buf[(size_t)i] == '\n';
            h->text.push_back(buf[(size_t)i]);
        }
        at += (uint64_t)i;
    }
    h->body_at = at;
    if (h->text.size() > 0x7FFFFFFFull) return "header text longer than 2^31 - 1 bytes";
    // the reference list: SN and LN of the @SQ lines (the text itself goes into the file as it is)
    std::unordered_set<std::string> seen;
    for (size_t a = 0; a < h->text.size();) {
        size_t e = h->text.find('\n', a);
        if (e == std::string::npos) e = h->text.size();
        if (e - a >= 4 && h->text.compare(a, 4, "@SQ\t") == 0) {
            std::string sn, ln;
            bool has_sn = false, has_ln = false;
            for (size_t f = a + 4; f <= e;) {
                size_t fe = h->text.find('\t', f);
                if (fe == std::string::npos || fe > e) fe = e;
                if (fe - f >= 3 && h->text.compare(f, 3, "SN:") == 0 && !has_sn) sn = h->text.substr(f + 3, fe - f - 3), has_sn = true;
                if (fe - f >= 3 && h->text.compare(f, 3, "LN:") == 0 && !has_ln) ln = h->text.substr(f + 3, fe - f - 3), has_ln = true;
                f = fe + 1;
            }
            const std::string line_no = std::to_string(h->names.size() + 1);
            if (!has_sn || sn.empty()) return "@SQ line " + line_no + " has no SN";
            if (!has_ln) return "@SQ line " + line_no + " (" + sn + ") has no LN";
            uint64_t v = 0;
            bool digits = !ln.empty();
            for (char ch : ln) {
                if (ch < '0' || ch > '9') digits = false;
                else if (v < ((uint64_t)1 << 40)) v = v * 10 + (uint64_t)(ch - '0');
            }
            if (!digits || v < 1 || v > 0x7FFFFFFFull) return "@SQ line " + line_no + " (" + sn + "): LN " + ln + " is outside 1..2147483647";
            if (!seen.insert(sn).second) return "@SQ line " + line_no + ": the sequence name " + sn + " stands in more than one @SQ line";
            h->names.push_back(sn);
            h->lens.push_back((uint32_t)v);
        }
        a = e + 1;
    }
    if (h->names.size() > 0x7FFFFFFFull) return "more than 2^31 - 1 @SQ lines";
    return "";
}

inline void put32(std::string &s, uint32_t v) {
    char b[4] = {(char)v, (char)(v >> 8), (char)(v >> 16), (char)(v >> 24)};
    s.append(b, 4);
}

// the header stream: magic, l_text, text, n_ref, names and lengths (SAM/BAM specification 4.2)
inline std::string header_stream(const std::string &text, const SamHeader &H) {
    const uint32_t n_refs = (uint32_t)H.names.size();
    std::string hs("BAM\1", 4);
    put32(hs, (uint32_t)text.size());
    hs += text;
    put32(hs, n_refs);
    for (uint32_t r = 0; r < n_refs; r++) {
        put32(hs, (uint32_t)H.names[r].size() + 1);
        hs += H.names[r];
        hs.push_back('\0');
        put32(hs, H.lens[r]);
    }
    return hs;
}

// the reference names for the device: words = [bad word | name_off[n_refs + 1] | table[slots]], names behind them
struct RefTable {
    std::vector<uint64_t> words;
    std::string names;
    uint32_t slots = 1, n_refs = 0;

    RefTable() = default;
    explicit RefTable(const SamHeader &H) : n_refs((uint32_t)H.names.size()) {
        while (slots < 2ull * n_refs) slots <<= 1;
        words.assign(1 + n_refs + 1 + (slots + 1) / 2, 0);
        words[0] = ~0ull;
        uint32_t *table = reinterpret_cast<uint32_t *>(words.data() + 1 + n_refs + 1);
        for (uint32_t r = 0; r < n_refs; r++) {
            words[1 + r] = names.size();
            names += H.names[r];
            uint32_t s = samtext_name_hash(reinterpret_cast<const uint8_t *>(H.names[r].data()), H.names[r].size()) & (slots - 1);
            while (table[s]) s = (s + 1) & (slots - 1);
            table[s] = r + 1;
        }
        words[1 + n_refs] = names.size();
    }
    size_t device_words() const { return words.size() + (names.size() + 7) / 8; }
    // words and names to d (device_words() of them) on s; the caller waits before this object goes
    hipError_t upload(uint64_t *d, hipStream_t s) const {
        hipError_t e = hipMemcpyAsync(d, words.data(), words.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s);
        if (e == hipSuccess && !names.empty()) e = hipMemcpyAsync(d + words.size(), names.data(), names.size(), hipMemcpyHostToDevice, s);
        return e;
    }
    unsigned long long *bad(uint64_t *d) const { return reinterpret_cast<unsigned long long *>(d); }
    SamTextRefs refs(const uint64_t *d) const {
        return SamTextRefs{reinterpret_cast<const uint32_t *>(d + 1 + n_refs + 1), d + 1, reinterpret_cast<const uint8_t *>(d + words.size()), slots, n_refs};
    }
};

// the header text of the coordinate-sorted file made from text[n] (samsort_header.cpp)
std::string sorted_header_text(const char *text, size_t n);

struct PinnedText {
    char *p = nullptr;
    ~PinnedText() {
        if (p) (void)hipHostFree(p);
    }
};

// The text behind the header, in chunks that end on a newline, through two pinned buffers: chunk k lies in pin[k & 1], and the
// bytes of the line it ended inside move to the front of the other buffer before that one is filled.
struct TextChunks {
    int fd = -1;
    uint64_t chunk_bytes = 0, file_at = 0;
    PinnedText pin[2];
    size_t carry = 0; // bytes of the line the last chunk ended inside, behind that chunk in its buffer
    bool eof = false;
    std::string long_line; // the refusal of a line that does not fit a chunk
    double read_ms = 0;

    size_t pin_bytes() const { return (size_t)chunk_bytes + 2 + ST_TEXT_SLACK; }
    hipError_t start(int fd_, uint64_t chunk_bytes_, uint64_t body_at) {
        fd = fd_, chunk_bytes = chunk_bytes_, file_at = body_at;
        for (auto &b : pin) {
            void *p = nullptr;
            const hipError_t e = hipHostMalloc(&p, pin_bytes(), hipHostMallocDefault);
            if (e != hipSuccess) return e;
            b.p = static_cast<char *>(p);
        }
        return hipSuccess;
    }
    // the next chunk into pin[slot]: *len bytes that end on a newline (0: the file has ended, or long_line says why not);
    // 0 or the errno of a failed read
    int fill(uint32_t slot, uint64_t *len) {
        const double t0 = now_ms();
        char *buf = pin[slot].p;
        size_t have = carry;
        *len = 0;
        if (!eof && have < chunk_bytes + 1) {
            const ssize_t r = pread_full(fd, buf + have, (size_t)chunk_bytes + 1 - have, file_at);
            if (r < 0) return (int)-r;
            if ((size_t)r < chunk_bytes + 1 - have) eof = true;
            have += (size_t)r;
            file_at += (uint64_t)r;
        }
        read_ms += now_ms() - t0;
        if (!have) return 0;
        const char *nl = static_cast<const char *>(memrchr(buf, '\n', have));
        size_t cut = nl ? (size_t)(nl - buf) + 1 : 0;
        if (!nl && have > chunk_bytes) {
            long_line = "line longer than " + std::to_string(chunk_bytes) + " bytes";
            return 0;
        }
        if (eof && cut < have) { // a last line without its newline is a line
            buf[have++] = '\n';
            cut = have;
        }
        carry = have - cut;
        *len = cut;
        return 0;
    }
    // before pin[slot][0, len) is copied up: the carry moves to the other buffer (the copy only reads)
    void move_carry(uint32_t slot, uint64_t len) {
        if (carry) memcpy(pin[slot ^ 1].p, pin[slot].p + len, carry);
    }
};

} // namespace ngsq
