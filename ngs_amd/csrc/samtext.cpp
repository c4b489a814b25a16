// samtext.cpp -- include/ngsq_samtext.h: `ngs convert --gzip device <SAM> <BAM>`.  The host reads the
// header (the leading '@' lines), builds the reference list and its hash table, and then only moves bytes: the text goes in
// chunks that end on a newline through two pinned buffers to the device, samtext_kernel.hip finds the lines and turns them
// into BAM records, the device DEFLATE encoder (deflate_kernels.h) makes BGZF blocks of them, and the output stage of
// device_out.h carries the blocks through its pinned ring to the descriptor.  While chunk k is written and compressed the host
// reads chunk k + 1 and copies it up on a second stream; while chunk k + 1 is parsed the writer copies chunk k down and
// writes it.  Per chunk the host reads four words: lines, record bytes, error word, compressed bytes.
#include "../../include/ngsq_samtext.h"

#include <fcntl.h>

#include <cstdarg>
#include <unordered_set>

#include "device_out.h"
#include "samtext_kernels.h"

using namespace ngsq;

namespace {

constexpr uint64_t ST_CHUNK_DEFAULT = (uint64_t)64 << 20, ST_CHUNK_MAX = (uint64_t)1 << 30; // (a line's record stays under 2^31 bytes)
constexpr const char *OPEN_CTX = "opening SAM input file: ";

int sfail(ngsq_ctx *c, int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

const char *samtext_error_text(uint32_t code) {
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
ssize_t pread_full(int fd, char *p, size_t n, uint64_t at) {
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
std::string read_header(int fd, SamHeader *h) {
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

void put32(std::string &s, uint32_t v) {
    char b[4] = {(char)v, (char)(v >> 8), (char)(v >> 16), (char)(v >> 24)};
    s.append(b, 4);
}

struct PinnedText {
    char *p = nullptr;
    ~PinnedText() {
        if (p) (void)hipHostFree(p);
    }
};

enum Ev { EV_UP0 = 0, EV_UP1, EV_H0, EV_H1, EV_P0, EV_P1, EV_W0, EV_W1, EV_Z1, EV_N };

enum HostWord : uint32_t { HW_LINES = 0, HW_BYTES, HW_BAD, HW_TEXT, HW_DEFLATE, HW_WORDS = HW_DEFLATE + DEFLATE_HOST_WORDS };

} // namespace

extern "C" {

int ngsq_sam_parse_f32(const char *text, uint32_t len, uint32_t *bits) {
    if (!text || !bits || len > ST_FLOAT_TEXT_MAX) return NGSQ_ERR_INVALID_ARGUMENT;
    return samtext_parse_f32_host(reinterpret_cast<const uint8_t *>(text), len, bits) ? NGSQ_OK : NGSQ_ERR_INVALID_ARGUMENT;
}

int ngsq_sam_check_header(const char *sam_path, uint32_t *n_refs, char *why, size_t why_cap) {
    auto say = [&](const std::string &m) {
        if (why && why_cap) snprintf(why, why_cap, "%s%s", OPEN_CTX, m.c_str());
        return NGSQ_ERR_INVALID_ARGUMENT;
    };
    if (why && why_cap) why[0] = 0;
    if (!sam_path) return say("null argument");
    Fd in;
    in.fd = open(sam_path, O_RDONLY | O_CLOEXEC);
    if (in.fd < 0) {
        const int e = errno;
        return say(std::string(strerror(e)) + " (os error " + std::to_string(e) + ")");
    }
    SamHeader h;
    const std::string m = read_header(in.fd, &h);
    if (!m.empty()) return say(m);
    if (n_refs) *n_refs = (uint32_t)h.names.size();
    return NGSQ_OK;
}

int ngsq_sam_write_bam(ngsq_ctx *c, const char *sam_path, int fd, uint64_t max_records, uint64_t chunk_bytes, ngsq_samtext_report *out) {
    if (out) memset(out, 0, sizeof *out);
    if (!c || !sam_path || fd < 0) return sfail(c, NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    const double t_begin = now_ms();
    if (!chunk_bytes) chunk_bytes = ST_CHUNK_DEFAULT;
    chunk_bytes = std::min(chunk_bytes, ST_CHUNK_MAX);
    Fd in;
    in.fd = open(sam_path, O_RDONLY | O_CLOEXEC);
    if (in.fd < 0) {
        const int e = errno;
        return sfail(c, NGSQ_ERR_INVALID_ARGUMENT, "%s%s (os error %d)", OPEN_CTX, strerror(e), e);
    }
    SamHeader H;
    {
        const std::string m = read_header(in.fd, &H);
        if (!m.empty()) return sfail(c, NGSQ_ERR_INVALID_ARGUMENT, "%s%s", OPEN_CTX, m.c_str());
    }
    const uint32_t n_refs = (uint32_t)H.names.size();
    // the header stream: magic, l_text, text, n_ref, names and lengths (SAM/BAM specification 4.2)
    std::string hs("BAM\1", 4);
    put32(hs, (uint32_t)H.text.size());
    hs += H.text;
    put32(hs, n_refs);
    for (uint32_t r = 0; r < n_refs; r++) {
        put32(hs, (uint32_t)H.names[r].size() + 1);
        hs += H.names[r];
        hs.push_back('\0');
        put32(hs, H.lens[r]);
    }
    // the reference names for the device: [bad word | name_off[n_refs + 1] | table[slots] | names]
    uint32_t slots = 1;
    while (slots < 2ull * n_refs) slots <<= 1;
    std::vector<uint64_t> setup(1 + n_refs + 1 + (slots + 1) / 2, 0);
    std::string names;
    setup[0] = ~0ull;
    {
        uint32_t *table = reinterpret_cast<uint32_t *>(setup.data() + 1 + n_refs + 1);
        for (uint32_t r = 0; r < n_refs; r++) {
            setup[1 + r] = names.size();
            names += H.names[r];
            uint32_t s = samtext_name_hash(reinterpret_cast<const uint8_t *>(H.names[r].data()), H.names[r].size()) & (slots - 1);
            while (table[s]) s = (s + 1) & (slots - 1);
            table[s] = r + 1;
        }
        setup[1 + n_refs] = names.size();
    }

    // ---- the device side; every HIP error leaves through `rc`, so that the writer is stopped either way
#define SHIP(expr)                                                                                  \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) return sfail(c, NGSQ_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
    hipStream_t st = c->stream, up = nullptr;
    DevArray<uint64_t> d_setup, d_tiles, d_start, d_off, d_flist;
    DevArray<uint8_t> d_fmark, d_text[2], d_rec;
    ScanScratch scan;
    BgzfEncoder enc; // d_rec's bytes become the blocks of a job
    JobSlots zslots; // of the encoder's blocks (d_text alternates with the chunks, apart from them)
    MappedBuf hw;
    PinnedText pin[2];
    HipEvents<EV_N> ev;
    DeviceWriter w;
    StreamDrain drain{st}, drain_up{nullptr, true}; // (behind the arrays: they run first)
    const size_t pin_bytes = (size_t)chunk_bytes + 2 + ST_TEXT_SLACK;
    uint64_t records = 0, text_bytes = 0, bam_bytes = 0, chunks = 0, bad = ~0ull;
    double read_ms = 0, h2d_ms = 0, parse_ms = 0, deflate_ms = 0;
    uint64_t file_at = H.body_at;
    size_t carry = 0; // bytes of the line the last chunk ended inside, at the front of the next buffer
    bool eof = false;
    std::string long_line; // the refusal of a line that does not fit a chunk

    // the next chunk into pin[slot]: *len bytes that end on a newline (0: the file has ended)
    auto fill = [&](uint32_t slot, uint64_t *len) -> int {
        const double t0 = now_ms();
        char *buf = pin[slot].p;
        size_t have = carry;
        *len = 0;
        if (!eof && have < chunk_bytes + 1) {
            const ssize_t r = pread_full(in.fd, buf + have, (size_t)chunk_bytes + 1 - have, file_at);
            if (r < 0) return sfail(c, NGSQ_ERR_INVALID_ARGUMENT, "reading SAM record: %s (os error %d)", strerror((int)-r), (int)-r);
            if ((size_t)r < chunk_bytes + 1 - have) eof = true;
            have += (size_t)r;
            file_at += (uint64_t)r;
        }
        read_ms += now_ms() - t0;
        if (!have) return NGSQ_OK;
        const char *nl = static_cast<const char *>(memrchr(buf, '\n', have));
        size_t cut = nl ? (size_t)(nl - buf) + 1 : 0;
        if (!nl && have > chunk_bytes) {
            long_line = "line longer than " + std::to_string(chunk_bytes) + " bytes";
            return NGSQ_OK;
        }
        if (eof && cut < have) { // a last line without its newline is a line
            buf[have++] = '\n';
            cut = have;
        }
        carry = have - cut;
        *len = cut;
        return NGSQ_OK;
    };
    // pin[slot][0, len) to d_text[slot] on the copy stream; the carry moves to the other buffer first (the copy only reads)
    auto upload = [&](uint32_t slot, uint64_t len) -> int {
        if (carry) memcpy(pin[slot ^ 1].p, pin[slot].p + len, carry);
        SHIP(d_text[slot].reserve(len + ST_TEXT_SLACK));
        SHIP(hipEventRecord(ev.e[EV_H0], up));
        SHIP(hipMemcpyAsync(d_text[slot].p, pin[slot].p, len, hipMemcpyHostToDevice, up));
        SHIP(hipEventRecord(ev.e[EV_H1], up));
        SHIP(hipEventRecord(ev.e[EV_UP0 + slot], up));
        return NGSQ_OK;
    };
    auto copy_failed = [&](hipError_t e) { return sfail(c, NGSQ_ERR_DEVICE, "copying the BGZF blocks to the host: %s", hipGetErrorString(e)); };
    // bytes of d_rec through the encoder into its buffer of the job's slot; push_job waits for it and hands the blocks to the writer
    auto compress = [&](uint64_t bytes) -> int {
        if (!zslots.acquire(&w)) return copy_failed(w.herr);
        SHIP(enc.launch(zslots.slot(), d_rec.p, bytes, st));
        SHIP(hipEventRecord(ev.e[EV_Z1], st));
        return NGSQ_OK;
    };
    auto push_job = [&](uint64_t bytes) -> int {
        SHIP(hipEventSynchronize(ev.e[EV_Z1]));
        const char *blocks = nullptr;
        uint64_t n = 0;
        if (const char *m = enc.collect(zslots.slot(), bytes, &blocks, &n)) return sfail(c, NGSQ_ERR_STATE, "%s", m);
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.e[EV_W1], ev.e[EV_Z1]) == hipSuccess) deflate_ms += ms;
        // (nothing may be queued on st between compress and here: `ready` would cover it and hold the copy back)
        SHIP(zslots.submit(w, blocks, n, st));
        bam_bytes += bytes;
        return NGSQ_OK;
    };

    auto run = [&]() -> int {
        SHIP(hipSetDevice(c->device));
        SHIP(pool_stream_get(false, &up));
        drain_up.s = up;
        SHIP(d_setup.reserve(setup.size() + (names.size() + 7) / 8));
        SHIP(hipMemcpyAsync(d_setup.p, setup.data(), setup.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        if (!names.empty()) SHIP(hipMemcpyAsync(d_setup.p + setup.size(), names.data(), names.size(), hipMemcpyHostToDevice, st));
        SHIP(hipStreamSynchronize(st)); // (setup and names are this function's)
        unsigned long long *const d_bad = reinterpret_cast<unsigned long long *>(d_setup.p);
        const SamTextRefs refs{reinterpret_cast<const uint32_t *>(d_setup.p + 1 + n_refs + 1), d_setup.p + 1, reinterpret_cast<const uint8_t *>(d_setup.p + setup.size()),
                               slots, n_refs};
        SHIP(hw.reserve(HW_WORDS * sizeof(unsigned long long)));
        memset(hw.h, 0, HW_WORDS * sizeof(unsigned long long));
        unsigned long long *const hdev = static_cast<unsigned long long *>(hw.dev);
        const unsigned long long *const h = static_cast<const unsigned long long *>(hw.h);
        for (int k = 0; k < 2; k++) {
            void *p = nullptr;
            SHIP(hipHostMalloc(&p, pin_bytes, hipHostMallocDefault));
            pin[k].p = static_cast<char *>(p);
        }
        enc.h = h + HW_DEFLATE;
        enc.hdev = hdev + HW_DEFLATE;
        for (int k = 0; k < EV_N; k++) {
            if (k == EV_UP0 || k == EV_UP1) SHIP(hipEventCreateWithFlags(&ev.e[k], hipEventDisableTiming));
            else SHIP(hipEventCreate(&ev.e[k]));
        }
        SHIP(zslots.create());
        SHIP(w.start(fd, c->device));
        // the header's blocks, in front of the first record (as samtools writes them)
        SHIP(d_rec.reserve(hs.size() + DEFLATE_IN_SLACK));
        SHIP(hipMemcpyAsync(d_rec.p, hs.data(), hs.size(), hipMemcpyHostToDevice, st));
        SHIP(hipEventRecord(ev.e[EV_W1], st));
        if (const int rc = compress(hs.size())) return rc;
        if (const int rc = push_job(hs.size())) return rc;
        // the chunks
        uint64_t len = 0;
        if (const int rc = fill(0, &len)) return rc;
        if (len)
            if (const int rc = upload(0, len)) return rc;
        while (len && !w.failed()) {
            const uint32_t slot = (uint32_t)(chunks & 1);
            // line starts
            const uint64_t tiles = samtext_tiles(len);
            SHIP(d_tiles.reserve(tiles + 1));
            SHIP(hipStreamWaitEvent(st, ev.e[EV_UP0 + slot], 0));
            SHIP(hipEventRecord(ev.e[EV_P0], st));
            SHIP(launch_samtext_count(d_text[slot].p, len, d_tiles.p, st));
            SHIP(scan.exclusive_scan(d_tiles.p, tiles + 1, st));
            SHIP(launch_samtext_word(d_tiles.p, tiles, hdev + HW_LINES, st));
            SHIP(hipStreamSynchronize(st));
            {
                float ms = 0;
                if (hipEventElapsedTime(&ms, ev.e[EV_H0], ev.e[EV_H1]) == hipSuccess) h2d_ms += ms;
            }
            const uint64_t lines = h[HW_LINES];
            const uint64_t n = max_records ? std::min(lines, max_records - records) : lines;
            // sizes, offsets, and the chunk's record bytes and error word to the host
            SHIP(d_start.reserve(n + 1));
            SHIP(d_off.reserve(n + 1));
            SHIP(d_fmark.reserve(n));
            SHIP(d_flist.reserve(n + 1));
            const SamTextFloats fl{d_fmark.p, d_flist.p + 1, reinterpret_cast<unsigned long long *>(d_flist.p)};
            SHIP(launch_samtext_scatter(d_text[slot].p, len, d_tiles.p, n, d_start.p, st));
            SHIP(launch_samtext_word(d_start.p, n, hdev + HW_TEXT, st));
            SHIP(launch_samtext_size(d_text[slot].p, d_start.p, n, records, refs, d_off.p, d_bad, fl, st));
            SHIP(scan.exclusive_scan(d_off.p, n + 1, st));
            SHIP(launch_samtext_total(d_off.p, n, d_bad, hdev + HW_BYTES, st));
            SHIP(hipEventRecord(ev.e[EV_P1], st));
            SHIP(hipStreamSynchronize(st));
            {
                float ms = 0;
                if (hipEventElapsedTime(&ms, ev.e[EV_P0], ev.e[EV_P1]) == hipSuccess) parse_ms += ms;
            }
            const uint64_t bytes = h[HW_BYTES];
            if (h[HW_BAD] != ~0ull) {
                bad = h[HW_BAD];
                break;
            }
            // the records, and their blocks
            SHIP(d_rec.reserve(bytes + DEFLATE_IN_SLACK));
            SHIP(hipEventRecord(ev.e[EV_W0], st));
            SHIP(launch_samtext_write(d_text[slot].p, d_start.p, n, refs, d_off.p, d_rec.p, fl, st));
            SHIP(hipEventRecord(ev.e[EV_W1], st));
            if (const int rc = compress(bytes)) return rc;
            records += n;
            text_bytes += h[HW_TEXT];
            chunks++;
            // the next chunk is read and copied up while this one is written and compressed
            uint64_t next = 0;
            if (!max_records || records < max_records) {
                if (const int rc = fill(slot ^ 1, &next)) return rc;
                if (next)
                    if (const int rc = upload(slot ^ 1, next)) return rc;
            }
            if (const int rc = push_job(bytes)) return rc;
            {
                float ms = 0;
                if (hipEventElapsedTime(&ms, ev.e[EV_W0], ev.e[EV_W1]) == hipSuccess) parse_ms += ms;
            }
            len = next;
        }
        SHIP(hipStreamSynchronize(st));
        SHIP(hipStreamSynchronize(up));
        return NGSQ_OK;
    };
    int rc = run();
#undef SHIP
    auto write_failed = [&](int e) { return sfail(c, NGSQ_ERR_INVALID_ARGUMENT, "writing BAM record: %s (os error %d)", strerror(e), e); };
    const WriterEnd end = w.end();
    if (rc == NGSQ_OK && end.herr != hipSuccess) rc = copy_failed(end.herr);
    if (rc == NGSQ_OK && end.werr) rc = write_failed(end.werr);
    if (rc == NGSQ_OK && bad != ~0ull)
        rc = sfail(c, NGSQ_ERR_MALFORMED_RECORD, "reading SAM record: record %llu: %s", (unsigned long long)(bad >> ST_ERR_BITS),
                   samtext_error_text((uint32_t)(bad & ((1u << ST_ERR_BITS) - 1))));
    if (rc == NGSQ_OK && !long_line.empty())
        rc = sfail(c, NGSQ_ERR_LIMIT, "reading SAM record: record %llu: %s", (unsigned long long)records, long_line.c_str());
    if (rc == NGSQ_OK) {
        if (const int e = write_bgzf_eof(fd)) rc = write_failed(e);
        enc.comp_bytes += sizeof BGZF_EOF_BLOCK;
    }
    if (out) {
        out->records = records;
        out->header_bytes = H.text.size();
        out->text_bytes = text_bytes;
        out->bam_bytes = bam_bytes;
        out->compressed_bytes = enc.comp_bytes;
        out->chunks = chunks;
        out->blocks = enc.blocks;
        out->stored_blocks = enc.stored;
        out->read_ms = read_ms;
        out->h2d_ms = h2d_ms;
        out->parse_ms = parse_ms;
        out->deflate_ms = deflate_ms;
        out->d2h_ms = w.copy_ms;
        out->write_ms = w.write_ms;
        out->total_ms = now_ms() - t_begin;
    }
    return rc;
}

} // extern "C"
