// generate.cpp -- include/ngsq_generate.h: `ngs generate`.  The host opens and measures the FASTAs
// (no HIP), brings them to the device as letters (reference_load.h) beside the providers' tables, and then only launches:
// k_gen_draw chooses and sizes every pair of a batch, the ingest's scan turns the sizes into offsets, k_gen_write writes both
// files' text, and the output stage of device_out.h (one writer thread per file) carries it through pinned rings to the
// descriptors while the next batch is drawn.  The host never sees a base.
#include "../../include/ngsq_generate.h"

#include <cstdarg>
#include <memory>
#include <unordered_set>

#include "device_out.h"
#include "generate_kernels.h"
#include "reference_load.h"

using namespace ngsq;

namespace {

thread_local std::string g_gen_err;

int gfail(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_gen_err = buf;
    return code;
}

#define GHIP(expr)                                                                                    \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return gfail(NGSQ_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

constexpr uint64_t GEN_BATCH_PAIRS = (uint64_t)1 << 19;
constexpr uint64_t GEN_MAX_BATCH_PAIRS = (uint64_t)1 << 24;

struct Provider {
    ngsq_generate_provider p{};
    std::string path, fname; // fname: Path::file_name
    ngsq_fasta *fa = nullptr;
    std::vector<std::string> names;
    std::vector<uint64_t> len; // bases of every record, file order
    uint64_t total = 0, eligible = 0;
    int64_t lower = 0;
    std::vector<uint64_t> table;
    FastaLetters letters;
    ~Provider() { ngsq_fasta_close(fa); }
};

} // namespace

struct ngsq_generate {
    std::vector<std::unique_ptr<Provider>> prov;
    uint64_t total_weight = 0;
    // the device side (ngsq_generate_load)
    ngsq_ctx *ctx = nullptr;
    DevArray<uint8_t> d_tables;
    GenTables T{};
};

extern "C" {

const char *ngsq_generate_last_error(void) { return g_gen_err.c_str(); }

void ngsq_generate_close(ngsq_generate *g) {
    if (!g) return;
    if (g->ctx) (void)hipSetDevice(g->ctx->device); // (the letters go back to that device's cache)
    delete g;
}

int ngsq_generate_open(const ngsq_generate_provider *providers, uint32_t n_providers, ngsq_generate **out) {
    if (!providers || !out || !n_providers) return gfail(NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    std::unique_ptr<ngsq_generate> g(new ngsq_generate());
    char why[1024];
    for (uint32_t k = 0; k < n_providers; k++) {
        if (!providers[k].path) return gfail(NGSQ_ERR_INVALID_ARGUMENT, "null argument");
        if (const int rc = ngsq_generate_check_provider(&providers[k], providers[k].path, why, sizeof why)) return gfail(rc, "%s", why);
        std::unique_ptr<Provider> P(new Provider());
        P->p = providers[k];
        P->path = providers[k].path;
        P->p.path = nullptr;
        const size_t slash = P->path.rfind('/');
        P->fname = slash == std::string::npos ? P->path : P->path.substr(slash + 1);
        uint64_t n = 0;
        if (const int rc = ngsq_generate_inner_table(P->p.mu, P->p.sigma, &P->lower, nullptr, 0, &n, why, sizeof why)) return gfail(rc, "%s", why);
        P->table.resize(n);
        (void)ngsq_generate_inner_table(P->p.mu, P->p.sigma, &P->lower, P->table.data(), n, &n, why, sizeof why);
        if (g->total_weight + P->p.weight < g->total_weight) return gfail(NGSQ_ERR_LIMIT, "the weights of the reference providers add up to more than 2^64");
        g->total_weight += P->p.weight;
        g->prov.push_back(std::move(P));
    }
    // (decision: the reference's choose_weighted(...).unwrap() panics)
    if (!g->total_weight) return gfail(NGSQ_ERR_INVALID_ARGUMENT, "every reference provider has a weight of 0: no provider can be chosen");
    for (auto &P : g->prov)
        if (ngsq_fasta_open(P->path.c_str(), 0, &P->fa) != NGSQ_OK) return gfail(NGSQ_ERR_INVALID_ARGUMENT, "%s", ngsq_fasta_last_error());
    for (auto &P : g->prov) {
        const int64_t nr = ngsq_fasta_n_records(P->fa);
        if (nr < 0) return gfail(NGSQ_ERR_INVALID_ARGUMENT, "%s: %s", P->fname.c_str(), ngsq_fasta_last_error());
        std::string err;
        if (const int rc = fasta_record_bases(P->fa, &P->len, &err)) return gfail(rc, "%s: %s", P->fname.c_str(), err.c_str());
        // (decision: the reference's HashMap keeps the last record of a name and the lengths of all of them)
        std::unordered_set<std::string> seen;
        for (int64_t i = 0; i < nr; i++) {
            P->names.push_back(ngsq_fasta_record_name(P->fa, (uint32_t)i));
            if (!seen.insert(P->names.back()).second)
                return gfail(NGSQ_ERR_INVALID_ARGUMENT, "%s: the sequence name %s stands in front of more than one record", P->fname.c_str(), P->names.back().c_str());
            P->total += P->len[(size_t)i];
            if (P->len[(size_t)i] >= 2 * P->p.read_length + 2) P->eligible += P->len[(size_t)i];
        }
        if (!P->eligible)
            return gfail(NGSQ_ERR_INVALID_ARGUMENT,
                         "%s: no sequence holds the %llu bases a pair of %llu-base reads is drawn from (twice the read length and two more)",
                         P->fname.c_str(), (unsigned long long)(2 * P->p.read_length + 2), (unsigned long long)P->p.read_length);
    }
    *out = g.release();
    return NGSQ_OK;
}

uint64_t ngsq_generate_reads_for_coverage(const ngsq_generate *g, uint64_t coverage) {
    if (!g || g->prov.empty()) return 0;
    const uint64_t per = g->prov[0]->total / g->prov[0]->p.read_length;
    return per && coverage > UINT64_MAX / per ? UINT64_MAX : coverage * per;
}
uint32_t ngsq_generate_n_sequences(const ngsq_generate *g, uint32_t p) { return g && p < g->prov.size() ? (uint32_t)g->prov[p]->names.size() : 0; }
const char *ngsq_generate_sequence_name(const ngsq_generate *g, uint32_t p, uint32_t s) {
    return g && p < g->prov.size() && s < g->prov[p]->names.size() ? g->prov[p]->names[s].c_str() : nullptr;
}
uint64_t ngsq_generate_sequence_length(const ngsq_generate *g, uint32_t p, uint32_t s) {
    return g && p < g->prov.size() && s < g->prov[p]->len.size() ? g->prov[p]->len[s] : 0;
}

int ngsq_generate_load(ngsq_generate *g, ngsq_ctx *c) {
    if (!g || !c) return gfail(NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    if (g->ctx) return gfail(NGSQ_ERR_STATE, "the providers of this generator are on a device already");
    GHIP(hipSetDevice(c->device));
    // ---- the letters of every FASTA
    for (auto &P : g->prov) {
        std::string err;
        if (const int rc = fasta_load_letters(P->fa, c->device, c->li, &P->letters, &err)) return gfail(rc, "%s: %s", P->fname.c_str(), err.c_str());
        for (size_t i = 0; i < P->len.size(); i++)
            if (P->letters.len[i] != P->len[i])
                return gfail(NGSQ_ERR_STATE, "%s: sequence %s has %llu bases on the device and %llu on the host", P->fname.c_str(), P->names[i].c_str(),
                             (unsigned long long)P->letters.len[i], (unsigned long long)P->len[i]);
    }
    // ---- the tables: providers | sequences | cumulative eligible lengths | inner tables | names
    std::vector<GenProviderDev> pv;
    std::vector<GenSeqDev> sv;
    std::vector<uint64_t> cum, inner;
    std::string names;
    uint64_t weight_end = 0;
    for (auto &P : g->prov) {
        GenProviderDev d{};
        d.read_length = P->p.read_length;
        d.error_freq = P->p.error_freq;
        d.inner_lower = P->lower;
        d.elig_total = P->eligible;
        d.weight_end = (weight_end += P->p.weight);
        d.seq_first = (uint32_t)sv.size();
        d.n_seq = (uint32_t)P->len.size();
        d.cum_first = (uint32_t)cum.size();
        d.tab_first = (uint32_t)inner.size();
        d.tab_n = (uint32_t)P->table.size();
        d.fname_off = (uint32_t)names.size();
        d.fname_len = (uint32_t)P->fname.size();
        names += P->fname;
        uint64_t run = 0;
        for (size_t i = 0; i < P->len.size(); i++) {
            sv.push_back(GenSeqDev{P->letters.d + P->letters.off[i], P->len[i], (uint32_t)names.size(), (uint32_t)P->names[i].size()});
            names += P->names[i];
            cum.push_back(run);
            if (P->len[i] >= 2 * P->p.read_length + 2) run += P->len[i];
        }
        cum.push_back(run);
        inner.insert(inner.end(), P->table.begin(), P->table.end());
        pv.push_back(d);
    }
    if (sv.size() > 0x7FFFFFFFull || cum.size() > 0x7FFFFFFFull || inner.size() > 0x7FFFFFFFull || names.size() > 0x7FFFFFFFull)
        return gfail(NGSQ_ERR_LIMIT, "the providers' tables pass 2^31 entries");
    const size_t o_prov = 0, o_seq = o_prov + pv.size() * sizeof(GenProviderDev), o_cum = o_seq + sv.size() * sizeof(GenSeqDev), o_inner = o_cum + cum.size() * 8,
                 o_names = o_inner + inner.size() * 8, bytes = o_names + names.size();
    GHIP(g->d_tables.reserve(bytes + 8));
    uint8_t *d = g->d_tables.p;
    hipStream_t st = c->stream;
    GHIP(hipMemcpyAsync(d + o_prov, pv.data(), pv.size() * sizeof(GenProviderDev), hipMemcpyHostToDevice, st));
    GHIP(hipMemcpyAsync(d + o_seq, sv.data(), sv.size() * sizeof(GenSeqDev), hipMemcpyHostToDevice, st));
    GHIP(hipMemcpyAsync(d + o_cum, cum.data(), cum.size() * 8, hipMemcpyHostToDevice, st));
    GHIP(hipMemcpyAsync(d + o_inner, inner.data(), inner.size() * 8, hipMemcpyHostToDevice, st));
    if (!names.empty()) GHIP(hipMemcpyAsync(d + o_names, names.data(), names.size(), hipMemcpyHostToDevice, st));
    GHIP(hipStreamSynchronize(st)); // (the vectors are this function's)
    g->T.prov = reinterpret_cast<const GenProviderDev *>(d + o_prov);
    g->T.seq = reinterpret_cast<const GenSeqDev *>(d + o_seq);
    g->T.seq_cum = reinterpret_cast<const uint64_t *>(d + o_cum);
    g->T.inner = reinterpret_cast<const uint64_t *>(d + o_inner);
    g->T.names = reinterpret_cast<const char *>(d + o_names);
    g->T.total_weight = g->total_weight;
    g->T.n_prov = (uint32_t)pv.size();
    g->ctx = c;
    return NGSQ_OK;
}

// bgzf: bit k set = file k receives BGZF (the batch's text compressed on the device in front of its writer), and the EOF block
// at the end; ext (optional) receives what the encoder did.
static int generate_write(ngsq_generate *g, int fd_one, int fd_two, uint64_t seed, uint64_t first_pair, uint64_t n_pairs, uint64_t batch_pairs,
                          ngsq_generate_report *out, uint32_t bgzf, ngsq_generate_bgzf_report *ext) {
    if (!g || fd_one < 0 || fd_two < 0) return gfail(NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    if (out) memset(out, 0, sizeof *out);
    auto write_failed = [](int k, int e) {
        return gfail(NGSQ_ERR_INVALID_ARGUMENT, "could not write record to read %s file: %s (os error %d)", k ? "two" : "one", strerror(e), e);
    };
    auto write_eof = [&](int k) -> int {
        const int e = write_bgzf_eof(k ? fd_two : fd_one);
        return e ? write_failed(k, e) : NGSQ_OK;
    };
    if (bgzf && !n_pairs && first_pair <= (UINT64_MAX >> GEN_ERR_BITS)) { // (no pair: no device)
        for (int k = 0; k < 2; k++)
            if (bgzf >> k & 1) {
                if (const int rc = write_eof(k)) return rc;
                if (ext) (k ? ext->compressed_bytes_two : ext->compressed_bytes_one) = sizeof BGZF_EOF_BLOCK;
            }
        return NGSQ_OK;
    }
    if (!g->ctx) return gfail(NGSQ_ERR_STATE, "ngsq_generate_load was not called");
    if (first_pair > (UINT64_MAX >> GEN_ERR_BITS) || n_pairs > (UINT64_MAX >> GEN_ERR_BITS) - first_pair)
        return gfail(NGSQ_ERR_LIMIT, "pair numbers are taken up to 2^56");
    if (!n_pairs) return NGSQ_OK;
    if (!batch_pairs) batch_pairs = GEN_BATCH_PAIRS;
    batch_pairs = std::min(batch_pairs, GEN_MAX_BATCH_PAIRS);
    const double t_begin = now_ms();
    ngsq_ctx *c = g->ctx;
    GHIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const uint64_t n0 = std::min(batch_pairs, n_pairs);
    DevArray<GenPick> d_pick;
    DevArray<uint64_t> d_off;
    DevArray<unsigned long long> d_work;
    DevArray<char> d_text[2][2]; // [file][batch & 1]
    ScanScratch scan;
    MappedBuf hw;
    HipEvents<4> ev; // draw a/b, write a/b
    JobSlots slots; // of d_text and of the encoders' blocks: the two files share the batch
    // BGZF: a file's encoder with its compressed batches [batch & 1], the words both hand the host, the time of a batch's launches
    BgzfEncoder enc[2];
    MappedBuf zhw;
    HipEvents<2> zev;
    double deflate_ms = 0;
    DeviceWriter w[2];     // (behind the buffers and events its copies use: its copy stream is drained before they go)
    StreamDrain drain{st}; // (behind the arrays: it runs first)
    if (bgzf) {
        GHIP(zhw.reserve(2 * DEFLATE_HOST_WORDS * sizeof(unsigned long long)));
        memset(zhw.h, 0, 2 * DEFLATE_HOST_WORDS * sizeof(unsigned long long));
        for (int k = 0; k < 2; k++) {
            enc[k].h = static_cast<const unsigned long long *>(zhw.h) + k * DEFLATE_HOST_WORDS;
            enc[k].hdev = static_cast<unsigned long long *>(zhw.dev) + k * DEFLATE_HOST_WORDS;
            enc[k].effort = c->bgzf_effort;
        }
        GHIP(hipEventCreate(&zev.e[0]));
        GHIP(hipEventCreate(&zev.e[1]));
    }
    GHIP(d_pick.reserve(n0));
    GHIP(d_off.reserve(n0 + 1));
    GHIP(d_work.reserve(GEN_WORK_WORDS));
    GHIP(hw.reserve(GEN_HOST_WORDS * sizeof(unsigned long long)));
    memset(hw.h, 0, GEN_HOST_WORDS * sizeof(unsigned long long));
    {
        unsigned long long init[GEN_WORK_WORDS] = {};
        init[GW_BAD] = ~0ull;
        GHIP(hipMemcpyAsync(d_work.p, init, sizeof init, hipMemcpyHostToDevice, st));
        GHIP(hipStreamSynchronize(st));
    }
    GHIP(slots.create());
    for (auto &e : ev.e) GHIP(hipEventCreate(&e));
    for (int k = 0; k < 2; k++) GHIP(w[k].start(k ? fd_two : fd_one, c->device));
    uint64_t done = 0, text_bytes = 0, bad = ~0ull;
    unsigned long long rej[3] = {0, 0, 0};
    double draw_ms = 0, format_ms = 0;
    bool write_pending = false;
    auto add_write_time = [&] {
        float ms = 0;
        if (write_pending && hipEventElapsedTime(&ms, ev.e[2], ev.e[3]) == hipSuccess) format_ms += ms;
        write_pending = false;
    };
    // one batch; the function's HIP errors leave through `rc`, so that the writers are stopped below either way
    auto batch = [&](uint64_t first, uint64_t n) -> int {
        GHIP(hipEventRecord(ev.e[0], st));
        GHIP(launch_gen_draw(g->T, seed, first, n, d_pick.p, d_off.p, d_work.p, st));
        GHIP(scan.exclusive_scan(d_off.p, n + 1, st));
        GHIP(launch_gen_total(d_off.p, n, d_work.p, static_cast<unsigned long long *>(hw.dev), st));
        GHIP(hipEventRecord(ev.e[1], st));
        GHIP(hipEventSynchronize(ev.e[1]));
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.e[0], ev.e[1]) == hipSuccess) draw_ms += ms;
        add_write_time();
        const unsigned long long *const h = static_cast<const unsigned long long *>(hw.h);
        const uint64_t bytes = h[0];
        for (int k = 0; k < 3; k++) rej[k] = h[1 + GW_REJ_START + k];
        if (h[1 + GW_BAD] != ~0ull) {
            bad = h[1 + GW_BAD];
            return NGSQ_OK;
        }
        if (!slots.acquire(w, 2)) return NGSQ_OK; // (the writer's error is read at the end)
        const uint32_t slot = slots.slot();
        GHIP(d_text[0][slot].reserve(bytes + 1 + (bgzf ? DEFLATE_IN_SLACK : 0)));
        GHIP(d_text[1][slot].reserve(bytes + 1 + (bgzf ? DEFLATE_IN_SLACK : 0)));
        GHIP(hipEventRecord(ev.e[2], st));
        GHIP(launch_gen_write(g->T, seed, first, n, d_pick.p, d_off.p, d_text[0][slot].p, d_text[1][slot].p, st));
        GHIP(hipEventRecord(ev.e[3], st));
        const char *src[2] = {d_text[0][slot].p, d_text[1][slot].p};
        uint64_t job_bytes[2] = {bytes, bytes};
        if (bgzf && bytes) {
            // the text of a compressed file stays on the device: its blocks are what the writer copies.  The host learns their
            // size from the encoder's pinned words, so it waits for the batch here (the writers still work on the one before).
            GHIP(hipEventRecord(zev.e[0], st));
            for (int k = 0; k < 2; k++)
                if (bgzf >> k & 1) GHIP(enc[k].launch(slot, d_text[k][slot].p, bytes, st));
            GHIP(hipEventRecord(zev.e[1], st));
            GHIP(hipEventSynchronize(zev.e[1]));
            float zms = 0;
            if (hipEventElapsedTime(&zms, zev.e[0], zev.e[1]) == hipSuccess) deflate_ms += zms;
            for (int k = 0; k < 2; k++)
                if (bgzf >> k & 1)
                    if (const char *m = enc[k].collect(slot, bytes, &src[k], &job_bytes[k])) return gfail(NGSQ_ERR_STATE, "%s", m);
        }
        GHIP(slots.submit(w, 2, src, job_bytes, st));
        write_pending = true;
        text_bytes += bytes;
        return NGSQ_OK;
    };
    int rc = NGSQ_OK;
    while (rc == NGSQ_OK && done < n_pairs && bad == ~0ull && !w[0].failed() && !w[1].failed()) {
        const uint64_t n = std::min(batch_pairs, n_pairs - done);
        rc = batch(first_pair + done, n);
        if (rc == NGSQ_OK && bad == ~0ull) done += n;
    }
    if (rc == NGSQ_OK) {
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = gfail(NGSQ_ERR_DEVICE, "hipStreamSynchronize: %s", hipGetErrorString(e));
        add_write_time();
    }
    const WriterEnd end[2] = {w[0].end(), w[1].end()};
    for (int k = 0; k < 2 && rc == NGSQ_OK; k++) {
        if (end[k].herr != hipSuccess) rc = gfail(NGSQ_ERR_DEVICE, "copying the FASTQ text to the host: %s", hipGetErrorString(end[k].herr));
        else if (end[k].werr) rc = write_failed(k, end[k].werr);
    }
    for (int k = 0; k < 2 && rc == NGSQ_OK && bad == ~0ull; k++)
        if (bgzf >> k & 1) {
            rc = write_eof(k);
            enc[k].comp_bytes += sizeof BGZF_EOF_BLOCK;
        }
    if (ext) {
        ext->compressed_bytes_one = enc[0].comp_bytes;
        ext->compressed_bytes_two = enc[1].comp_bytes;
        ext->blocks = enc[0].blocks + enc[1].blocks;
        ext->stored_blocks = enc[0].stored + enc[1].stored;
        ext->deflate_ms = deflate_ms;
    }
    if (rc == NGSQ_OK && bad != ~0ull) {
        const uint64_t pair = bad >> GEN_ERR_BITS;
        // which provider: the pair's first draw, as k_gen_draw makes it
        const uint64_t xw = (uint64_t)(((unsigned __int128)ngsq_generate_draw(seed, pair, 0, 0) * g->total_weight) >> 64);
        size_t p = 0;
        uint64_t end = 0;
        for (; p + 1 < g->prov.size(); p++)
            if ((end += g->prov[p]->p.weight) > xw) break;
        rc = gfail(NGSQ_ERR_INVALID_ARGUMENT,
                   "no read pair could be drawn from %s for pair %llu in %u attempts: either the sequences are almost all N (a fragment may hold "
                   "nothing but A, C, G and T), or the inner distances are too long for the sequences (a fragment must end inside its sequence)",
                   g->prov[p]->fname.c_str(), (unsigned long long)pair, NGSQ_GENERATE_MAX_ATTEMPTS);
    }
    if (out) {
        out->pairs = done;
        out->rejected_start = rej[0];
        out->rejected_end = rej[1];
        out->rejected_base = rej[2];
        out->text_bytes_one = out->text_bytes_two = text_bytes;
        out->batches = slots.jobs;
        out->draw_ms = draw_ms;
        out->format_ms = format_ms;
        out->copy_ms = w[0].copy_ms + w[1].copy_ms;
        out->write_ms = w[0].write_ms + w[1].write_ms;
        out->total_ms = now_ms() - t_begin;
    }
    return rc;
}

int ngsq_generate_write(ngsq_generate *g, int fd_one, int fd_two, uint64_t seed, uint64_t first_pair, uint64_t n_pairs, uint64_t batch_pairs,
                        ngsq_generate_report *out) {
    return generate_write(g, fd_one, fd_two, seed, first_pair, n_pairs, batch_pairs, out, 0, nullptr);
}

int ngsq_generate_write_bgzf(ngsq_generate *g, int fd_one, int fd_two, uint64_t seed, uint64_t first_pair, uint64_t n_pairs, uint64_t batch_pairs,
                             uint32_t flags, ngsq_generate_bgzf_report *out) {
    if (out) memset(out, 0, sizeof *out);
    if (flags & ~(NGSQ_GENERATE_PLAIN_ONE | NGSQ_GENERATE_PLAIN_TWO)) return gfail(NGSQ_ERR_INVALID_ARGUMENT, "unknown flags 0x%x", flags);
    return generate_write(g, fd_one, fd_two, seed, first_pair, n_pairs, batch_pairs, out ? &out->text : nullptr, 3u & ~flags, out);
}

} // extern "C"
