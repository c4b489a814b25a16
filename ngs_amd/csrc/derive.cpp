// derive.cpp -- ngsq_bam_derive_instrument, ngsq_derive_lookup and ngsq_derive_predict (include/ngsq_derive.h): the device
// ingest hands out the file's records batch by batch, derive_kernel.hip collects the instrument ids and flowcell ids of
// their names into two exact sets on the device, and the host reads the appended strings once at the end.  The sequencer
// is predicted on the host from this file's own tables of name patterns.  DESIGN.md section 14.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../include/ngsq_derive.h"
#include "context.h"
#include "derive_kernels.h"
#include "device_out.h"
#include "ingest_consumer.h"

using namespace ngsq;

struct ngsq_derive_names {
    std::vector<std::string> set[2];
};

namespace {

constexpr uint64_t BATCH_RECORDS = (uint64_t)1 << 22;

// ---- the pattern tables ----------------------------------------------------------------------
// A pattern: the literal `prefix`, then lo..hi characters of a class, then the literal `suffix`, then a tail, then the end
// of the text.  OPEN has nothing behind its prefix, not even the end: any text that starts with it matches.
enum Cls : uint8_t { DIGITS, UPPER_DIGITS };                     // [0-9] | [A-Z0-9]
enum Tail : uint8_t { END, OPEN, OPT_UNDERSCORE_9_DIGITS, ONE_UPPER_COMMA_DIGIT }; // $ | nothing | (_[0-9]{9})?$ | [A-Z,0-9]$
struct Pattern {
    const char *prefix;
    Cls cls;
    uint8_t lo, hi;
    const char *suffix;
    Tail tail;
    const char *machines[4];
};

const Pattern INSTRUMENTS[] = {
    {"HWI-M", DIGITS, 4, 4, "", END, {"MiSeq"}},
    {"HWUSI", DIGITS, 0, 0, "", OPEN, {"Genome Analyzer IIx"}},
    {"M", DIGITS, 5, 5, "", END, {"MiSeq"}},
    {"HWI-C", DIGITS, 5, 5, "", END, {"HiSeq 1500"}},
    {"C", DIGITS, 5, 5, "", END, {"HiSeq 1500"}},
    {"HWI-ST", DIGITS, 3, 5, "", OPT_UNDERSCORE_9_DIGITS, {"HiSeq 2000"}},
    {"HWI-D", DIGITS, 5, 5, "", END, {"HiSeq 2000", "HiSeq 2500"}},
    {"A", DIGITS, 5, 5, "", END, {"NovaSeq"}},
    {"D", DIGITS, 5, 5, "", END, {"HiSeq 2500"}},
    {"J", DIGITS, 5, 5, "", END, {"HiSeq 3000"}},
    {"K", DIGITS, 5, 5, "", END, {"HiSeq 3000", "HiSeq 4000"}},
    {"E", DIGITS, 5, 5, "", END, {"HiSeq X"}},
    {"N", DIGITS, 5, 5, "", END, {"NextSeq"}},
    {"NB", DIGITS, 6, 6, "", END, {"NextSeq"}},
    {"NS", DIGITS, 6, 6, "", END, {"NextSeq"}},
    {"MN", DIGITS, 5, 5, "", END, {"MiniSeq"}},
};

const Pattern FLOWCELLS[] = {
    {"C", UPPER_DIGITS, 4, 4, "ANXX", END, {"HiSeq 1500", "HiSeq 2000", "HiSeq 2500"}},               // high output (8-lane) v4
    {"C", UPPER_DIGITS, 4, 4, "ACXX", END, {"HiSeq 1000", "HiSeq 1500", "HiSeq 2000", "HiSeq 2500"}}, // high output (8-lane) v3
    {"D", UPPER_DIGITS, 4, 4, "ACXX", END, {"HiSeq 1000", "HiSeq 1500", "HiSeq 2000", "HiSeq 2500"}},
    {"H", UPPER_DIGITS, 4, 4, "ADXX", END, {"HiSeq 1500", "HiSeq 2000", "HiSeq 2500"}}, // rapid run (2-lane) v1
    {"H", UPPER_DIGITS, 4, 4, "BCXX", END, {"HiSeq 1500", "HiSeq 2500"}},               // rapid run (2-lane) v2
    {"H", UPPER_DIGITS, 4, 4, "BCXY", END, {"HiSeq 1500", "HiSeq 2500"}},
    {"H", UPPER_DIGITS, 4, 4, "BBXX", END, {"HiSeq 4000"}}, // (8-lane) v1
    {"H", UPPER_DIGITS, 4, 4, "BBXY", END, {"HiSeq 4000"}},
    {"H", UPPER_DIGITS, 4, 4, "CCXX", END, {"HiSeq X"}}, // (8-lane)
    {"H", UPPER_DIGITS, 4, 4, "CCXY", END, {"HiSeq X"}},
    {"H", UPPER_DIGITS, 4, 4, "ALXX", END, {"HiSeq X"}},
    {"H", UPPER_DIGITS, 4, 4, "BGX", ONE_UPPER_COMMA_DIGIT, {"NextSeq"}}, // high output
    {"H", UPPER_DIGITS, 4, 4, "AFXX", END, {"NextSeq"}},                  // mid output
    {"H", UPPER_DIGITS, 5, 5, "RXX", END, {"NovaSeq"}},                   // S1 and SP
    {"H", UPPER_DIGITS, 5, 5, "MXX", END, {"NovaSeq"}},                   // S2
    {"H", UPPER_DIGITS, 5, 5, "SXX", END, {"NovaSeq"}},                   // S4
    {"A", UPPER_DIGITS, 4, 4, "", END, {"MiSeq"}},
    {"B", UPPER_DIGITS, 4, 4, "", END, {"MiSeq"}},
    {"D", UPPER_DIGITS, 4, 4, "", END, {"MiSeq"}}, // nano
    {"G", UPPER_DIGITS, 4, 4, "", END, {"MiSeq"}}, // micro
};

inline bool is_digit(unsigned char c) { return c >= '0' && c <= '9'; }
inline bool is_upper(unsigned char c) { return c >= 'A' && c <= 'Z'; }
inline bool in_class(Cls k, unsigned char c) { return is_digit(c) || (k == UPPER_DIGITS && is_upper(c)); }

// what stands behind the class characters: the suffix, the tail, the end of the text
bool rest_matches(const Pattern &p, const unsigned char *s, size_t n) {
    const size_t ls = strlen(p.suffix);
    if (n < ls || memcmp(s, p.suffix, ls) != 0) return false;
    s += ls;
    n -= ls;
    switch (p.tail) {
    case END: return n == 0;
    case OPEN: return true;
    case OPT_UNDERSCORE_9_DIGITS:
        if (n == 0) return true;
        if (n != 10 || s[0] != '_') return false;
        for (size_t k = 1; k < 10; k++)
            if (!is_digit(s[k])) return false;
        return true;
    case ONE_UPPER_COMMA_DIGIT: return n == 1 && (is_upper(s[0]) || is_digit(s[0]) || s[0] == ',');
    }
    return false;
}

bool matches(const Pattern &p, const unsigned char *s, size_t n) {
    const size_t lp = strlen(p.prefix);
    if (n < lp || memcmp(s, p.prefix, lp) != 0) return false;
    s += lp;
    n -= lp;
    for (size_t c = 0; c <= p.hi; c++) { // c characters of the class, every count the pattern allows
        if (c >= p.lo && rest_matches(p, s + c, n - c)) return true;
        if (c == n || !in_class(p.cls, s[c])) break;
    }
    return false;
}

using Machines = std::set<std::string>;

Machines machines_for(int which, const char *q, uint32_t len) {
    Machines out;
    const Pattern *tab = which == NGSQ_DERIVE_FLOWCELLS ? FLOWCELLS : INSTRUMENTS;
    const size_t n = which == NGSQ_DERIVE_FLOWCELLS ? sizeof FLOWCELLS / sizeof *FLOWCELLS : sizeof INSTRUMENTS / sizeof *INSTRUMENTS;
    for (size_t k = 0; k < n; k++)
        if (matches(tab[k], reinterpret_cast<const unsigned char *>(q), len))
            for (const char *m : tab[k].machines)
                if (m) out.insert(m);
    return out;
}

// compute.rs:141-153 with :25-42: the intersection of the queries' machines; `any`: some query had a machine
struct Detection {
    Machines possible;
    bool any = false;
};
Detection detect(int which, const char *const *names, const uint32_t *lens, uint64_t n) {
    Detection d;
    std::set<std::string> seen;
    bool first = true;
    for (uint64_t k = 0; k < n; k++) {
        const std::string q(names[k] ? names[k] : "", lens[k]);
        if (!seen.insert(q).second) continue;
        const Machines m = machines_for(which, q.data(), (uint32_t)q.size());
        if (first) {
            d.possible = m;
        } else {
            Machines both;
            std::set_intersection(d.possible.begin(), d.possible.end(), m.begin(), m.end(), std::inserter(both, both.begin()));
            d.possible.swap(both);
        }
        first = false;
        if (!m.empty()) d.any = true;
    }
    return d;
}

struct Verdict {
    bool succeeded;
    const Machines *instruments; // null: None
    const char *confidence, *evidence, *comment; // null: None
};

std::string document(const Verdict &v) {
    auto text = [](const char *s) { return s ? "\"" + std::string(s) + "\"" : std::string("null"); };
    std::string o = "{\n  \"succeeded\": ";
    o += v.succeeded ? "true" : "false";
    o += ",\n  \"instruments\": ";
    if (!v.instruments) {
        o += "null";
    } else if (v.instruments->empty()) {
        o += "[]";
    } else {
        o += "[";
        bool first = true;
        for (const std::string &m : *v.instruments) {
            o += first ? "\n    \"" : ",\n    \"";
            o += m + "\"";
            first = false;
        }
        o += "\n  ]";
    }
    o += ",\n  \"confidence\": " + text(v.confidence);
    o += ",\n  \"evidence\": " + text(v.evidence);
    o += ",\n  \"comment\": " + text(v.comment);
    o += "\n}";
    return o;
}

int give_text(const std::string &s, char *out, size_t cap, size_t *need) {
    if (need) *need = s.size() + 1;
    if (!out || cap < s.size() + 1) return NGSQ_ERR_BUFFER_TOO_SMALL;
    memcpy(out, s.data(), s.size());
    out[s.size()] = 0;
    return NGSQ_OK;
}

} // namespace

extern "C" int ngsq_derive_lookup(int which, const char *query, uint32_t len, char *out, size_t cap, size_t *need) {
    if ((which != NGSQ_DERIVE_INSTRUMENTS && which != NGSQ_DERIVE_FLOWCELLS) || (!query && len)) return NGSQ_ERR_INVALID_ARGUMENT;
    std::string s;
    for (const std::string &m : machines_for(which, query, len)) s += m + "\n";
    return give_text(s, out, cap, need);
}

// compute.rs:157-267, case by case
extern "C" int ngsq_derive_predict(const char *const *instruments, const uint32_t *instrument_lens, uint64_t n_instruments,
                                   const char *const *flowcells, const uint32_t *flowcell_lens, uint64_t n_flowcells, char *json, size_t cap,
                                   size_t *need) {
    if ((n_instruments && (!instruments || !instrument_lens)) || (n_flowcells && (!flowcells || !flowcell_lens)))
        return NGSQ_ERR_INVALID_ARGUMENT;
    const Detection iid = detect(NGSQ_DERIVE_INSTRUMENTS, instruments, instrument_lens, n_instruments);
    const Detection fcid = detect(NGSQ_DERIVE_FLOWCELLS, flowcells, flowcell_lens, n_flowcells);
    Machines both;
    Verdict v;
    if (iid.possible.empty() && iid.any) {
        v = {false, nullptr, "unknown", "instrument id", "multiple instruments were detected in this file via the instrument id"};
    } else if (fcid.possible.empty() && fcid.any) {
        v = {false, nullptr, "unknown", "flowcell id", "multiple instruments were detected in this file via the flowcell id"};
    } else if (iid.possible.empty() && fcid.possible.empty()) {
        v = {false, nullptr, "unknown", nullptr, "no matching instruments were found"};
    } else if (iid.possible.empty()) {
        v = {true, &fcid.possible, fcid.possible.size() == 1 ? "medium" : "low", "flowcell id", nullptr};
    } else if (fcid.possible.empty()) {
        v = {true, &iid.possible, iid.possible.size() == 1 ? "medium" : "low", "instrument id", nullptr};
    } else {
        std::set_intersection(fcid.possible.begin(), fcid.possible.end(), iid.possible.begin(), iid.possible.end(),
                              std::inserter(both, both.begin()));
        if (both.empty())
            v = {false, nullptr, "high", "instrument and flowcell id",
                 "Case needs triaging, results from instrument id and flowcell id are mutually exclusive."};
        else v = {true, &both, "high", "instrument and flowcell id", nullptr};
    }
    return give_text(document(v), json, cap, need);
}

extern "C" uint64_t ngsq_derive_names_count(const ngsq_derive_names *names, int which) {
    return names && (which == 0 || which == 1) ? names->set[which].size() : 0;
}

extern "C" const char *ngsq_derive_names_get(const ngsq_derive_names *names, int which, uint64_t i, uint32_t *len) {
    if (!names || (which != 0 && which != 1) || i >= names->set[which].size()) return nullptr;
    if (len) *len = (uint32_t)names->set[which][i].size();
    return names->set[which][i].data();
}

extern "C" void ngsq_derive_names_free(ngsq_derive_names *names) { delete names; }

extern "C" int ngsq_bam_derive_instrument(ngsq_bam *b, ngsq_ctx *c, uint64_t max_records, uint64_t batch_records, uint32_t table_slots,
                                          ngsq_derive_names **out, ngsq_derive_report *rep) {
    if (!b || !c || !out) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (rep) memset(rep, 0, sizeof *rep);
    const uint32_t slots = table_slots ? table_slots : NGSQ_DERIVE_TABLE_SLOTS;
    if (slots & (slots - 1)) return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "table_slots must be a power of two: %u", table_slots);
    if (const int rc = require_fresh_reader(b, "the instrument is derived")) return rc;
    if (!batch_records) batch_records = BATCH_RECORDS;
    const double t_begin = now_ms();
    BHIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    // ---- device state: the two tables, the arena, the entry list, the scan's words
    DevArray<DeriveSlot> d_table;
    DevArray<uint8_t> d_arena;
    DevArray<DeriveEntry> d_entries;
    DevArray<DeriveState> d_state;
    BHIP(d_table.reserve(2 * (size_t)slots));
    BHIP(d_arena.reserve(NGSQ_DERIVE_ARENA_BYTES));
    BHIP(d_entries.reserve(NGSQ_DERIVE_MAX_ENTRIES));
    BHIP(d_state.reserve(1));
    DeriveState s0;
    memset(&s0, 0, sizeof s0);
    s0.bad = ~0ull;
    BHIP(hipMemsetAsync(d_table.p, 0, 2 * (size_t)slots * sizeof(DeriveSlot), st));
    BHIP(hipMemcpyAsync(d_state.p, &s0, sizeof s0, hipMemcpyHostToDevice, st));
    BHIP(hipStreamSynchronize(st)); // (s0 leaves scope with this call)
    DeriveSets S;
    S.table[0] = d_table.p;
    S.table[1] = d_table.p + slots;
    S.slots = slots;
    S.arena = d_arena.p;
    S.arena_cap = NGSQ_DERIVE_ARENA_BYTES;
    S.entries = d_entries.p;
    S.entries_cap = NGSQ_DERIVE_MAX_ENTRIES;
    S.state = d_state.p;
    MappedBuf pin;
    BHIP(pin.reserve(DERIVE_HOST_WORDS * sizeof(unsigned long long)));
    memset(pin.h, 0, DERIVE_HOST_WORDS * sizeof(unsigned long long));
    static_cast<unsigned long long *>(pin.h)[0] = ~0ull;
    const unsigned long long *const pin_h = static_cast<const unsigned long long *>(pin.h);
    HipEvents<2> ev; // around a batch's kernel
    BHIP(hipEventCreate(&ev.e[0]));
    BHIP(hipEventCreate(&ev.e[1]));
    // every way out below waits for the stream first: the arrays above go back to the block cache when they leave scope
    StreamDrain drain{st};
    // ---- the scan: every batch of the device ingest, in file order
    uint64_t records = 0, batches = 0;
    double scan_ms = 0, kernel_ms = 0;
    bool pending = false; // a batch's kernels are queued whose words the host has not read yet
    // The words of the batch launched last.  All batches in front of it were clean, so a bad index it reports is the file's
    // first, and the name beside it was copied on the device while the batch's bytes were still there.
    auto read_pending = [&]() -> int {
        if (!pending) return NGSQ_OK;
        pending = false;
        BHIP(hipEventSynchronize(ev.e[1]));
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.e[0], ev.e[1]) == hipSuccess) kernel_ms += ms;
        if (pin_h[0] != ~0ull)
            return ngsq_bam_fail(NGSQ_ERR_INVALID_ARGUMENT, "Could not parse Illumina-formatted query names for read: %.*s", (int)pin_h[2],
                                 reinterpret_cast<const char *>(pin_h + 4));
        if (pin_h[1])
            return ngsq_bam_fail(NGSQ_ERR_LIMIT, "%s: more distinct instrument or flowcell names than one scan holds (%u bytes, %u strings)",
                                 b->path.c_str(), NGSQ_DERIVE_ARENA_BYTES, NGSQ_DERIVE_MAX_ENTRIES);
        return NGSQ_OK;
    };
    for (;;) {
        const uint64_t left = max_records ? max_records - records : ~0ull;
        if (!left) break;
        ngsq_batch bt;
        BatchOrigin o;
        const double s_begin = now_ms();
        const int rc = next_batch_with_origin(b, c, std::min(batch_records, left), &bt, &o);
        scan_ms += now_ms() - s_begin;
        if (rc) return rc;
        // (the ingest has waited for its own kernels, queued behind the last batch's: this returns at once)
        if (const int rp = read_pending()) return rp;
        const uint64_t n = bt.n_records;
        if (!n) break;
        BHIP(hipEventRecord(ev.e[0], st));
        BHIP(launch_derive_names(bt, o, records, (uint32_t)(batches + 1), S, static_cast<unsigned long long *>(pin.dev), st));
        BHIP(hipEventRecord(ev.e[1], st));
        pending = true;
        records += n;
        batches++;
    }
    if (const int rp = read_pending()) return rp;
    // ---- the end: the appended strings to the host, de-duplicated exactly
    DeriveState fin;
    BHIP(hipMemcpyAsync(&fin, d_state.p, sizeof fin, hipMemcpyDeviceToHost, st));
    BHIP(hipStreamSynchronize(st));
    const uint64_t n_entries = fin.n_entries, arena_used = fin.arena_used;
    if (fin.overflow || n_entries > NGSQ_DERIVE_MAX_ENTRIES || arena_used > NGSQ_DERIVE_ARENA_BYTES)
        return ngsq_bam_fail(NGSQ_ERR_LIMIT, "%s: more distinct instrument or flowcell names than one scan holds (%u bytes, %u strings)",
                             b->path.c_str(), NGSQ_DERIVE_ARENA_BYTES, NGSQ_DERIVE_MAX_ENTRIES);
    std::vector<DeriveEntry> entries(n_entries);
    std::vector<char> arena(arena_used);
    if (n_entries) BHIP(hipMemcpyAsync(entries.data(), d_entries.p, n_entries * sizeof(DeriveEntry), hipMemcpyDeviceToHost, st));
    if (arena_used) BHIP(hipMemcpyAsync(arena.data(), d_arena.p, arena_used, hipMemcpyDeviceToHost, st));
    BHIP(hipStreamSynchronize(st));
    std::set<std::string> sets[2];
    uint64_t candidates = 0;
    for (const DeriveEntry &e : entries) {
        if ((uint64_t)e.off + e.len > arena_used) return ngsq_bam_fail(NGSQ_ERR_DEVICE, "%s: a derive entry lies outside the arena", b->path.c_str());
        if (e.set & DERIVE_CANDIDATE) candidates++;
        sets[e.set & 1u].insert(std::string(arena.data() + e.off, e.len));
    }
    ngsq_derive_names *names = new ngsq_derive_names;
    for (int k = 0; k < 2; k++) names->set[k].assign(sets[k].begin(), sets[k].end());
    *out = names;
    if (rep) {
        rep->records = records;
        rep->skipped = fin.skipped;
        rep->instruments = names->set[0].size();
        rep->flowcells = names->set[1].size();
        rep->entries = n_entries;
        rep->candidates = candidates;
        rep->batches = batches;
        rep->scan_ms = scan_ms;
        rep->kernel_ms = kernel_ms;
        rep->total_ms = now_ms() - t_begin;
    }
    return NGSQ_OK;
}
