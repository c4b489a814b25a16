// cli.h -- what the commands of `ngs` share: the log, the error exit, option helpers, file-format sniffing, and the
// reader plus facet-less context that `index`, `convert`, `derive`, `view`, `depth`, `fastq` and `markdup` walk a file with.  One file per command beside it:
// qc.cpp, index.cpp, convert.cpp, derive.cpp, view.cpp, generate.cpp, depth.cpp, fastq.cpp, markdup.cpp; ngs_main.cpp dispatches.  The command line includes the library's public headers only.
#pragma once

#include <unistd.h>

#include <cerrno>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/ngsq.h"
#include "../../../include/ngsq_bam.h"
#include "../../../include/ngsq_comm.h"

// the commands: argv[at] is the command's name; the return value is the process's exit status
int qc_main(int argc, char **argv);
int index_main(int argc, char **argv, int at);
int convert_main(int argc, char **argv, int at);
int derive_main(int argc, char **argv, int at);
int view_main(int argc, char **argv, int at);
int generate_main(int argc, char **argv, int at);
int depth_main(int argc, char **argv, int at);
int fastq_main(int argc, char **argv, int at);
int markdup_main(int argc, char **argv, int at);

inline int g_level = 2; // 0 off (-q), 2 info (default), 3 debug (-v)   src/main.rs:71-83

// -q / --quiet / -v / --verbose, wherever they stand: true when `s` was one of them
inline bool verbosity_option(const char *s) {
    if (!strcmp(s, "-q") || !strcmp(s, "--quiet")) g_level = 0;
    else if (!strcmp(s, "-v") || !strcmp(s, "--verbose")) g_level = 3;
    else return false;
    return true;
}

inline void logf(int level, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
inline void logf(int level, const char *fmt, ...) {
    if (level > g_level) return;
    char ts[64];
    const auto now = std::chrono::system_clock::now();
    const std::time_t t = std::chrono::system_clock::to_time_t(now);
    std::tm tm{};
    gmtime_r(&t, &tm);
    const long us = (long)(std::chrono::duration_cast<std::chrono::microseconds>(now.time_since_epoch()).count() % 1000000);
    strftime(ts, sizeof ts, "%Y-%m-%dT%H:%M:%S", &tm);
    fprintf(stderr, "%s.%06ldZ %5s ngs::qc::command: ", ts, us, level <= 1 ? "ERROR" : level == 2 ? "INFO" : "DEBUG");
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}

[[noreturn]] inline void bail(const std::string &msg) { // anyhow::bail! -> "Error: ..." and exit code 1
    fprintf(stderr, "Error: %s\n", msg.c_str());
    if (ngsq_comm_rccl_stuck()) { // a thread is still inside ncclCommInitRank: the exit handlers may wait for it
        fflush(nullptr);
        _exit(1);
    }
    exit(1);
}

// the value of option argv[*i], which `name` names in the message; *i moves on to it
inline std::string option_value(int argc, char **argv, int *i, const char *name) {
    if (*i + 1 >= argc) bail(std::string("a value is required for '") + name + "' but none was supplied");
    return argv[++*i];
}

// a size: decimal digits with an optional K, M or G, powers of 1024 (as `samtools sort -m` reads its value), at least one byte;
// `name` names the option in the message
inline unsigned long long size_value(const std::string &v, const char *name) {
    const std::string what = "invalid value '" + v + "' for '" + name + "': ";
    size_t d = 0;
    while (d < v.size() && v[d] >= '0' && v[d] <= '9') d++;
    if (!d) bail(what + "a size is decimal digits with an optional K, M or G suffix");
    unsigned shift = 0;
    if (d + 1 == v.size() && (v[d] == 'K' || v[d] == 'k')) shift = 10;
    else if (d + 1 == v.size() && (v[d] == 'M' || v[d] == 'm')) shift = 20;
    else if (d + 1 == v.size() && (v[d] == 'G' || v[d] == 'g')) shift = 30;
    else if (d != v.size()) bail(what + "a size is decimal digits with an optional K, M or G suffix");
    errno = 0;
    const unsigned long long digits = strtoull(v.substr(0, d).c_str(), nullptr, 10);
    if (errno || digits > (~0ull >> shift)) bail(what + "number too large to fit in target type");
    if (!digits) bail(what + "a size is at least one byte");
    return digits << shift;
}

inline std::string with_commas(unsigned long long v) { // num_format Locale::en
    std::string s = std::to_string(v), out;
    for (size_t i = 0; i < s.size(); i++) {
        out += s[i];
        const size_t left = s.size() - 1 - i;
        if (left && left % 3 == 0) out += ',';
    }
    return out;
}

inline bool ieq(const std::string &a, const std::string &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (tolower((unsigned char)a[i]) != tolower((unsigned char)b[i])) return false;
    return true;
}

// cores the command may use: the cgroup's CPU quota when there is one (as the library's readers count them)
inline int cgroup_cores() {
    int n = (int)std::thread::hardware_concurrency();
    if (n < 1) n = 1;
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char quota[32] = {0};
        long period = 0;
        if (fscanf(f, "%31s %ld", quota, &period) == 2 && strcmp(quota, "max") != 0 && period > 0) {
            const long q = atol(quota) / period;
            if (q >= 1 && q < n) n = (int)q;
        }
        fclose(f);
    }
    return n;
}

inline bool trace_on() { // NGSQ_INGEST_TRACE=1 (measurement aid)
    static const bool on = getenv("NGSQ_INGEST_TRACE") && atoi(getenv("NGSQ_INGEST_TRACE"));
    return on;
}

// NGSQ_INGEST_TRACE=1: wall clock of the command's stages on stderr, from the first call on
inline void milestone(const char *what) {
    static const auto t0 = std::chrono::steady_clock::now();
    if (trace_on()) fprintf(stderr, "[ngs] %8.1f ms  %s\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), what);
}

// utils/formats.rs:117-186  BioinformaticsFileFormat::try_detect, with the names its Display prints (:79-101).
// "" = no format (the callers then report the extension).  `.gz` / `.bgz` look at the whole name, case-sensitively,
// the other extensions are matched case-insensitively -- as the reference does.
inline std::string detect_format(const std::string &path) {
    auto ends_with = [&](const char *suf) {
        const size_t n = strlen(suf);
        return path.size() >= n && path.compare(path.size() - n, n, suf) == 0;
    };
    const size_t slash = path.rfind('/');
    const size_t dot = path.rfind('.');
    if (dot == std::string::npos || (slash != std::string::npos && dot < slash) || dot + 1 == path.size() ||
        dot == (slash == std::string::npos ? 0 : slash + 1))
        return ""; // no extension (a leading dot is not one)
    std::string ext = path.substr(dot + 1);
    for (auto &c : ext) c = (char)tolower((unsigned char)c);
    if (ext == "bgz") {
        if (ends_with("gff.bgz") || ends_with("gff3.bgz")) return "Block-gzipped GFF";
    } else if (ext == "gz") {
        if (ends_with("fasta.gz") || ends_with("fna.gz") || ends_with("fa.gz")) return "Gzipped FASTA";
        if (ends_with("fq.gz") || ends_with("fastq.gz")) return "Gzipped FASTQ";
        if (ends_with("vcf.gz")) return "Gzipped VCF";
        if (ends_with("gff.gz") || ends_with("gff3.gz")) return "Gzipped GFF";
        if (ends_with("gtf.gz")) return "Gzipped GTF";
        return "";
    }
    static const struct { const char *ext, *name; } table[] = {
        {"fasta", "FASTA"}, {"fna", "FASTA"}, {"fa", "FASTA"}, {"fastq", "FASTQ"}, {"fq", "FASTQ"}, {"sam", "SAM"},
        {"ubam", "Unaligned BAM"}, {"bam", "BAM"}, {"cram", "CRAM"}, {"vcf", "VCF"}, {"bcf", "BCF"}, {"gff", "GFF"},
        {"gff3", "GFF"}, {"gtf", "GTF"}, {"bed", "BED"}};
    for (const auto &t : table)
        if (ext == t.ext) return t.name;
    return "";
}

// what follows the last dot of a path, for the messages about a file without a known format
inline std::string extension_of(const std::string &path) {
    const size_t dot = path.rfind('.');
    return dot == std::string::npos ? "" : path.substr(dot + 1);
}

// A context without facets on `device` for the @SQ lengths of an open reader: what `index`, `convert` and `derive` walk a file with.
// nullptr: no context (ngsq_last_global_error says why).
inline ngsq_ctx *plain_context(const ngsq_bam *bam, int device) {
    const uint32_t n_refs = ngsq_bam_n_refs(bam);
    std::vector<uint32_t> lens(n_refs);
    for (uint32_t r = 0; r < n_refs; r++) lens[r] = ngsq_bam_ref_len(bam, r);
    ngsq_config cfg{};
    cfg.struct_size = sizeof cfg;
    cfg.facets = 0;
    cfg.device = device;
    cfg.n_refs = n_refs;
    cfg.ref_len = lens.data();
    ngsq_ctx *ctx = nullptr;
    return ngsq_create(&cfg, &ctx) == NGSQ_OK ? ctx : nullptr;
}
