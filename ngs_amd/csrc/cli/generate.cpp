// generate.cpp -- `ngs generate` (src/generate/command.rs:30-131): paired FASTQ reads sampled from one or
// more reference FASTAs, drawn and written as text on the GPU by ngsq_generate_write (include/ngsq_generate.h).
#include <fcntl.h>

#include <cerrno>
#include <cmath>
#include <memory>

#include "../../../include/ngsq_bgzf.h"
#include "../../../include/ngsq_generate.h"
#include "cli.h"

namespace {

struct GenerateArgs {
    std::vector<std::string> pos;
    bool has_n = false, has_c = false, has_seed = false;
    unsigned long long n = 0, coverage = 0, seed = 0, batch_pairs = 0;
    int device = 0;
    bool gzip_device = false; // --gzip device: .gz outputs are BGZF written on the GPU
    bool has_effort = false;  // --gzip-effort: how hard the GPU's encoder searches
    uint32_t effort = NGSQ_BGZF_EFFORT_NORMAL;
};

const char *const USAGE = "Usage: ngs generate [OPTIONS] <--num-records <USIZE>|--coverage <USIZE>> <READ_ONES_FILE> <READ_TWOS_FILE> <REFERENCE_PROVIDERS>...";

unsigned long long usize_value(const std::string &v, const char *name) {
    char *e = nullptr;
    errno = 0;
    const unsigned long long x = strtoull(v.c_str(), &e, 10);
    if (v.empty() || *e || errno || v[0] == '-' || (v[0] == '+' && v.size() == 1) || isspace((unsigned char)v[0]))
        bail("invalid value '" + v + "' for '" + name + "': invalid digit found in string");
    return x;
}

// command.rs:19-28 error_rate_in_range
void check_error_rate(const std::string &raw) {
    char *e = nullptr;
    const float x = raw.empty() || isspace((unsigned char)raw[0]) ? 0.f : strtof(raw.c_str(), &e);
    const bool hex = raw.find_first_of("xXpP") != std::string::npos; // (Rust's parse takes no hexadecimal floats)
    if (!e || *e || e == raw.c_str() || hex) bail("invalid value '" + raw + "' for '--error-rate <F32>': " + raw + " isn't a float");
    if (!(x >= 0.f && x <= 1.f)) bail("invalid value '" + raw + "' for '--error-rate <F32>': Error rate must be between 0.0 and 1.0");
}

// false: --help has been answered
bool parse_args(int argc, char **argv, int at, GenerateArgs *a) {
    for (int i = at + 1; i < argc; i++) {
        const std::string s = argv[i];
        auto val = [&](const char *name) { return option_value(argc, argv, &i, name); };
        if (verbosity_option(argv[i])) continue;
        if (s == "-h" || s == "--help") {
            fprintf(stderr,
                    "Generates a BAM file from a given reference genome\n\n%s\n\n"
                    "Arguments:\n"
                    "  <READ_ONES_FILE>          Destination for the FASTQ file containing all read ones\n"
                    "  <READ_TWOS_FILE>          Destination for the FASTQ file containing all read twos\n"
                    "  <REFERENCE_PROVIDERS>...  One or more reference FASTAs to generate the data based off of,\n"
                    "                            each as PATH:ERROR_FREQ:MU:SIGMA:READ_LENGTH:WEIGHT\n\n"
                    "Options:\n"
                    "  -e, --error-rate <F32>\n"
                    "          The error rate for the sequencer as a fraction between [0.0, 1.0] (per base) [default: 0.0001]\n"
                    "          (checked and then unused, as in the reference: a provider's ERROR_FREQ sets the substitutions)\n"
                    "  -n, --num-records <USIZE>\n"
                    "          Specifies the number of records to generate\n"
                    "  -c, --coverage <USIZE>\n"
                    "          Dynamically calculate the number of reads needed for a particular mean coverage\n"
                    "      --seed <U64>\n"
                    "          The seed of every draw: the same seed gives the same two files (additive, this build)\n"
                    "          [default: from the clock and the process id, logged]\n"
                    "      --device <N>\n"
                    "          GPU the pairs are drawn and written on (additive, this build) [default: 0]\n"
                    "      --batch-pairs <N>\n"
                    "          Pairs per launch; the output does not depend on it (additive, this build)\n"
                    "      --gzip <WHERE>\n"
                    "          Where gzipped outputs are compressed (additive, this build): host threads behind a pipe, or the GPU,\n"
                    "          which writes BGZF and sends only compressed bytes to the host; plain outputs are not affected\n"
                    "          [default: host] [possible values: host, device]\n"
                    "      --gzip-effort <EFFORT>\n"
                    "          With --gzip device (additive, this build): `high` has the GPU's encoder search harder for matches, which\n"
                    "          gives smaller files for more encoder time [default: normal] [possible values: normal, high]\n\n"
                    "Outputs are FASTQ (.fastq, .fq) or gzipped FASTQ (.fastq.gz, .fq.gz).\n",
                    USAGE);
            return false;
        } else if (s == "-e" || s == "--error-rate") {
            check_error_rate(val("--error-rate <F32>"));
        } else if (s == "-n" || s == "--num-records") {
            a->n = usize_value(val("--num-records <USIZE>"), "--num-records <USIZE>");
            a->has_n = true;
        } else if (s == "-c" || s == "--coverage") {
            a->coverage = usize_value(val("--coverage <USIZE>"), "--coverage <USIZE>");
            a->has_c = true;
        } else if (s == "--seed") {
            a->seed = usize_value(val("--seed <U64>"), "--seed <U64>");
            a->has_seed = true;
        } else if (s == "--batch-pairs") {
            a->batch_pairs = usize_value(val("--batch-pairs <N>"), "--batch-pairs <N>");
        } else if (s == "--gzip") {
            const std::string v = val("--gzip <WHERE>");
            if (v == "host") a->gzip_device = false;
            else if (v == "device") a->gzip_device = true;
            else bail("invalid value '" + v + "' for '--gzip <WHERE>' [possible values: host, device]");
        } else if (s == "--gzip-effort") {
            const std::string v = val("--gzip-effort <EFFORT>");
            if (v == "normal") a->effort = NGSQ_BGZF_EFFORT_NORMAL;
            else if (v == "high") a->effort = NGSQ_BGZF_EFFORT_HIGH;
            else bail("invalid value '" + v + "' for '--gzip-effort <EFFORT>' [possible values: normal, high]");
            a->has_effort = true;
        } else if (s == "--device") {
            a->device = atoi(val("--device <N>").c_str());
        } else if (!s.empty() && s[0] == '-' && s != "-") bail("unexpected argument '" + s + "' found");
        else a->pos.push_back(s);
    }
    return true;
}

// formats::fastq::writer (formats/fastq.rs:16-44) for one output; "" or the message
struct Output {
    std::string path;
    int fd = -1, write_fd = -1;
    ngsq_gzip_pipe *gz = nullptr;
    bool gzip = false;
};

std::string check_output(const std::string &path, Output *o) {
    const std::string f = detect_format(path);
    if (f.empty()) return "Not able to determine filetype for extension: " + extension_of(path);
    if (f != "FASTQ" && f != "Gzipped FASTQ") return "incompatible formats: required FASTQ, found " + f;
    o->path = path;
    o->gzip = f == "Gzipped FASTQ";
    return "";
}

std::string create_output(Output *o) {
    o->fd = open(o->path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    if (o->fd < 0) return std::string(strerror(errno)) + " (os error " + std::to_string(errno) + ")";
    o->write_fd = o->fd;
    return "";
}

} // namespace

// argv[at] is "generate".  Exit 0 on success, 1 on every error (anyhow::bail! in the reference).
int generate_main(int argc, char **argv, int at) {
    GenerateArgs a;
    if (!parse_args(argc, argv, at, &a)) return 0;
    if (a.has_n && a.has_c) bail(std::string("the argument '--num-records <USIZE>' cannot be used with '--coverage <USIZE>'\n\n") + USAGE);
    {
        std::string missing;
        if (!a.has_n && !a.has_c) missing += " <--num-records <USIZE>|--coverage <USIZE>>";
        if (a.pos.size() < 1) missing += " <READ_ONES_FILE>";
        if (a.pos.size() < 2) missing += " <READ_TWOS_FILE>";
        if (a.pos.size() < 3) missing += " <REFERENCE_PROVIDERS>...";
        if (!missing.empty()) bail("the following required arguments were not provided:" + missing);
    }
    // (additive) the effort is the device encoder's; refused before any file is opened
    if (a.has_effort && !(a.gzip_device && (detect_format(a.pos[0]) == "Gzipped FASTQ" || detect_format(a.pos[1]) == "Gzipped FASTQ")))
        bail("--gzip-effort needs --gzip device");
    // (0) the providers: the strings, the FASTA formats, then the files themselves -- before anything is created
    const size_t np = a.pos.size() - 2;
    std::vector<ngsq_generate_provider> prov(np);
    std::vector<std::vector<char>> paths(np);
    const std::string pctx = "parsing reference providers: ";
    for (size_t k = 0; k < np; k++) {
        const std::string &s = a.pos[2 + k];
        paths[k].resize(s.size() + 1);
        char err[1024];
        if (ngsq_generate_parse_provider(s.c_str(), paths[k].data(), paths[k].size(), &prov[k], err, sizeof err) != NGSQ_OK) bail(pctx + err);
        const std::string path = prov[k].path, format = detect_format(path); // formats::fasta::open (formats/fasta.rs:22-39)
        if (format == "Gzipped FASTA") bail(pctx + "This command does not yet support gzipped FASTA files. Please unzip your FASTA file and try again.");
        if (format.empty()) bail(pctx + "Not able to determine filetype for extension: " + extension_of(path));
        if (format != "FASTA") bail(pctx + "incompatible formats: required FASTA, found " + format);
    }
    ngsq_generate *g = nullptr;
    if (ngsq_generate_open(prov.data(), (uint32_t)np, &g) != NGSQ_OK) bail(pctx + ngsq_generate_last_error());
    logf(2, "Starting generate command...");
    // (1) the outputs, read ones first (decision: the format is looked at before the file is created)
    Output o[2];
    const char *const octx[2] = {"opening reads one file: ", "opening reads two file: "};
    for (int k = 0; k < 2; k++) {
        std::string e = check_output(a.pos[(size_t)k], &o[k]);
        if (e.empty()) e = create_output(&o[k]);
        if (!e.empty()) {
            ngsq_generate_close(g);
            bail(octx[k] + a.pos[(size_t)k] + ": " + e);
        }
    }
    const uint64_t total = a.has_n ? a.n : ngsq_generate_reads_for_coverage(g, a.coverage);
    logf(2, "Generating %llu reads...", (unsigned long long)total);
    if (!a.has_seed) {
        const auto now = std::chrono::system_clock::now().time_since_epoch();
        a.seed = (unsigned long long)std::chrono::duration_cast<std::chrono::nanoseconds>(now).count() * 0x9E3779B97F4A7C15ull ^ (unsigned long long)getpid();
        logf(2, "Seed: %llu", a.seed);
    }
    // (2) the device, the FASTAs' way to it, the pairs
    ngsq_generate_report rep{};
    ngsq_generate_bgzf_report zrep{};
    const bool on_device = a.gzip_device && (o[0].gzip || o[1].gzip);
    std::string msg;
    ngsq_ctx *ctx = nullptr;
    if (total) {
        ngsq_config cfg{};
        cfg.struct_size = sizeof cfg;
        cfg.facets = 0;
        cfg.device = a.device;
        if (ngsq_create(&cfg, &ctx) != NGSQ_OK) msg = ngsq_last_global_error();
        else if (ngsq_bgzf_set_effort(ctx, a.effort) != NGSQ_OK) msg = ngsq_last_error(ctx);
        else if (ngsq_generate_load(g, ctx) != NGSQ_OK) msg = ngsq_generate_last_error();
    }
    for (int k = 0; k < 2 && msg.empty() && !on_device; k++)
        if (o[k].gzip && ngsq_gzip_pipe_open(o[k].fd, 8, &o[k].gz, &o[k].write_fd) != NGSQ_OK) msg = std::string(octx[k]) + o[k].path + ": could not start the compressor";
    if (msg.empty() && on_device) {
        // (also without a pair: a compressed output is the EOF block then, where the host path writes one empty member)
        const uint32_t plain = (o[0].gzip ? 0u : NGSQ_GENERATE_PLAIN_ONE) | (o[1].gzip ? 0u : NGSQ_GENERATE_PLAIN_TWO);
        if (ngsq_generate_write_bgzf(g, o[0].write_fd, o[1].write_fd, a.seed, 0, total, a.batch_pairs, plain, &zrep) != NGSQ_OK) msg = ngsq_generate_last_error();
        rep = zrep.text;
    } else if (msg.empty() && total && ngsq_generate_write(g, o[0].write_fd, o[1].write_fd, a.seed, 0, total, a.batch_pairs, &rep) != NGSQ_OK)
        msg = ngsq_generate_last_error();
    for (int k = 0; k < 2; k++) {
        int e = 0;
        if (o[k].gz) {
            close(o[k].write_fd); // the pipe's end: the compressor finishes
            e = ngsq_gzip_pipe_close(o[k].gz);
        }
        if (close(o[k].fd) != 0 && !e) e = errno;
        if (e && msg.empty())
            msg = std::string("could not write record to read ") + (k ? "two" : "one") + " file: " + strerror(e) + " (os error " + std::to_string(e) + ")";
    }
    ngsq_generate_close(g);
    if (ctx) ngsq_destroy(ctx);
    if (!msg.empty()) bail(msg);
    if (g_level >= 3)
        fprintf(stderr, "[ngs] generate: %llu pairs in %llu batches, %llu text bytes per file; rejected attempts: %llu start, %llu end, %llu base; "
                        "draw %.1f ms, format %.1f ms, copy %.1f ms, write %.1f ms, total %.1f ms\n",
                (unsigned long long)rep.pairs, (unsigned long long)rep.batches, (unsigned long long)rep.text_bytes_one,
                (unsigned long long)rep.rejected_start, (unsigned long long)rep.rejected_end, (unsigned long long)rep.rejected_base, rep.draw_ms,
                rep.format_ms, rep.copy_ms, rep.write_ms, rep.total_ms);
    if (g_level >= 3 && on_device)
        fprintf(stderr, "[ngs] generate: BGZF on the device at effort %s: %llu and %llu compressed bytes in %llu blocks (%llu stored), deflate %.1f ms\n",
                a.effort == NGSQ_BGZF_EFFORT_HIGH ? "high" : "normal", (unsigned long long)zrep.compressed_bytes_one,
                (unsigned long long)zrep.compressed_bytes_two, (unsigned long long)zrep.blocks, (unsigned long long)zrep.stored_blocks, zrep.deflate_ms);
    return 0;
}
