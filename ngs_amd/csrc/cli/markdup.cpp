// markdup.cpp -- `ngs markdup` (this build's own command, the reference has none): the duplicate reads of
// a BAM file marked with flag 0x400, or with --remove left out, and the file written again as BAM.  Ends, scores, mates, groups
// and flags are the GPU's, as is the BGZF of the output (ngsq_bam_mark_duplicates, include/ngsq_markdup.h).  The output must not
// exist, so it is this command's own file: after every error it is removed.
#include <fcntl.h>
#include <sys/stat.h>

#include <algorithm>
#include <cerrno>

#include "../../../include/ngsq_bgzf.h"
#include "../../../include/ngsq_markdup.h"
#include "cli.h"

namespace {

const char *const USAGE = "Usage: ngs markdup [OPTIONS] <BAM> <OUT_BAM>";

std::string metrics_json(const ngsq_markdup_report &r) {
    char buf[1024];
    snprintf(buf, sizeof buf,
             "{\n  \"records\": %llu,\n  \"candidates\": %llu,\n  \"pairs\": %llu,\n  \"fragments\": %llu,\n  \"duplicate_pairs\": %llu,\n"
             "  \"duplicate_fragments\": %llu,\n  \"duplicate_records\": %llu,\n  \"cleared\": %llu,\n  \"ambiguous\": %llu,\n"
             "  \"name_collisions\": %llu,\n  \"duplication\": %.6f\n}\n",
             (unsigned long long)r.records, (unsigned long long)r.candidates, (unsigned long long)r.pairs, (unsigned long long)r.fragments,
             (unsigned long long)r.duplicate_pairs, (unsigned long long)r.duplicate_fragments, (unsigned long long)r.duplicate_records,
             (unsigned long long)r.cleared, (unsigned long long)r.ambiguous, (unsigned long long)r.name_collisions, r.duplication);
    return buf;
}

} // namespace

// argv[at] is "markdup".  Exit 0 on success, 1 on every error.
int markdup_main(int argc, char **argv, int at) {
    std::vector<std::string> pos;
    std::string metrics_path;
    bool has_n = false, has_metrics = false;
    unsigned long long n = 0;
    ngsq_markdup_options opt{};
    opt.struct_size = sizeof opt;
    uint32_t effort = NGSQ_BGZF_EFFORT_NORMAL;
    int device = 0;
    for (int i = at + 1; i < argc; i++) {
        const std::string s = argv[i];
        auto val = [&](const char *name) { return option_value(argc, argv, &i, name); };
        if (verbosity_option(argv[i])) continue;
        if (s == "-h" || s == "--help") {
            fprintf(stderr,
                    "Marks the duplicate reads of a BAM file\n\n%s\n\n"
                    "Arguments:\n"
                    "  <BAM>      Source BAM, in any record order; no index is needed\n"
                    "  <OUT_BAM>  Destination BAM: the same header and records in the same order, flag 0x400 set on the duplicates and\n"
                    "             cleared on every other record; it must not exist\n\n"
                    "Options:\n"
                    "      --remove\n"
                    "          Leave the duplicates out instead of marking them\n"
                    "      --metrics <FILE>\n"
                    "          Write the counts as one JSON document to this file\n"
                    "      --gzip-effort <EFFORT>\n"
                    "          `high` has the GPU's encoder search harder for matches, which gives a smaller BAM for more encoder time\n"
                    "          [default: normal] [possible values: normal, high]\n"
                    "  -n, --num-records <USIZE>\n"
                    "          Examine and write only the first N records of the file (at least one, as `ngs convert` counts them)\n"
                    "      --memory <SIZE>\n"
                    "          Device memory the records may take, digits with an optional K, M or G [default: the free memory less 4G]\n"
                    "      --device <N>\n"
                    "          GPU the duplicates are marked on [default: 0]\n"
                    "  -t, --threads <N>\n"
                    "          Accepted and unused\n\n"
                    "A candidate is a mapped primary record (none of 0x4, 0x100, 0x800).  Its end is its unclipped 5' position and strand.\n"
                    "Mates are paired by name; pairs with the same two ends are duplicates of the pair with the largest sum of base\n"
                    "qualities >= 15, and so are reads without a mapped mate that share an end, or that share it with a pair.  The file is\n"
                    "treated as one library; secondary and supplementary records are never marked.  The output is BGZF from the GPU's encoder.\n",
                    USAGE);
            return 0;
        } else if (s == "--remove") {
            opt.remove = 1;
        } else if (s == "--metrics") {
            metrics_path = val("--metrics <FILE>");
            has_metrics = true;
        } else if (s == "--gzip-effort") {
            const std::string v = val("--gzip-effort <EFFORT>");
            if (v == "normal") effort = NGSQ_BGZF_EFFORT_NORMAL;
            else if (v == "high") effort = NGSQ_BGZF_EFFORT_HIGH;
            else bail("invalid value '" + v + "' for '--gzip-effort <EFFORT>' [possible values: normal, high]");
        } else if (s == "-n" || s == "--num-records") {
            const std::string v = val("--num-records <USIZE>");
            char *e = nullptr;
            errno = 0;
            n = strtoull(v.c_str(), &e, 10);
            if (v.empty() || *e || errno || v[0] == '-' || v[0] == '+') bail("invalid value '" + v + "' for '--num-records <USIZE>': invalid digit found in string");
            has_n = true;
        } else if (s == "--memory") {
            opt.memory_budget = size_value(val("--memory <SIZE>"), "--memory <SIZE>");
        } else if (s == "--device") {
            device = atoi(val("--device <N>").c_str());
        } else if (s == "-t" || s == "--threads") {
            (void)val("--threads <N>");
        } else if (!s.empty() && s[0] == '-' && s != "-") bail("unexpected argument '" + s + "' found");
        else pos.push_back(s);
    }
    {
        std::string missing;
        if (pos.size() < 1) missing += " <BAM>";
        if (pos.size() < 2) missing += " <OUT_BAM>";
        if (!missing.empty()) bail("the following required arguments were not provided:" + missing + "\n\n" + USAGE);
    }
    if (pos.size() > 2) bail("unexpected argument '" + pos[2] + "' found");
    const std::string &from = pos[0], &to = pos[1];
    // (0) every refusal comes before any file is created; the formats in `ngs convert`'s words
    const std::string ff = detect_format(from);
    if (ff.empty()) bail("failed to detect from input filetype: " + from + ": Failed parsing of bioinformatics file format.");
    const std::string tf = detect_format(to);
    if (tf.empty()) bail("failed to deteect to input filetype: " + to + ": Failed parsing of bioinformatics file format.");
    if (ff != "BAM") bail("opening BAM input file: " + from + ": incompatible formats: required BAM, found " + ff);
    if (tf != "BAM") bail("opening BAM output file: " + to + ": incompatible formats: required BAM, found " + tf);
    if (from == to) bail("Conversion from BAM to BAM needs two files: " + to + " is the input");
    ngsq_bam *bam = nullptr;
    if (ngsq_bam_open(from.c_str(), 0, &bam) != NGSQ_OK) bail(std::string("opening BAM input file: ") + ngsq_bam_last_error());
    struct stat sf, stt;
    const bool to_exists = stat(to.c_str(), &stt) == 0;
    if (to_exists && stat(from.c_str(), &sf) == 0 && sf.st_dev == stt.st_dev && sf.st_ino == stt.st_ino) {
        ngsq_bam_close(bam);
        bail("Conversion from BAM to BAM needs two files: " + to + " is the input");
    }
    if (to_exists) {
        ngsq_bam_close(bam);
        bail("refusing to overwrite existing output file: " + to + ". Please delete and rerun if you'd like to replace it.");
    }
    if (has_metrics && stat(metrics_path.c_str(), &stt) == 0 && stat(from.c_str(), &sf) == 0 && sf.st_dev == stt.st_dev && sf.st_ino == stt.st_ino) {
        ngsq_bam_close(bam);
        bail("opening metrics file: " + metrics_path + ": the same file as the input");
    }
    if (has_metrics && metrics_path == to) {
        ngsq_bam_close(bam);
        bail("opening metrics file: " + metrics_path + ": the same file as the output");
    }
    logf(2, "Starting markdup command...");
    // (1) the device, then the output: a machine without a device leaves no file behind
    ngsq_ctx *ctx = plain_context(bam, device);
    if (!ctx) {
        ngsq_bam_close(bam);
        bail(ngsq_last_global_error());
    }
    std::string msg;
    if (ngsq_bgzf_set_effort(ctx, effort) != NGSQ_OK) msg = ngsq_last_error(ctx);
    int fd = -1;
    if (msg.empty()) {
        fd = open(to.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_CLOEXEC, 0666);
        if (fd < 0) {
            const int e = errno;
            msg = std::string("opening BAM output file: ") + strerror(e) + " (os error " + std::to_string(e) + ")";
        }
    }
    ngsq_markdup_report rep{};
    if (msg.empty()) {
        opt.max_records = has_n ? std::max<unsigned long long>(n, 1) : 0;
        if (ngsq_bam_mark_duplicates(bam, ctx, fd, &opt, &rep) != NGSQ_OK) msg = ngsq_bam_last_error();
    }
    if (fd >= 0 && close(fd) != 0 && msg.empty()) {
        const int e = errno;
        msg = std::string("writing BAM record: ") + strerror(e) + " (os error " + std::to_string(e) + ")";
    }
    ngsq_destroy(ctx);
    ngsq_bam_close(bam);
    if (msg.empty() && has_metrics) {
        const std::string doc = metrics_json(rep);
        FILE *f = fopen(metrics_path.c_str(), "w");
        if (!f || fwrite(doc.data(), 1, doc.size(), f) != doc.size() || fclose(f) != 0) {
            const int e = errno;
            msg = "writing metrics file: " + metrics_path + ": " + strerror(e) + " (os error " + std::to_string(e) + ")";
        }
    }
    if (!msg.empty()) {
        if (fd >= 0) unlink(to.c_str()); // (created here, a moment ago: the partial file is this command's to remove)
        bail(msg);
    }
    logf(2, "%llu duplicate records of %llu: %llu duplicate pairs of %llu, %llu duplicate fragments of %llu (duplication %.6f)%s",
         (unsigned long long)rep.duplicate_records, (unsigned long long)rep.records, (unsigned long long)rep.duplicate_pairs, (unsigned long long)rep.pairs,
         (unsigned long long)rep.duplicate_fragments, (unsigned long long)rep.fragments, rep.duplication, opt.remove ? ", removed" : "");
    if (g_level >= 3)
        fprintf(stderr, "[ngs] markdup: %llu records in %llu batches, %llu resident bytes: %llu candidates, %llu pairs, %llu fragments, %llu + %llu duplicates, "
                        "%llu cleared, %llu ambiguous, %llu name collisions, %llu sort passes; %llu BAM bytes in %llu pieces, %llu blocks (%llu stored), "
                        "%llu compressed at effort %s; walk %.1f ms (ingest %.1f ms), ends %.1f ms, match %.1f ms, mark %.1f ms, gather %.1f ms, "
                        "deflate %.1f ms, down %.1f ms, write %.1f ms, total %.1f ms\n",
                (unsigned long long)rep.records, (unsigned long long)rep.batches, (unsigned long long)rep.resident_bytes, (unsigned long long)rep.candidates,
                (unsigned long long)rep.pairs, (unsigned long long)rep.fragments, (unsigned long long)rep.duplicate_pairs,
                (unsigned long long)rep.duplicate_fragments, (unsigned long long)rep.cleared, (unsigned long long)rep.ambiguous,
                (unsigned long long)rep.name_collisions, (unsigned long long)rep.sort_passes, (unsigned long long)rep.bam_bytes, (unsigned long long)rep.pieces,
                (unsigned long long)rep.blocks, (unsigned long long)rep.stored_blocks, (unsigned long long)rep.compressed_bytes,
                effort == NGSQ_BGZF_EFFORT_HIGH ? "high" : "normal", rep.walk_ms, rep.scan_ms, rep.ends_ms, rep.match_ms, rep.mark_ms, rep.gather_ms,
                rep.deflate_ms, rep.d2h_ms, rep.write_ms, rep.total_ms);
    return 0;
}
