// depth.cpp -- `ngs depth` (DESIGN.md sections 23 and 24; this build's own command, the reference has none): the per-base depth of
// a coordinate-sorted BAM file, or of one region of it, as bedGraph text on stdout or in a file, or with --by <N|BED> its mean
// per window or per interval of a BED file, and with --thresholds <T,...> beside each mean the positions at or above each depth
// (section 25).  The records are read, added up, reduced and formatted on the GPU by ngsq_bam_depth, ngsq_bam_depth_windows and
// ngsq_bam_depth_thresholds (include/ngsq_depth.h).
#include <fcntl.h>

#include <cerrno>
#include <csignal>

#include "../../../include/ngsq_depth.h"
#include "cli.h"

namespace {

// an unsigned integer of at most `max`, in the words of Rust's integer parser
uint32_t int_value(const std::string &v, const char *name, unsigned long long max) {
    const std::string what = "invalid value '" + v + "' for '" + name + "': ";
    const size_t at = !v.empty() && v[0] == '+' ? 1 : 0;
    if (v.empty()) bail(what + "cannot parse integer from empty string");
    if (at == v.size()) bail(what + "invalid digit found in string");
    unsigned long long x = 0;
    bool large = false;
    for (size_t k = at; k < v.size(); k++) {
        if (v[k] < '0' || v[k] > '9') bail(what + "invalid digit found in string");
        x = x * 10 + (unsigned long long)(v[k] - '0');
        if (x > max) large = true, x = max + 1;
    }
    if (large) bail(what + "number too large to fit in target type");
    return (uint32_t)x;
}

} // namespace

// argv[at] is "depth".  Exit 0 on success, 1 on every error.
int depth_main(int argc, char **argv, int at) {
    std::vector<std::string> pos;
    std::string out_path, by, thr_list;
    bool to_file = false, has_by = false, has_thr = false;
    uint32_t exclude = NGSQ_DEPTH_EXCLUDE_FLAGS, min_mapq = 0;
    int device = 0;
    for (int i = at + 1; i < argc; i++) {
        const std::string s = argv[i];
        if (verbosity_option(argv[i])) continue;
        if (s == "-h" || s == "--help") {
            fprintf(stderr, "Usage: ngs depth [OPTIONS] <BAM> [QUERY]\n\n"
                            "Arguments:\n"
                            "  <BAM>    Coordinate-sorted source BAM\n"
                            "  [QUERY]  If given, the region the depth is written of (name, name:S or name:S-E, 1-based, inclusive);\n"
                            "           needs <BAM>.bai\n\n"
                            "Options:\n"
                            "  -o, --output <PATH>\n"
                            "          File the bedGraph text is written to, created or truncated [default: stdout]\n"
                            "      --by <N|BED>\n"
                            "          Write the mean depth of every window of N positions, or of every interval of the BED file, instead\n"
                            "          (digits are a window size: write ./500 for a file of that name; a BED file not with [QUERY])\n"
                            "      --thresholds <T,...>\n"
                            "          With --by: behind each mean, the number of the interval's positions whose depth is at least T, for each of\n"
                            "          1 to 8 depths, comma-separated and strictly ascending (as in: 1,10,20,30)\n"
                            "      --exclude-flags <INT>\n"
                            "          Records with any of these flag bits do not count [default: 1796]\n"
                            "      --min-mapq <INT>\n"
                            "          Records with a lower mapping quality do not count [default: 0]\n"
                            "      --device <N>\n"
                            "          GPU the depth is computed on [default: 0]\n\n"
                            "Lines: <name> <start> <end> <depth>, tab-separated, 0-based half-open, one per run of equal depth, zero included.\n"
                            "With --by: <name> <start> <end> <mean>, one per window or interval, the mean with two decimals, rounded half up.\n"
                            "With --thresholds: <name> <start> <end> <mean> <n_1> ... <n_K>, n_k the positions of the interval at or above the k-th depth.\n"
                            "A record covers its alignment start to its alignment end, deletions and skips included.\n");
            return 0;
        } else if (s == "-o" || s == "--output") {
            out_path = option_value(argc, argv, &i, "--output <PATH>");
            to_file = true;
        } else if (s == "--by") {
            by = option_value(argc, argv, &i, "--by <N|BED>");
            has_by = true;
        } else if (s == "--thresholds") {
            thr_list = option_value(argc, argv, &i, "--thresholds <T,...>");
            has_thr = true;
        } else if (s == "--exclude-flags") {
            exclude = int_value(option_value(argc, argv, &i, "--exclude-flags <INT>"), "--exclude-flags <INT>", 65535);
        } else if (s == "--min-mapq") {
            min_mapq = int_value(option_value(argc, argv, &i, "--min-mapq <INT>"), "--min-mapq <INT>", 255);
        } else if (s == "--device") {
            device = atoi(option_value(argc, argv, &i, "--device <N>").c_str());
        } else if (!s.empty() && s[0] == '-' && s != "-") bail("unexpected argument '" + s + "' found");
        else pos.push_back(s);
    }
    if (pos.empty()) bail("the following required arguments were not provided: <BAM>");
    if (pos.size() > 2) bail("unexpected argument '" + pos[2] + "' found");
    // --by: decimal digits behind an optional '+' are a window size, anything else is the path of a BED file
    uint32_t window = 0;
    const size_t digits_at = !by.empty() && by[0] == '+' ? 1 : 0;
    const bool by_bed = has_by && (by.size() == digits_at || by.find_first_not_of("0123456789", digits_at) != std::string::npos);
    if (has_by && !by_bed) {
        window = int_value(by, "--by <N|BED>", 2147483647);
        if (!window) bail("invalid value '" + by + "' for '--by <N|BED>': window size must be at least 1");
    }
    if (by_bed && pos.size() > 1) bail("the argument '--by <BED>' cannot be used with '[QUERY]'");
    // --thresholds: 1 to 8 integers from 1 to 2^31 - 1, comma-separated, strictly ascending
    uint32_t thresholds[NGSQ_DEPTH_MAX_THRESHOLDS] = {}, n_thresholds = 0;
    if (has_thr) {
        if (!has_by) bail("the following required arguments were not provided: --by <N|BED>");
        const std::string what = "invalid value '" + thr_list + "' for '--thresholds <T,...>': ";
        std::vector<uint32_t> t;
        for (size_t a = 0;;) {
            const size_t comma = thr_list.find(',', a);
            const std::string element = thr_list.substr(a, comma == std::string::npos ? std::string::npos : comma - a);
            t.push_back(int_value(element, "--thresholds <T,...>", 2147483647));
            if (!t.back()) bail("invalid value '0' for '--thresholds <T,...>': a threshold must be at least 1");
            if (comma == std::string::npos) break;
            a = comma + 1;
        }
        if (t.size() > NGSQ_DEPTH_MAX_THRESHOLDS) bail(what + "at most 8 thresholds");
        for (size_t k = 1; k < t.size(); k++)
            if (t[k] <= t[k - 1]) bail(what + "thresholds must be strictly ascending");
        n_thresholds = (uint32_t)t.size();
        std::copy(t.begin(), t.end(), thresholds);
    }
    const std::string &src = pos[0];
    const std::string format = detect_format(src);
    if (format.empty()) bail("Not able to determine filetype for extension: " + extension_of(src));
    if (format != "BAM") bail("incompatible formats: required BAM, found " + format);
    // (1) the header, the order it promises, the query and its index: before any GPU work and before the output is touched
    ngsq_bam *bam = nullptr;
    if (ngsq_bam_open(src.c_str(), 0, &bam) != NGSQ_OK) bail(ngsq_bam_last_error());
    if (!ngsq_bam_sorted_by_coordinate(bam)) bail("the input BAM must be coordinate-sorted to compute depth");
    const char *query = pos.size() > 1 ? pos[1].c_str() : nullptr;
    if (query) {
        uint64_t n = 0;
        if (ngsq_bam_query_chunks(bam, nullptr, query, nullptr, nullptr, nullptr, nullptr, 0, &n) != NGSQ_OK) bail(ngsq_bam_last_error());
    }
    ngsq_depth_interval *intervals = nullptr;
    uint64_t n_intervals = 0;
    if (by_bed && ngsq_depth_read_bed(bam, by.c_str(), &intervals, &n_intervals) != NGSQ_OK) bail(ngsq_bam_last_error());
    // (2) the device, then the output; a reader that goes away ends the command with the write's error, not with a signal
    ngsq_ctx *ctx = plain_context(bam, device);
    if (!ctx) bail(ngsq_last_global_error());
    signal(SIGPIPE, SIG_IGN);
    int fd = STDOUT_FILENO;
    if (to_file) {
        fd = open(out_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
        if (fd < 0) bail("creating " + out_path + ": " + strerror(errno) + " (os error " + std::to_string(errno) + ")");
    }
    // (3) the depth
    ngsq_depth_report rep{};
    ngsq_depth_windows_report wrep{};
    ngsq_depth_thresholds_report trep{};
    const int rc = has_thr ? ngsq_bam_depth_thresholds(bam, ctx, fd, window, intervals, n_intervals, thresholds, n_thresholds, query, nullptr, exclude, min_mapq, 0,
                                                       0, 0, 0, &trep)
                   : has_by ? ngsq_bam_depth_windows(bam, ctx, fd, window, intervals, n_intervals, query, nullptr, exclude, min_mapq, 0, 0, 0, 0, &wrep)
                          : ngsq_bam_depth(bam, ctx, fd, query, nullptr, exclude, min_mapq, 0, 0, 0, &rep);
    ngsq_depth_free_intervals(intervals);
    std::string msg = rc ? ngsq_bam_last_error() : "";
    if (to_file && close(fd) != 0 && !rc) msg = "writing depth to stream: " + std::string(strerror(errno)) + " (os error " + std::to_string(errno) + ")";
    ngsq_destroy(ctx);
    ngsq_bam_close(bam);
    if (!msg.empty()) bail(msg);
    std::string covered; // the -v line of a thresholds call: the K covered totals
    if (has_thr) {
        memcpy(&wrep, &trep, sizeof wrep); // (the thresholds report begins with the windows report's fields)
        covered = ", covered";
        for (uint32_t k = 0; k < n_thresholds; k++) covered += " " + std::to_string((unsigned long long)trep.covered[k]);
    }
    if (g_level >= 3 && has_by)
        fprintf(stderr, "[ngs] depth: %llu of %llu records counted in %llu batches and %llu range walks; %llu lines of %llu sequences in %llu tiles and "
                        "%llu format passes, depth sum %llu%s, %llu text bytes; ingest %.1f ms, add %.1f ms, reduce %.1f ms, format %.1f ms, copy %.1f ms, "
                        "write %.1f ms, total %.1f ms\n",
                (unsigned long long)wrep.records_counted, (unsigned long long)wrep.records_scanned, (unsigned long long)wrep.batches,
                (unsigned long long)wrep.ranges, (unsigned long long)wrep.lines, (unsigned long long)wrep.sequences, (unsigned long long)wrep.tiles,
                (unsigned long long)wrep.passes, (unsigned long long)wrep.depth_sum, covered.c_str(), (unsigned long long)wrep.text_bytes, wrep.scan_ms, wrep.add_ms,
                wrep.reduce_ms, wrep.format_ms, wrep.copy_ms, wrep.write_ms, wrep.total_ms);
    else if (g_level >= 3)
        fprintf(stderr, "[ngs] depth: %llu of %llu records counted in %llu batches and %llu range walks; %llu runs of %llu sequences in %llu tiles, "
                        "%llu text bytes; ingest %.1f ms, add %.1f ms, runs %.1f ms, format %.1f ms, copy %.1f ms, write %.1f ms, total %.1f ms\n",
                (unsigned long long)rep.records_counted, (unsigned long long)rep.records_scanned, (unsigned long long)rep.batches,
                (unsigned long long)rep.ranges, (unsigned long long)rep.runs, (unsigned long long)rep.sequences, (unsigned long long)rep.tiles,
                (unsigned long long)rep.text_bytes, rep.scan_ms, rep.add_ms, rep.runs_ms, rep.format_ms, rep.copy_ms, rep.write_ms, rep.total_ms);
    return 0;
}
