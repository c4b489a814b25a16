// fastq.cpp -- `ngs fastq` (this build's own command, the reference has none): the reads of a BAM file
// back as FASTQ, in one file or split into read ones, read twos and others by the flag.  The records are read, classified
// and formatted on the GPU by ngsq_bam_write_fastq (include/ngsq_fastq.h); gzipped outputs are compressed by host threads
// behind a pipe or, with --gzip device, written as BGZF by the GPU's encoder, as `ngs generate` writes its files.  With --collate
// the mates are paired by name on the GPU (ngsq_bam_write_fastq_collated, include/ngsq_collate.h): the two
// files pair line by line whatever the order of the BAM, and a fourth output takes the singletons.
#include <fcntl.h>
#include <sys/stat.h>

#include <algorithm>
#include <cerrno>

#include "../../../include/ngsq_bgzf.h"
#include "../../../include/ngsq_collate.h"
#include "../../../include/ngsq_fastq.h"
#include "../../../include/ngsq_generate.h"
#include "cli.h"

namespace {

const char *const USAGE = "Usage: ngs fastq [OPTIONS] <BAM> <READ_ONES_FILE> [<READ_TWOS_FILE>]";

// an unsigned integer of at most `max`, in the words of Rust's integer parser (as `ngs depth` reads its integers)
unsigned long long int_value(const std::string &v, const char *name, unsigned long long max) {
    const std::string what = "invalid value '" + v + "' for '" + name + "': ";
    const size_t at = !v.empty() && v[0] == '+' ? 1 : 0;
    if (v.empty()) bail(what + "cannot parse integer from empty string");
    if (at == v.size()) bail(what + "invalid digit found in string");
    unsigned long long x = 0;
    bool large = false;
    for (size_t k = at; k < v.size(); k++) {
        if (v[k] < '0' || v[k] > '9') bail(what + "invalid digit found in string");
        if (x > (max - (unsigned long long)(v[k] - '0')) / 10) large = true;
        else x = x * 10 + (unsigned long long)(v[k] - '0');
    }
    if (large) bail(what + "number too large to fit in target type");
    return x;
}

struct Output {
    std::string path;
    const char *opening = nullptr, *writing = nullptr; // "opening reads one file: ", "read one file"
    int fd = -1, write_fd = -1;
    ngsq_gzip_pipe *gz = nullptr;
    bool gzip = false;
};

// formats::fastq::writer's test of one output (as `ngs generate` makes it); "" or the message
std::string check_output(Output *o) {
    const std::string f = detect_format(o->path);
    if (f.empty()) return "Not able to determine filetype for extension: " + extension_of(o->path);
    if (f != "FASTQ" && f != "Gzipped FASTQ") return "incompatible formats: required FASTQ, found " + f;
    o->gzip = f == "Gzipped FASTQ";
    return "";
}

// true: the two paths name one existing file, or are the same words
bool same_file(const std::string &a, const std::string &b) {
    if (a == b) return true;
    struct stat sa, sb;
    return stat(a.c_str(), &sa) == 0 && stat(b.c_str(), &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino;
}

} // namespace

// argv[at] is "fastq".  Exit 0 on success, 1 on every error.
int fastq_main(int argc, char **argv, int at) {
    std::vector<std::string> pos;
    std::string other_path, single_path;
    bool has_other = false, has_n = false, gzip_device = false, has_effort = false, collate = false, has_single = false, has_memory = false;
    unsigned long long n = 0, collate_memory = 0;
    ngsq_fastq_options opt{};
    opt.struct_size = sizeof opt;
    opt.exclude_flags = NGSQ_FASTQ_EXCLUDE_FLAGS;
    opt.default_quality = NGSQ_FASTQ_DEFAULT_QUALITY;
    uint32_t effort = NGSQ_BGZF_EFFORT_NORMAL;
    int device = 0;
    for (int i = at + 1; i < argc; i++) {
        const std::string s = argv[i];
        auto val = [&](const char *name) { return option_value(argc, argv, &i, name); };
        if (verbosity_option(argv[i])) continue;
        if (s == "-h" || s == "--help") {
            fprintf(stderr,
                    "Writes the reads of a BAM file as FASTQ\n\n%s\n\n"
                    "Arguments:\n"
                    "  <BAM>              Source BAM, in any record order; no index is needed\n"
                    "  <READ_ONES_FILE>   Destination for the FASTQ file containing all read ones; without <READ_TWOS_FILE>, all reads\n"
                    "  [<READ_TWOS_FILE>] Destination for the FASTQ file containing all read twos\n\n"
                    "Options:\n"
                    "      --other <FILE>\n"
                    "          With <READ_TWOS_FILE>: destination for the reads that are neither a read one nor a read two (flag bits\n"
                    "          0x40 and 0x80 both clear or both set) [default: they are dropped and counted]\n"
                    "      --collate\n"
                    "          Pair the mates by name on the GPU, whatever the order of the BAM: pair p's read one is record p of\n"
                    "          <READ_ONES_FILE> and its read two record p of <READ_TWOS_FILE> (without <READ_TWOS_FILE>: interleaved), in\n"
                    "          the order of each pair's earlier record; reads without exactly one mate are singletons\n"
                    "      --singletons <FILE>\n"
                    "          With --collate: destination for the singletons [default: they are dropped and counted]\n"
                    "      --collate-memory <SIZE>\n"
                    "          With --collate: device memory the kept records may take, digits with an optional K, M or G\n"
                    "          [default: the free memory less 4G]\n"
                    "      --exclude-flags <INT>\n"
                    "          Records with any of these flag bits are not written [default: 2304]\n"
                    "      --require-flags <INT>\n"
                    "          Records must have all of these flag bits to be written [default: 0]\n"
                    "  -n, --num-records <USIZE>\n"
                    "          Examine only the first N records of the file, written or not\n"
                    "      --name-suffix\n"
                    "          Append /1 to the names of read ones and /2 to the names of read twos\n"
                    "      --default-quality <INT>\n"
                    "          The score, 0 to 93, written for every base of a record without qualities [default: 1]\n"
                    "      --gzip <WHERE>\n"
                    "          Where gzipped outputs are compressed: host threads behind a pipe, or the GPU, which writes BGZF and sends\n"
                    "          only compressed bytes to the host; plain outputs are not affected [default: host] [possible values: host, device]\n"
                    "      --gzip-effort <EFFORT>\n"
                    "          With --gzip device: `high` has the GPU's encoder search harder for matches, which gives smaller files for\n"
                    "          more encoder time [default: normal] [possible values: normal, high]\n"
                    "      --device <N>\n"
                    "          GPU the reads are formatted on [default: 0]\n"
                    "  -t, --threads <N>\n"
                    "          Accepted and unused\n\n"
                    "Outputs are FASTQ (.fastq, .fq) or gzipped FASTQ (.fastq.gz, .fq.gz).  A record becomes @<name>, its bases, +, its\n"
                    "qualities; a record on the reverse strand (flag 0x10) is reverse-complemented and its qualities reversed, so that the\n"
                    "read comes out as the sequencer gave it.  Secondary and supplementary records are left out by default.\n"
                    "Nothing is paired unless --collate is given: every file holds its reads in the order of the BAM.  The two files of a\n"
                    "name-grouped BAM correspond line by line; those of a coordinate-sorted BAM hold the same reads in different orders --\n"
                    "group it by name first, or give --collate.\n",
                    USAGE);
            return 0;
        } else if (s == "--other") {
            other_path = val("--other <FILE>");
            has_other = true;
        } else if (s == "--collate") {
            collate = true;
        } else if (s == "--singletons") {
            single_path = val("--singletons <FILE>");
            has_single = true;
        } else if (s == "--collate-memory") {
            collate_memory = size_value(val("--collate-memory <SIZE>"), "--collate-memory <SIZE>");
            has_memory = true;
        } else if (s == "--exclude-flags") {
            opt.exclude_flags = (uint32_t)int_value(val("--exclude-flags <INT>"), "--exclude-flags <INT>", 65535);
        } else if (s == "--require-flags") {
            opt.require_flags = (uint32_t)int_value(val("--require-flags <INT>"), "--require-flags <INT>", 65535);
        } else if (s == "-n" || s == "--num-records") {
            n = int_value(val("--num-records <USIZE>"), "--num-records <USIZE>", ~0ull);
            has_n = true;
        } else if (s == "--name-suffix") {
            opt.name_suffix = 1;
        } else if (s == "--default-quality") {
            const std::string v = val("--default-quality <INT>");
            const unsigned long long q = int_value(v, "--default-quality <INT>", 255);
            if (q > NGSQ_FASTQ_MAX_QUALITY) bail("invalid value '" + v + "' for '--default-quality <INT>': a quality score is at most 93");
            opt.default_quality = (uint32_t)q;
        } else if (s == "--gzip") {
            const std::string v = val("--gzip <WHERE>");
            if (v == "host") gzip_device = false;
            else if (v == "device") gzip_device = true;
            else bail("invalid value '" + v + "' for '--gzip <WHERE>' [possible values: host, device]");
        } else if (s == "--gzip-effort") {
            const std::string v = val("--gzip-effort <EFFORT>");
            if (v == "normal") effort = NGSQ_BGZF_EFFORT_NORMAL;
            else if (v == "high") effort = NGSQ_BGZF_EFFORT_HIGH;
            else bail("invalid value '" + v + "' for '--gzip-effort <EFFORT>' [possible values: normal, high]");
            has_effort = true;
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
        if (pos.size() < 2) missing += " <READ_ONES_FILE>";
        if (!missing.empty()) bail("the following required arguments were not provided:" + missing + "\n\n" + USAGE);
    }
    if (pos.size() > 3) bail("unexpected argument '" + pos[3] + "' found");
    const bool two_files = pos.size() == 3;
    if (has_other && !two_files) bail("the argument '--other <FILE>' needs <READ_TWOS_FILE>: in one-file mode every read goes to the one file");
    if (has_single && !collate) bail("the argument '--singletons <FILE>' needs --collate");
    if (has_memory && !collate) bail("the argument '--collate-memory <SIZE>' needs --collate");
    // (0) the outputs' formats and names, then the input: every refusal comes before any file is created
    Output o[4];
    o[0].path = pos[1], o[0].opening = "opening reads one file: ", o[0].writing = "read one file";
    o[1].path = two_files ? pos[2] : "", o[1].opening = "opening reads two file: ", o[1].writing = "read two file";
    o[2].path = other_path, o[2].opening = "opening other reads file: ", o[2].writing = "other reads file";
    o[3].path = single_path, o[3].opening = "opening singletons file: ", o[3].writing = "singletons file";
    std::vector<int> act = {0}; // the outputs that are given, in the order of their numbers
    if (two_files) act.push_back(1);
    if (two_files && has_other) act.push_back(2);
    if (has_single) act.push_back(3);
    for (const int k : act) {
        const std::string e = check_output(&o[k]);
        if (!e.empty()) bail(o[k].opening + o[k].path + ": " + e);
    }
    for (const int k : act)
        for (const int j : act)
            if (j < k && same_file(o[j].path, o[k].path)) bail(o[k].opening + o[k].path + ": the same file as the " + o[j].writing);
    bool any_gzip = false;
    for (const int k : act) any_gzip |= o[k].gzip;
    if (has_effort && !(gzip_device && any_gzip)) bail("--gzip-effort needs --gzip device");
    const std::string &src = pos[0];
    const std::string format = detect_format(src);
    if (format.empty()) bail("failed to detect from input filetype: " + src + ": Failed parsing of bioinformatics file format.");
    if (format != "BAM") bail("opening BAM input file: " + src + ": incompatible formats: required BAM, found " + format);
    for (const int k : act)
        if (same_file(src, o[k].path)) bail(o[k].opening + o[k].path + ": the same file as the input");
    ngsq_bam *bam = nullptr;
    if (ngsq_bam_open(src.c_str(), 0, &bam) != NGSQ_OK) bail(std::string("opening BAM input file: ") + ngsq_bam_last_error());
    for (const int k : act) // (a link to the input made under another name)
        if (same_file(src, o[k].path)) bail(o[k].opening + o[k].path + ": the same file as the input");
    logf(2, "Starting fastq command...");
    // (1) the device, then the outputs, read ones first: a machine without a device leaves no file behind
    ngsq_ctx *ctx = plain_context(bam, device);
    if (!ctx) {
        ngsq_bam_close(bam);
        bail(ngsq_last_global_error());
    }
    for (const int k : act) {
        o[k].fd = open(o[k].path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
        if (o[k].fd < 0) {
            const int e = errno;
            ngsq_destroy(ctx);
            ngsq_bam_close(bam);
            bail(o[k].opening + o[k].path + ": " + strerror(e) + " (os error " + std::to_string(e) + ")");
        }
        o[k].write_fd = o[k].fd;
    }
    // (2) the compressors, the reads
    const bool on_device = gzip_device && any_gzip;
    std::string msg;
    if (ngsq_bgzf_set_effort(ctx, effort) != NGSQ_OK) msg = ngsq_last_error(ctx);
    for (const int k : act) {
        if (!msg.empty()) break;
        if (!o[k].gzip) continue;
        if (on_device) opt.bgzf_mask |= 1u << k;
        else if (ngsq_gzip_pipe_open(o[k].fd, 8, &o[k].gz, &o[k].write_fd) != NGSQ_OK) msg = std::string(o[k].opening) + o[k].path + ": could not start the compressor";
    }
    ngsq_fastq_report rep{};
    ngsq_collate_report crep{};
    if (msg.empty() && has_n && n == 0) {
        // no record is examined: every output is empty, which for a BGZF output is the EOF block alone
        for (const int k : act)
            if (msg.empty() && (opt.bgzf_mask >> k & 1)) {
                uint8_t eof[64];
                uint64_t len = 0;
                if (ngsq_bgzf_deflate_device(ctx, nullptr, 0, eof, sizeof eof, &len, NGSQ_BGZF_EOF, nullptr) != NGSQ_OK) msg = ngsq_last_error(ctx);
                else if (write(o[k].fd, eof, (size_t)len) != (ssize_t)len)
                    msg = std::string("could not write record to ") + o[k].writing + ": " + strerror(errno) + " (os error " + std::to_string(errno) + ")";
            }
    } else if (msg.empty() && collate) {
        ngsq_collate_options copt{};
        copt.struct_size = sizeof copt;
        copt.require_flags = opt.require_flags, copt.exclude_flags = opt.exclude_flags;
        copt.default_quality = opt.default_quality, copt.name_suffix = opt.name_suffix, copt.bgzf_mask = opt.bgzf_mask;
        copt.max_records = has_n ? n : 0;
        copt.memory_budget = collate_memory;
        auto fd_of = [&](int k) { return std::find(act.begin(), act.end(), k) != act.end() ? o[k].write_fd : -1; };
        if (ngsq_bam_write_fastq_collated(bam, ctx, fd_of(0), fd_of(1), fd_of(2), fd_of(3), &copt, &crep) != NGSQ_OK) msg = ngsq_bam_last_error();
    } else if (msg.empty()) {
        opt.max_records = has_n ? n : 0;
        if (ngsq_bam_write_fastq(bam, ctx, o[0].write_fd, two_files ? o[1].write_fd : -1, has_other ? o[2].write_fd : -1, &opt, &rep) != NGSQ_OK)
            msg = ngsq_bam_last_error();
    }
    for (const int k : act) {
        int e = 0;
        if (o[k].gz) {
            close(o[k].write_fd); // the pipe's end: the compressor finishes
            e = ngsq_gzip_pipe_close(o[k].gz);
        }
        if (close(o[k].fd) != 0 && !e) e = errno;
        if (e && msg.empty()) msg = std::string("could not write record to ") + o[k].writing + ": " + strerror(e) + " (os error " + std::to_string(e) + ")";
    }
    if (ctx) ngsq_destroy(ctx);
    ngsq_bam_close(bam);
    if (!msg.empty()) bail(msg);
    if (collate) {
        logf(2, "%llu pairs, %llu singletons (%llu ambiguous, %llu dropped), %llu other reads dropped", (unsigned long long)crep.pairs,
             (unsigned long long)crep.singletons, (unsigned long long)crep.ambiguous, (unsigned long long)crep.dropped_singletons,
             (unsigned long long)crep.dropped_other);
        if (g_level >= 3)
            fprintf(stderr, "[ngs] fastq --collate: %llu records in %llu batches: %llu excluded, %llu without a sequence, %llu read ones, %llu read twos, "
                            "%llu others; %llu resident records of %llu bytes, %llu sort passes, %llu name collisions, %llu pieces; "
                            "%llu + %llu + %llu + %llu text bytes, %llu + %llu + %llu + %llu compressed; walk %.1f ms (ingest %.1f ms), match %.1f ms, format %.1f ms, "
                            "deflate %.1f ms, copy %.1f ms, write %.1f ms, total %.1f ms\n",
                    (unsigned long long)crep.records_scanned, (unsigned long long)crep.batches, (unsigned long long)crep.excluded,
                    (unsigned long long)crep.no_sequence, (unsigned long long)crep.reads_one, (unsigned long long)crep.reads_two,
                    (unsigned long long)crep.reads_other, (unsigned long long)crep.resident_records, (unsigned long long)crep.resident_bytes,
                    (unsigned long long)crep.sort_passes, (unsigned long long)crep.name_collisions, (unsigned long long)crep.pieces,
                    (unsigned long long)crep.text_bytes[0], (unsigned long long)crep.text_bytes[1], (unsigned long long)crep.text_bytes[2],
                    (unsigned long long)crep.text_bytes[3], (unsigned long long)crep.compressed_bytes[0], (unsigned long long)crep.compressed_bytes[1],
                    (unsigned long long)crep.compressed_bytes[2], (unsigned long long)crep.compressed_bytes[3], crep.walk_ms, crep.scan_ms, crep.match_ms,
                    crep.format_ms, crep.deflate_ms, crep.copy_ms, crep.write_ms, crep.total_ms);
        return 0;
    }
    if (two_files && rep.reads_one != rep.reads_two)
        logf(2, "%llu read ones and %llu read twos were written: the two files do not pair line by line", (unsigned long long)rep.reads_one,
             (unsigned long long)rep.reads_two);
    if (rep.dropped_other)
        logf(2, "%llu reads that are neither a read one nor a read two were dropped (--other <FILE> keeps them)", (unsigned long long)rep.dropped_other);
    if (g_level >= 3)
        fprintf(stderr, "[ngs] fastq: %llu records in %llu batches: %llu excluded, %llu without a sequence, %llu read ones, %llu read twos, %llu others "
                        "(%llu dropped); %llu + %llu + %llu text bytes; ingest %.1f ms, format %.1f ms, deflate %.1f ms, copy %.1f ms, write %.1f ms, "
                        "total %.1f ms\n",
                (unsigned long long)rep.records_scanned, (unsigned long long)rep.batches, (unsigned long long)rep.excluded,
                (unsigned long long)rep.no_sequence, (unsigned long long)rep.reads_one, (unsigned long long)rep.reads_two,
                (unsigned long long)rep.reads_other, (unsigned long long)rep.dropped_other, (unsigned long long)rep.text_bytes[0],
                (unsigned long long)rep.text_bytes[1], (unsigned long long)rep.text_bytes[2], rep.scan_ms, rep.format_ms, rep.deflate_ms, rep.copy_ms,
                rep.write_ms, rep.total_ms);
    if (g_level >= 3 && on_device)
        fprintf(stderr, "[ngs] fastq: BGZF on the device at effort %s: %llu + %llu + %llu compressed bytes in %llu blocks (%llu stored)\n",
                effort == NGSQ_BGZF_EFFORT_HIGH ? "high" : "normal", (unsigned long long)rep.compressed_bytes[0], (unsigned long long)rep.compressed_bytes[1],
                (unsigned long long)rep.compressed_bytes[2], (unsigned long long)rep.blocks, (unsigned long long)rep.stored_blocks);
    return 0;
}
