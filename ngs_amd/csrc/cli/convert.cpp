// convert.cpp -- `ngs convert` (src/convert/command.rs:26-172, src/convert/bam.rs:24-70): BAM to SAM, the
// text formatted on the GPU by ngsq_bam_write_sam (include/ngsq_sam.h); and, behind the additive `--gzip device`, SAM to BAM
// (src/convert/sam.rs:26-90): the text parsed and the BGZF written on the GPU by ngsq_sam_write_bam
// (include/ngsq_samtext.h); with the additive `--sort coordinate` beside it the records are sorted there too
// (ngsq_sam_write_sorted_bam); and with both flags BAM to sorted BAM (ngsq_bam_write_sorted_bam,
// include/ngsq_bamsort.h); with the additive `--write-index` beside those two the BAI of the sorted BAM is
// written with it; a BAM whose records do not fit the device's memory, or the additive `--sort-memory`,
// is sorted in rounds (ngsq_bam_write_sorted_bam_rounds).  Without the flags every command line answers as a build without that direction.
#include <fcntl.h>
#include <sys/stat.h>

#include <algorithm>
#include <cerrno>

#include "../../../include/ngsq_bamsort.h"
#include "../../../include/ngsq_bgzf.h"
#include "../../../include/ngsq_sam.h"
#include "../../../include/ngsq_samtext.h"
#include "cli.h"

namespace {

struct ConvertArgs {
    std::vector<std::string> pos;
    bool has_n = false, has_fasta = false; // (-r and -c take no part in BAM to SAM, as in the reference)
    bool gzip_device = false;              // --gzip device: SAM to BAM is converted, its BGZF written on the GPU
    bool sort_coordinate = false;          // --sort coordinate: ... and its records sorted there
    bool write_index = false;              // --write-index: ... and <TO>.bai written beside the sorted BAM
    bool has_sort_memory = false;          // --sort-memory: what the resident records may take of device memory
    unsigned long long sort_memory = 0;
    bool has_effort = false;               // --gzip-effort: how hard the GPU's encoder searches
    uint32_t effort = NGSQ_BGZF_EFFORT_NORMAL;
    unsigned long long n = 0;
    int device = 0;
};

// false: --help has been answered
bool parse_args(int argc, char **argv, int at, ConvertArgs *a) {
    for (int i = at + 1; i < argc; i++) {
        const std::string s = argv[i];
        auto val = [&](const char *name) { return option_value(argc, argv, &i, name); };
        if (verbosity_option(argv[i])) continue;
        if (s == "-h" || s == "--help") {
            fprintf(stderr,
                    "Usage: ngs convert [OPTIONS] <FROM> <TO>\n\n"
                    "Arguments:\n"
                    "  <FROM>  Path to the source file from which we are converting\n"
                    "  <TO>    Path to the destination file to which we are converting\n\n"
                    "Options:\n"
                    "  -n, --num-records <USIZE>\n"
                    "          Number of records to process before exiting the conversion\n"
                    "  -r, --reference-fasta <REFERENCE_FASTA>\n"
                    "          If available, the FASTA reference file used to generate the file\n"
                    "  -c, --compression-strategy <COMPRESSION_STRATEGY>\n"
                    "          [default: balanced] [possible values: best, balanced, fastest]\n"
                    "      --device <N>\n"
                    "          GPU the SAM text is formatted on (additive, this build) [default: 0]\n"
                    "      --gzip <WHERE>\n"
                    "          Where BGZF output is compressed (additive, this build): `device` converts SAM to BAM on the GPU;\n"
                    "          `host` changes nothing [default: host] [possible values: host, device]\n"
                    "      --gzip-effort <EFFORT>\n"
                    "          With --gzip device (additive, this build): `high` has the GPU's encoder search harder for matches, which\n"
                    "          gives a smaller BAM for more encoder time [default: normal] [possible values: normal, high]\n"
                    "      --sort <ORDER>\n"
                    "          Order of the records of a BAM written with --gzip device (additive, this build): `coordinate` sorts them\n"
                    "          on the GPU, unplaced records last, and writes SO:coordinate; with it BAM to BAM is converted too, a BAM in\n"
                    "          any record order to a sorted one [default: none] [possible values: none, coordinate]\n"
                    "      --write-index\n"
                    "          With --gzip device and --sort coordinate (additive, this build): write the index <TO>.bai beside the sorted\n"
                    "          BAM, the file `ngs index <TO>` would write, built on the GPU while the BAM is written\n"
                    "      --sort-memory <SIZE>\n"
                    "          With --gzip device and --sort coordinate (additive, this build): device memory the records being sorted may\n"
                    "          take, in bytes or with a K, M or G suffix; a BAM beyond it is sorted in rounds, each a walk of the input that\n"
                    "          keeps one range of the sorted order [default: the free memory of the device, less 4 GiB]\n\n"
                    "This build converts BAM to SAM, and with --gzip device SAM to BAM: the text is parsed and the BGZF blocks are\n"
                    "written on the GPU, whose encoder has one setting (-c is checked and takes no part).  With --gzip device and\n"
                    "--sort coordinate it also converts BAM to BAM: the file is inflated, sorted and compressed on the GPU.\n"
                    "One setting as far as -c goes: how hard the encoder searches is chosen with --gzip-effort.\n");
            return false;
        } else if (s == "-n" || s == "--num-records") {
            const std::string v = val("--num-records <USIZE>");
            char *e = nullptr;
            errno = 0;
            a->n = strtoull(v.c_str(), &e, 10);
            if (v.empty() || *e || errno || v[0] == '-' || v[0] == '+')
                bail("invalid value '" + v + "' for '--num-records <USIZE>': invalid digit found in string");
            a->has_n = true;
        } else if (s == "-r" || s == "--reference-fasta") {
            (void)val("--reference-fasta <REFERENCE_FASTA>");
            a->has_fasta = true;
        } else if (s == "-c" || s == "--compression-strategy") {
            const std::string v = val("--compression-strategy <COMPRESSION_STRATEGY>");
            if (v != "best" && v != "balanced" && v != "fastest")
                bail("invalid value '" + v + "' for '--compression-strategy <COMPRESSION_STRATEGY>' [possible values: best, balanced, fastest]");
        } else if (s == "--device") {
            a->device = atoi(val("--device <N>").c_str());
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
        } else if (s == "--sort") {
            const std::string v = val("--sort <ORDER>");
            if (v == "none") a->sort_coordinate = false;
            else if (v == "coordinate") a->sort_coordinate = true;
            else bail("invalid value '" + v + "' for '--sort <ORDER>' [possible values: none, coordinate]");
        } else if (s == "--write-index") {
            a->write_index = true;
        } else if (s == "--sort-memory") {
            a->sort_memory = size_value(val("--sort-memory <SIZE>"), "--sort-memory <SIZE>");
            a->has_sort_memory = true;
        } else if (!s.empty() && s[0] == '-' && s != "-") bail("unexpected argument '" + s + "' found");
        else a->pos.push_back(s);
    }
    return true;
}

// --write-index: an index that exists is refused in the words of `ngs index`, before <TO> is opened
bool index_exists(const std::string &bai) {
    struct stat sb;
    return stat(bai.c_str(), &sb) == 0;
}
std::string existing_index_refusal(const std::string &bai) {
    return "refusing to overwrite existing index file: " + bai + ". Please delete and rerun if you'd like to replace it.";
}

const char *effort_name(const ConvertArgs &a) { return a.effort == NGSQ_BGZF_EFFORT_HIGH ? "high" : "normal"; }

void log_index_report(const ngsq_index_report &irep) {
    if (g_level >= 3)
        fprintf(stderr, "[ngs] convert: index of %llu records (%llu without coordinates), %llu chunks in %llu bins; device %.1f ms, write %.1f ms\n",
                (unsigned long long)irep.records, (unsigned long long)irep.n_no_coor, (unsigned long long)irep.runs, (unsigned long long)irep.bins,
                irep.scan_ms, irep.write_ms);
}

// to_bam_async (sam.rs:26-90): (1) open the SAM and read its header, (2) create the BAM file, (3) the header, (4) every record
int sam_to_bam(const ConvertArgs &a, const std::string &from, const std::string &to) {
    char why[1024];
    if (ngsq_sam_check_header(from.c_str(), nullptr, why, sizeof why) != NGSQ_OK) bail(why);
    const std::string bai = to + ".bai";
    if (a.write_index && index_exists(bai)) bail(existing_index_refusal(bai));
    const int fd = open(to.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    if (fd < 0) {
        const int e = errno;
        bail(std::string("opening BAM output file: ") + strerror(e) + " (os error " + std::to_string(e) + ")");
    }
    ngsq_config cfg{};
    cfg.struct_size = sizeof cfg;
    cfg.device = a.device;
    ngsq_ctx *ctx = nullptr;
    if (ngsq_create(&cfg, &ctx) != NGSQ_OK) {
        close(fd);
        bail(ngsq_last_global_error());
    }
    if (ngsq_bgzf_set_effort(ctx, a.effort) != NGSQ_OK) {
        const std::string m = ngsq_last_error(ctx);
        ngsq_destroy(ctx);
        close(fd);
        bail(m);
    }
    const uint64_t max_records = a.has_n ? std::max<unsigned long long>(a.n, 1) : 0;
    ngsq_samtext_report rep{};
    ngsq_samsort_report srep{};
    ngsq_index_report irep{};
    // (--sort-memory is the budget and nothing else here: SAM input stays in memory)
    const int rc = a.write_index       ? ngsq_sam_write_sorted_bam_indexed(ctx, from.c_str(), fd, max_records, 0, 0, a.sort_memory, &srep, bai.c_str(), 0, &irep)
                   : a.sort_coordinate ? ngsq_sam_write_sorted_bam(ctx, from.c_str(), fd, max_records, 0, 0, a.sort_memory, &srep)
                                       : ngsq_sam_write_bam(ctx, from.c_str(), fd, max_records, 0, &rep);
    const std::string msg = rc ? ngsq_last_error(ctx) : "";
    const int close_rc = close(fd), close_errno = errno;
    ngsq_destroy(ctx);
    if (rc) bail(msg);
    if (close_rc) bail(std::string("writing BAM record: ") + strerror(close_errno) + " (os error " + std::to_string(close_errno) + ")");
    const uint64_t written = a.sort_coordinate ? srep.records : rep.records;
    for (uint64_t m = 1; m <= written / 1000000; m++) logf(2, "  [*] Processed %s records.", with_commas(m * 1000000).c_str());
    if (g_level >= 3 && a.sort_coordinate)
        fprintf(stderr, "[ngs] convert: %llu records in %llu chunks sorted in %u of 8 passes, %llu header + %llu text bytes -> %llu BAM bytes in %llu pieces, "
                        "%llu blocks (%llu stored), %llu compressed at effort %s; read %.1f ms, up %.1f ms, parse %.1f ms, sort %.1f ms, gather %.1f ms, "
                        "deflate %.1f ms, down %.1f ms, write %.1f ms, total %.1f ms\n",
                (unsigned long long)srep.records, (unsigned long long)srep.chunks, srep.passes_run, (unsigned long long)srep.header_bytes,
                (unsigned long long)srep.text_bytes, (unsigned long long)srep.bam_bytes, (unsigned long long)srep.pieces, (unsigned long long)srep.blocks,
                (unsigned long long)srep.stored_blocks, (unsigned long long)srep.compressed_bytes, effort_name(a), srep.read_ms, srep.h2d_ms, srep.parse_ms, srep.sort_ms,
                srep.gather_ms, srep.deflate_ms, srep.d2h_ms, srep.write_ms, srep.total_ms);
    else if (g_level >= 3)
        fprintf(stderr, "[ngs] convert: %llu records in %llu chunks, %llu header + %llu text bytes -> %llu BAM bytes in %llu blocks (%llu stored), "
                        "%llu compressed at effort %s; read %.1f ms, up %.1f ms, parse %.1f ms, deflate %.1f ms, down %.1f ms, write %.1f ms, total %.1f ms\n",
                (unsigned long long)rep.records, (unsigned long long)rep.chunks, (unsigned long long)rep.header_bytes,
                (unsigned long long)rep.text_bytes, (unsigned long long)rep.bam_bytes, (unsigned long long)rep.blocks,
                (unsigned long long)rep.stored_blocks, (unsigned long long)rep.compressed_bytes, effort_name(a), rep.read_ms, rep.h2d_ms, rep.parse_ms,
                rep.deflate_ms, rep.d2h_ms, rep.write_ms, rep.total_ms);
    if (a.write_index) log_index_report(irep);
    return 0;
}

// BAM to sorted BAM: (1) open the BAM, (2) <TO> must be another file, (3) create it, (4) every record, sorted
int bam_to_sorted_bam(const ConvertArgs &a, const std::string &from, const std::string &to) {
    ngsq_bam *bam = nullptr;
    if (ngsq_bam_open(from.c_str(), 0, &bam) != NGSQ_OK) bail(std::string("opening BAM input file: ") + ngsq_bam_last_error());
    struct stat sf, stt;
    if (stat(from.c_str(), &sf) == 0 && stat(to.c_str(), &stt) == 0 && sf.st_dev == stt.st_dev && sf.st_ino == stt.st_ino) {
        ngsq_bam_close(bam);
        bail("Conversion from BAM to BAM needs two files: " + to + " is the input");
    }
    const std::string bai = to + ".bai";
    if (a.write_index && index_exists(bai)) {
        ngsq_bam_close(bam);
        bail(existing_index_refusal(bai));
    }
    const int fd = open(to.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    if (fd < 0) {
        const int e = errno;
        ngsq_bam_close(bam);
        bail(std::string("opening BAM output file: ") + strerror(e) + " (os error " + std::to_string(e) + ")");
    }
    ngsq_ctx *ctx = plain_context(bam, a.device);
    if (!ctx) {
        close(fd);
        bail(ngsq_last_global_error());
    }
    if (ngsq_bgzf_set_effort(ctx, a.effort) != NGSQ_OK) {
        const std::string m = ngsq_last_error(ctx);
        ngsq_destroy(ctx);
        ngsq_bam_close(bam);
        close(fd);
        bail(m);
    }
    const uint64_t max_records = a.has_n ? std::max<unsigned long long>(a.n, 1) : 0;
    ngsq_bamsort_report rep{};
    ngsq_index_report irep{};
    ngsq_bamsort_rounds rrep{};
    const int rc = ngsq_bam_write_sorted_bam_rounds(bam, ctx, fd, max_records, 0, 0, a.sort_memory, &rep, a.write_index ? bai.c_str() : nullptr, 0, &irep, &rrep);
    const std::string msg = rc ? ngsq_bam_last_error() : "";
    const int close_rc = close(fd), close_errno = errno;
    ngsq_destroy(ctx);
    ngsq_bam_close(bam);
    if (rc) bail(msg);
    if (close_rc) bail(std::string("writing BAM record: ") + strerror(close_errno) + " (os error " + std::to_string(close_errno) + ")");
    for (uint64_t m = 1; m <= rep.records / 1000000; m++) logf(2, "  [*] Processed %s records.", with_commas(m * 1000000).c_str());
    if (g_level >= 3)
        fprintf(stderr, "[ngs] convert: %llu records in %llu batches and %llu slabs sorted in %u of 8 passes, %llu header bytes -> %llu BAM bytes in "
                        "%llu pieces, %llu blocks (%llu stored), %llu compressed at effort %s; ingest %.1f ms, keep %.1f ms, sort %.1f ms, gather %.1f ms, "
                        "deflate %.1f ms, down %.1f ms, write %.1f ms, total %.1f ms\n",
                (unsigned long long)rep.records, (unsigned long long)rep.batches, (unsigned long long)rep.slabs, rep.passes_run,
                (unsigned long long)rep.header_bytes, (unsigned long long)rep.bam_bytes, (unsigned long long)rep.pieces, (unsigned long long)rep.blocks,
                (unsigned long long)rep.stored_blocks, (unsigned long long)rep.compressed_bytes, effort_name(a), rep.scan_ms, rep.keep_ms, rep.sort_ms, rep.gather_ms,
                rep.deflate_ms, rep.d2h_ms, rep.write_ms, rep.total_ms);
    if (g_level >= 3 && rrep.rounds > 1)
        fprintf(stderr, "[ngs] convert: %llu rounds over %llu walks of the input, budget %llu bytes, survey %llu bytes in %.1f ms\n",
                (unsigned long long)rrep.rounds, (unsigned long long)rrep.walks, (unsigned long long)rrep.budget, (unsigned long long)rrep.survey_bytes,
                rrep.survey_ms);
    if (a.write_index) log_index_report(irep);
    return 0;
}

} // namespace

// argv[at] is "convert".  Exit 0 on success, 1 on every error (anyhow::bail! in the reference).
int convert_main(int argc, char **argv, int at) {
    ConvertArgs a;
    if (!parse_args(argc, argv, at, &a)) return 0;
    const std::vector<std::string> &pos = a.pos;
    if (pos.size() < 2) bail(pos.empty() ? "the following required arguments were not provided: <FROM> <TO>"
                                         : "the following required arguments were not provided: <TO>");
    if (pos.size() > 2) bail("unexpected argument '" + pos[2] + "' found");
    const std::string &from = pos[0], &to = pos[1];
    // BioinformaticsFileFormat::try_detect of <FROM>, then of <TO> (command.rs:63-82), with their contexts
    const std::string ff = detect_format(from);
    if (ff.empty()) bail("failed to detect from input filetype: " + from + ": Failed parsing of bioinformatics file format.");
    const std::string tf = detect_format(to);
    if (tf.empty()) bail("failed to deteect to input filetype: " + to + ": Failed parsing of bioinformatics file format.");
    // the pairs the reference converts (command.rs:104-171)
    const bool cram = (ff == "SAM" && tf == "CRAM") || (ff == "CRAM" && tf == "SAM") || (ff == "BAM" && tf == "CRAM") ||
                      (ff == "CRAM" && tf == "BAM");
    const bool reference_only = (ff == "SAM" && tf == "BAM") || (ff == "GFF" && tf == "Block-gzipped GFF") || cram;
    if (cram && !a.has_fasta) bail("--reference-fasta is a required argument when converting to/from a CRAM file");
    // (additive) the index is written where a sorted path is reached; refused before any file is opened
    if (a.write_index && !(a.gzip_device && a.sort_coordinate && tf == "BAM" && (ff == "SAM" || ff == "BAM")))
        bail("--write-index needs --gzip device and --sort coordinate and a BAM to write");
    if (a.has_sort_memory && !(a.gzip_device && a.sort_coordinate && tf == "BAM" && (ff == "SAM" || ff == "BAM")))
        bail("--sort-memory needs --gzip device and --sort coordinate and a BAM to write");
    // (additive) the effort is the device encoder's: refused where no path that runs it is reached
    if (a.has_effort && !(a.gzip_device && tf == "BAM" && (ff == "SAM" || (ff == "BAM" && a.sort_coordinate)))) bail("--gzip-effort needs --gzip device");
    if (ff == "SAM" && tf == "BAM" && a.gzip_device) return sam_to_bam(a, from, to);
    if (ff == "BAM" && tf == "BAM" && a.gzip_device && a.sort_coordinate) return bam_to_sorted_bam(a, from, to);
    if (reference_only)
        bail("Conversion from " + ff + " to " + tf + " is done by the reference `ngs convert` but not by this build, which converts BAM to SAM only");
    if (!(ff == "BAM" && tf == "SAM")) bail("Conversion from " + ff + " to " + tf + " is not currently supported");
    // to_sam_async: (1) open the BAM (IndexCheck::None), (2) create the SAM file, (3) the header, (4) every record
    ngsq_bam *bam = nullptr;
    if (ngsq_bam_open(from.c_str(), 0, &bam) != NGSQ_OK) bail(std::string("opening BAM input file: ") + ngsq_bam_last_error());
    const int fd = open(to.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    if (fd < 0) {
        const int e = errno;
        ngsq_bam_close(bam);
        bail(std::string("creating SAM output file: ") + strerror(e) + " (os error " + std::to_string(e) + ")");
    }
    ngsq_ctx *ctx = plain_context(bam, a.device);
    if (!ctx) {
        close(fd);
        bail(ngsq_last_global_error());
    }
    // RecordCounter::time_to_break (utils/display.rs:58-63) is tested behind the write: -n N writes max(N, 1) records
    const uint64_t max_records = a.has_n ? std::max<unsigned long long>(a.n, 1) : 0;
    ngsq_sam_report rep{};
    const int rc = ngsq_bam_write_sam(bam, ctx, fd, max_records, 0, &rep);
    const std::string msg = rc ? ngsq_bam_last_error() : "";
    const int close_rc = close(fd), close_errno = errno;
    ngsq_destroy(ctx);
    ngsq_bam_close(bam);
    if (rc) bail(msg);
    if (close_rc) bail(std::string("writing SAM record: ") + strerror(close_errno) + " (os error " + std::to_string(close_errno) + ")");
    // RecordCounter::inc (display.rs:43-52): one line per million records written
    for (uint64_t m = 1; m <= rep.records / 1000000; m++) logf(2, "  [*] Processed %s records.", with_commas(m * 1000000).c_str());
    if (g_level >= 3)
        fprintf(stderr, "[ngs] convert: %llu records in %llu batches, %llu header + %llu text bytes; ingest %.1f ms, format %.1f ms, copy %.1f ms, "
                        "write %.1f ms, total %.1f ms\n",
                (unsigned long long)rep.records, (unsigned long long)rep.batches, (unsigned long long)rep.header_bytes,
                (unsigned long long)rep.text_bytes, rep.scan_ms, rep.format_ms, rep.copy_ms, rep.write_ms, rep.total_ms);
    return 0;
}
