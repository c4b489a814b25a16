// view.cpp -- `ngs view` (src/view/command.rs:16-98, src/view/bam.rs:16-82): the SAM text of a BAM file or
// of one region of it on stdout, the records found through the BAI, selected and formatted on the GPU by ngsq_bam_view
// (include/ngsq_view.h).  BAM only in this build.
#include <csignal>

#include "../../../include/ngsq_view.h"
#include "cli.h"

namespace {

struct ViewArgs {
    std::vector<std::string> pos;
    bool has_fasta = false; // (-r takes no part in viewing a BAM file, as in the reference)
    uint32_t mode = NGSQ_VIEW_FULL;
    int device = 0;
};

// false: --help has been answered
bool parse_args(int argc, char **argv, int at, ViewArgs *a) {
    for (int i = at + 1; i < argc; i++) {
        const std::string s = argv[i];
        auto val = [&](const char *name) { return option_value(argc, argv, &i, name); };
        if (verbosity_option(argv[i])) continue;
        if (s == "-h" || s == "--help") {
            fprintf(stderr,
                    "Usage: ngs view [OPTIONS] <FILE> [QUERY]\n\n"
                    "Arguments:\n"
                    "  <FILE>   Path to the file to view\n"
                    "  [QUERY]  If available, the query region for this view\n\n"
                    "Options:\n"
                    "  -r, --reference-fasta <REFERENCE_FASTA>\n"
                    "          If available, the FASTA reference file used to generate the file\n"
                    "  -m, --mode <MODE>\n"
                    "          Shows either the header (\"header-only\"), the records (\"records-only\"), or both (\"full\")\n"
                    "          [default: full] [possible values: full, header-only, records-only]\n"
                    "      --device <N>\n"
                    "          GPU the records are selected and formatted on (additive, this build) [default: 0]\n\n"
                    "This build views BAM files only.\n");
            return false;
        } else if (s == "-m" || s == "--mode") {
            const std::string v = val("--mode <MODE>");
            if (v == "full") a->mode = NGSQ_VIEW_FULL;
            else if (v == "header-only") a->mode = NGSQ_VIEW_HEADER_ONLY;
            else if (v == "records-only") a->mode = NGSQ_VIEW_RECORDS_ONLY;
            else bail("invalid value '" + v + "' for '--mode <MODE>' [possible values: full, header-only, records-only]");
        } else if (s == "-r" || s == "--reference-fasta") {
            (void)val("--reference-fasta <REFERENCE_FASTA>");
            a->has_fasta = true;
        } else if (s == "--device") {
            a->device = atoi(val("--device <N>").c_str());
        } else if (!s.empty() && s[0] == '-' && s != "-") bail("unexpected argument '" + s + "' found");
        else a->pos.push_back(s);
    }
    return true;
}

} // namespace

// argv[at] is "view".  Exit 0 on success, 1 on every error (anyhow::bail! in the reference).
int view_main(int argc, char **argv, int at) {
    ViewArgs a;
    if (!parse_args(argc, argv, at, &a)) return 0;
    const std::vector<std::string> &pos = a.pos;
    if (pos.empty()) bail("the following required arguments were not provided: <FILE>");
    if (pos.size() > 2) bail("unexpected argument '" + pos[2] + "' found");
    const std::string &src = pos[0];
    // BioinformaticsFileFormat::try_detect of <FILE> (command.rs:63-97)
    const std::string ff = detect_format(src);
    if (ff.empty()) bail("Not able to determine bioinformatics file type for path: " + src);
    if (ff == "CRAM" && !a.has_fasta) bail("--reference-fasta is a required argument when converting to/from a CRAM file");
    if (ff == "SAM" || ff == "CRAM" || ff == "GFF" || ff == "Gzipped GFF" || ff == "GTF" || ff == "Gzipped GTF")
        bail(ff + " files are viewed by the reference `ngs view` but not by this build, which views BAM files only");
    if (ff != "BAM")
        bail(ff + " files are not supported by this command. This may be because we haven't supported this file format yet or because "
                  "it does not make sense to view a file of this kind. If you believe this format should be supported, please search "
                  "for and upvote the related issue on Github (or file a new one).");
    // (1) open the BAM (IndexCheck::HeaderOnly: no index is needed without a query)
    ngsq_bam *bam = nullptr;
    if (ngsq_bam_open(src.c_str(), 0, &bam) != NGSQ_OK) bail(std::string("opening BAM input file: ") + ngsq_bam_last_error());
    // (2) stdout; a reader that goes away ends the command with the write's error, not with a signal
    signal(SIGPIPE, SIG_IGN);
    // (3)-(5) header and records; the device is acquired before the first byte is written
    ngsq_ctx *ctx = nullptr;
    if (a.mode != NGSQ_VIEW_HEADER_ONLY) {
        ctx = plain_context(bam, a.device);
        if (!ctx) bail(ngsq_last_global_error());
    }
    ngsq_view_report rep{};
    const int rc = ngsq_bam_view(bam, ctx, STDOUT_FILENO, pos.size() > 1 ? pos[1].c_str() : nullptr, nullptr, a.mode, 0, 0, &rep);
    const std::string msg = rc ? ngsq_bam_last_error() : "";
    if (ctx) ngsq_destroy(ctx);
    ngsq_bam_close(bam);
    if (rc) bail(msg);
    if (g_level >= 3)
        fprintf(stderr, "[ngs] view: %llu of %llu records in %llu batches, %llu chunks in %llu range walks, %llu header + %llu text bytes; "
                        "ingest %.1f ms, select %.1f ms, format %.1f ms, copy %.1f ms, write %.1f ms, total %.1f ms\n",
                (unsigned long long)rep.records_written, (unsigned long long)rep.records_scanned, (unsigned long long)rep.batches,
                (unsigned long long)rep.chunks, (unsigned long long)rep.ranges, (unsigned long long)rep.header_bytes,
                (unsigned long long)rep.text_bytes, rep.scan_ms, rep.select_ms, rep.format_ms, rep.copy_ms, rep.write_ms, rep.total_ms);
    return 0;
}
