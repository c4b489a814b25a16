// index.cpp -- `ngs index` (src/index/command.rs:26-46, src/index/bam.rs:39-109): <BAM>.bai, built on
// the GPU by ngsq_bam_build_index (include/ngsq_index.h).  BAM only in this build.
#include <sys/stat.h>

#include "../../../include/ngsq_index.h"
#include "cli.h"

// argv[at] is "index".  Exit 0 on success, 1 on every error (anyhow::bail! in the reference).
int index_main(int argc, char **argv, int at) {
    std::string src;
    int device = 0, n_pos = 0;
    for (int i = at + 1; i < argc; i++) {
        const std::string s = argv[i];
        if (verbosity_option(argv[i])) continue;
        if (s == "-h" || s == "--help") {
            fprintf(stderr, "Usage: ngs index [--device <N>] <BAM/CRAM/FASTA>\n\n"
                            "Arguments:\n  <BAM/CRAM/FASTA>  Path to the file to index (BAM only in this build)\n\n"
                            "Options:\n      --device <N>  GPU the index is built on (additive, this build) [default: 0]\n");
            return 0;
        } else if (s == "--device") {
            device = atoi(option_value(argc, argv, &i, "--device <N>").c_str());
        } else if (!s.empty() && s[0] == '-') bail("unexpected argument '" + s + "' found");
        else {
            src = s;
            n_pos++;
        }
    }
    if (n_pos == 0) bail("the following required arguments were not provided: <BAM/CRAM/FASTA>");
    if (n_pos > 1) bail("unexpected argument found: `ngs index` takes one file");
    // BioinformaticsFileFormat::try_detect by extension (utils/formats.rs), as for qc
    const std::string format = detect_format(src);
    if (format.empty()) bail("Not able to determine bioinformatics file type for path: " + src);
    if (format == "CRAM" || format == "FASTA")
        bail(format + " files are indexed by the reference `ngs index` but not by this build, which indexes BAM files only");
    if (format != "BAM")
        bail(format + " files are not supported by this command. This may be because we haven't supported this file format yet or "
                      "because it does not make sense to index a file of this kind. If you believe this format should be supported, "
                      "please search for and upvote the related issue on Github (or file a new one).");
    // (1) open and parse (IndexCheck::None), (2) refuse an existing index, (3) require SO:coordinate -- before any GPU work
    ngsq_bam *bam = nullptr;
    if (ngsq_bam_open(src.c_str(), 0, &bam) != NGSQ_OK) bail(ngsq_bam_last_error());
    const std::string bai = src + ".bai";
    struct stat sb;
    if (stat(bai.c_str(), &sb) == 0)
        bail("refusing to overwrite existing index file: " + bai + ". Please delete and rerun if you'd like to replace it.");
    if (!ngsq_bam_sorted_by_coordinate(bam)) bail("the input BAM must be coordinate-sorted to be indexed");
    // (5) the index: the device ingest and the index kernels on one GPU; a context without facets
    ngsq_ctx *ctx = plain_context(bam, device);
    if (!ctx) bail(ngsq_last_global_error());
    ngsq_index_report rep{};
    if (ngsq_bam_build_index(bam, ctx, bai.c_str(), &rep) != NGSQ_OK) {
        const std::string msg = ngsq_bam_last_error();
        ngsq_destroy(ctx);
        ngsq_bam_close(bam);
        bail(msg);
    }
    if (g_level >= 3)
        fprintf(stderr, "[ngs] index: %llu records (%llu without coordinates), %llu chunks in %llu bins; scan %.1f ms, write %.1f ms\n",
                (unsigned long long)rep.records, (unsigned long long)rep.n_no_coor, (unsigned long long)rep.runs,
                (unsigned long long)rep.bins, rep.scan_ms, rep.write_ms);
    ngsq_destroy(ctx);
    ngsq_bam_close(bam);
    return 0;
}
