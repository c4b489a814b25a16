// derive.cpp -- `ngs derive instrument` (src/derive/command/instrument.rs:17-110): the sequencer that
// produced a BAM, predicted from the instrument ids and flowcell ids of its read names.  The names are scanned on the GPU
// by ngsq_bam_derive_instrument, the prediction is ngsq_derive_predict's (include/ngsq_derive.h).
#include <cerrno>

#include "../../../include/ngsq_derive.h"
#include "cli.h"

namespace {

unsigned long long usize_value(const std::string &v, const char *name) {
    char *e = nullptr;
    errno = 0;
    const unsigned long long x = strtoull(v.c_str(), &e, 10);
    if (v.empty() || *e || errno || v[0] == '-' || v[0] == '+')
        bail("invalid value '" + v + "' for '" + name + "': invalid digit found in string");
    return x;
}

} // namespace

// argv[at] is "derive".  Exit 0 once the document is printed (also when it says succeeded: false), 1 on every error.
int derive_main(int argc, char **argv, int at) {
    std::vector<std::string> pos;
    unsigned long long n = 0;
    int device = 0;
    for (int i = at + 1; i < argc; i++) {
        const std::string s = argv[i];
        if (verbosity_option(argv[i])) continue;
        if (s == "-h" || s == "--help") {
            fprintf(stderr, "Usage: ngs derive instrument [OPTIONS] <BAM>\n\n"
                            "Arguments:\n"
                            "  <BAM>  Source BAM\n\n"
                            "Options:\n"
                            "  -n, --num-records <USIZE>\n"
                            "          Only examine the first n records in the file\n"
                            "  -t, --threads <USIZE>\n"
                            "          Use a specific number of threads (accepted; the names are scanned on the GPU)\n"
                            "      --device <N>\n"
                            "          GPU the names are scanned on (additive, this build) [default: 0]\n");
            return 0;
        } else if (s == "-n" || s == "--num-records") {
            n = usize_value(option_value(argc, argv, &i, "--num-records <USIZE>"), "--num-records <USIZE>");
        } else if (s == "-t" || s == "--threads") {
            (void)usize_value(option_value(argc, argv, &i, "--threads <USIZE>"), "--threads <USIZE>");
        } else if (s == "--device") {
            device = atoi(option_value(argc, argv, &i, "--device <N>").c_str());
        } else if (!s.empty() && s[0] == '-' && s != "-") bail("unexpected argument '" + s + "' found");
        else pos.push_back(s);
    }
    if (pos.empty() || pos[0] != "instrument")
        bail(pos.empty() ? "`ngs derive` requires a subcommand: this build provides `ngs derive instrument`"
                         : "unrecognized subcommand '" + pos[0] + "': this build provides `ngs derive instrument`");
    if (pos.size() < 2) bail("the following required arguments were not provided: <BAM>");
    if (pos.size() > 2) bail("unexpected argument '" + pos[2] + "' found");
    const std::string &src = pos[1];
    // open_and_parse(src, IndexCheck::Full) (utils/formats/bam.rs:32-56, :77-96): the format by extension, the header, <BAM>.bai
    const std::string format = detect_format(src);
    if (format.empty()) bail("Not able to determine filetype for extension: " + extension_of(src));
    if (format != "BAM") bail("incompatible formats: required BAM, found " + format);
    ngsq_bam *bam = nullptr;
    if (ngsq_bam_open(src.c_str(), 0, &bam) != NGSQ_OK) bail(ngsq_bam_last_error());
    if (ngsq_bam_check_index(src.c_str()) != NGSQ_OK) bail(ngsq_bam_last_error());
    // (1) the names: the counter is tested behind the record (instrument.rs:92-97), so -n N examines N + 1 records; 0: all
    ngsq_ctx *ctx = plain_context(bam, device);
    if (!ctx) bail(ngsq_last_global_error());
    ngsq_derive_names *names = nullptr;
    ngsq_derive_report rep{};
    const int rc = ngsq_bam_derive_instrument(bam, ctx, n ? n + 1 : 0, 0, 0, &names, &rep);
    const std::string msg = rc ? ngsq_bam_last_error() : "";
    ngsq_destroy(ctx);
    ngsq_bam_close(bam);
    if (rc) bail(msg);
    // (2) the prediction, (3) the document on stdout, without a final newline
    std::vector<const char *> p[2];
    std::vector<uint32_t> l[2];
    for (int k = 0; k < 2; k++) {
        const uint64_t cnt = ngsq_derive_names_count(names, k);
        for (uint64_t i = 0; i < cnt; i++) {
            uint32_t len = 0;
            p[k].push_back(ngsq_derive_names_get(names, k, i, &len));
            l[k].push_back(len);
        }
    }
    size_t need = 0;
    (void)ngsq_derive_predict(p[0].data(), l[0].data(), p[0].size(), p[1].data(), l[1].data(), p[1].size(), nullptr, 0, &need);
    std::string doc(need, '\0');
    if (ngsq_derive_predict(p[0].data(), l[0].data(), p[0].size(), p[1].data(), l[1].data(), p[1].size(), &doc[0], doc.size(), &need) != NGSQ_OK)
        bail("the instrument prediction could not be written");
    ngsq_derive_names_free(names);
    fputs(doc.c_str(), stdout);
    fflush(stdout);
    if (g_level >= 3)
        fprintf(stderr, "[ngs] derive instrument: %llu records (%llu without a name) in %llu batches, %llu instrument and %llu flowcell ids "
                        "(%llu strings appended, %llu candidates); ingest %.1f ms, kernel %.1f ms, total %.1f ms\n",
                (unsigned long long)rep.records, (unsigned long long)rep.skipped, (unsigned long long)rep.batches,
                (unsigned long long)rep.instruments, (unsigned long long)rep.flowcells, (unsigned long long)rep.entries,
                (unsigned long long)rep.candidates, rep.scan_ms, rep.kernel_ms, rep.total_ms);
    return 0;
}
