// ngs_main.cpp -- the `ngs` command line over the MI355X hot path: global -q/-v and the dispatch (src/main.rs:19-105).
// The commands this build provides, one file each: `ngs qc` (qc.cpp), `ngs index` (index.cpp), `ngs convert`
// (convert.cpp), `ngs derive instrument` (derive.cpp), `ngs view` (view.cpp), `ngs generate` (generate.cpp), `ngs depth` (depth.cpp), `ngs fastq` (fastq.cpp), `ngs markdup` (markdup.cpp); what they share is in cli.h.  (NGSQ_RETURN_WHEN_DONE is explained in qc.cpp: fork_return_when_done.)
#include "cli.h"

int main(int argc, char **argv) {
    milestone("main");
    int k = 1;
    while (k < argc && verbosity_option(argv[k])) k++;
    if (k < argc && !strcmp(argv[k], "index")) return index_main(argc, argv, k);
    if (k < argc && !strcmp(argv[k], "convert")) return convert_main(argc, argv, k);
    if (k < argc && !strcmp(argv[k], "derive")) return derive_main(argc, argv, k);
    if (k < argc && !strcmp(argv[k], "view")) return view_main(argc, argv, k);
    if (k < argc && !strcmp(argv[k], "generate")) return generate_main(argc, argv, k);
    if (k < argc && !strcmp(argv[k], "depth")) return depth_main(argc, argv, k);
    if (k < argc && !strcmp(argv[k], "fastq")) return fastq_main(argc, argv, k);
    if (k < argc && !strcmp(argv[k], "markdup")) return markdup_main(argc, argv, k);
    return qc_main(argc, argv); // (takes "qc" wherever it stands among its arguments, and answers a command line without it)
}
