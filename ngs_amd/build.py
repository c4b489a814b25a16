"""Build ngs_amd/libngsq.so with hipcc for gfx950 (cross-compiles without a GPU).

    python -m ngs_amd.build [--force]
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libngsq.so")
SOURCES = ["kernels.hip", "qual_kernel.hip", "fields_kernel.hip", "cov_scan.hip", "cov_stream.hip", "synth.hip", "bgzf_inflate.hip", "bgzf_deflate.hip", "bgzf_deflate.cpp",
           "bam_device.hip", "features_kernel.hip", "edits_kernel.hip", "exchange_kernels.hip", "comm.cpp", "exchange.cpp", "mem_pool.cpp", "context.cpp", "stager.cpp", "results.cpp", "bam_reader.cpp", "bam_device_reader.cpp", "synth_bam.cpp",
           "reference.cpp", "reference_kernels.hip", "bai_kernel.hip", "bai.cpp",
           "sam_kernel.hip", "sam.cpp", "derive_kernel.hip", "derive.cpp",
           "view_kernel.hip", "view_query.cpp", "view.cpp",
           "generate_kernel.hip", "generate_args.cpp", "generate_gzip.cpp", "generate.cpp",
           "samtext_kernel.hip", "samtext.cpp",
           "sort_kernel.hip", "sort.cpp", "samsort.cpp", "samsort_header.cpp", "bamsort.cpp",
           "depth_kernel.hip", "depth.cpp", "depth_bed.cpp", "depth_windows_kernel.hip", "depth_windows.cpp",
           "fastq_kernel.hip", "fastq.cpp", "collate_kernel.hip", "collate.cpp",
           "markdup_kernel.hip", "markdup.cpp"]
HEADERS = ["kernels.h", "context.h", "comm.h", "mem_pool.h", "bam_reader.h", "ingest_consumer.h", "ingest_kernels.h", "bgzf.h", "bgzf_crc.h", "deflate_kernels.h", "../../include/ngsq_bgzf.h", "reference_kernels.h", "../../include/ngsq.h",
           "../../include/ngsq_reference.h", "../../include/ngsq_comm.h",
           "../../include/ngsq_shared.h", "../../include/ngsq_synth.h", "../../include/ngsq_bam.h", "../../include/ngsq_stage.h",
           "bai_kernels.h", "bai_host.h", "aux_cg.h", "../../include/ngsq_index.h", "sam_kernels.h", "../../include/ngsq_sam.h",
           "derive_kernels.h", "../../include/ngsq_derive.h",
           "device_out.h", "sam_run.h", "view_kernels.h", "view_query.h", "../../include/ngsq_view.h",
           "generate_kernels.h", "generate_draw.h", "reference_load.h", "../../include/ngsq_generate.h",
           "samtext_kernels.h", "samtext_host.h", "samtext_run.h", "../../include/ngsq_samtext.h",
           "sort_kernels.h", "../../include/ngsq_sort.h", "sort_resident.h", "../../include/ngsq_bamsort.h",
           "depth_kernels.h", "depth_run.h", "depth_windows_kernels.h", "../../include/ngsq_depth.h",
           "fastq_kernels.h", "fastq_format.h", "../../include/ngsq_fastq.h", "collate_kernels.h", "../../include/ngsq_collate.h",
           "name_key.h", "markdup_kernels.h", "../../include/ngsq_markdup.h"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-result", "-fno-gpu-rdc"]
FLAGS += os.environ.get("NGSQ_EXTRA_FLAGS", "").split()  # extra compiler flags for a local build, e.g. -save-temps (use --force)
OBJ_DIR = os.path.join(HERE, "_obj")  # per-source objects (git-ignored): only changed sources recompile


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found")


def up_to_date() -> bool:
    if not os.path.exists(OUT):
        return False
    t = os.path.getmtime(OUT)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return all(os.path.getmtime(d) <= t for d in deps)


CLI_DIR = os.path.join(CSRC, "cli")
CLI_SOURCES = [os.path.join(CLI_DIR, f) for f in ("ngs_main.cpp", "qc.cpp", "index.cpp", "convert.cpp", "derive.cpp", "view.cpp", "generate.cpp", "depth.cpp", "fastq.cpp", "markdup.cpp")]  # one file per command
CLI_HEADERS = sorted(os.path.join(CLI_DIR, f) for f in os.listdir(CLI_DIR) if f.endswith(".h"))
CLI_PUBLIC_HEADERS = [os.path.join(HERE, "..", "include", f) for f in (
    "ngsq.h", "ngsq_bam.h", "ngsq_bamsort.h", "ngsq_bgzf.h", "ngsq_collate.h", "ngsq_comm.h", "ngsq_depth.h", "ngsq_derive.h", "ngsq_fastq.h", "ngsq_generate.h", "ngsq_index.h", "ngsq_markdup.h", "ngsq_reference.h", "ngsq_sam.h", "ngsq_samtext.h", "ngsq_sort.h", "ngsq_stage.h", "ngsq_view.h")]
CLI_OUT = os.path.join(HERE, "ngs")


def build_cli(force: bool = False, verbose: bool = True) -> str:
    """The `ngs` command line (host C++ only), linked against libngsq.so next to it."""
    deps = CLI_SOURCES + CLI_HEADERS + CLI_PUBLIC_HEADERS + [OUT]
    if not force and os.path.exists(CLI_OUT) and all(os.path.getmtime(d) <= os.path.getmtime(CLI_OUT) for d in deps):
        return CLI_OUT
    cmd = ["g++", "-O2", "-std=c++17", "-Wall"] + CLI_SOURCES + ["-L" + HERE, "-lngsq", "-Wl,-rpath,$ORIGIN",
           "-Wl,-rpath-link," + "/opt/rocm/lib", "-lz", "-lpthread", "-o", CLI_OUT + ".tmp"]
    if verbose:
        print("[ngs_amd.build]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    os.replace(CLI_OUT + ".tmp", CLI_OUT)
    return CLI_OUT


def build(force: bool = False, verbose: bool = True) -> str:
    if not force and up_to_date():
        build_cli(False, verbose)
        return OUT
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(OBJ_DIR, exist_ok=True)
    hdr_t = max(os.path.getmtime(os.path.join(CSRC, h)) for h in HEADERS)
    hdr_t = max(hdr_t, os.path.getmtime(os.path.abspath(__file__)))
    cc = hipcc()

    def compile_one(src: str) -> str:
        obj = os.path.join(OBJ_DIR, src.replace("/", "_") + ".o")
        path = os.path.join(CSRC, src)
        if not force and os.path.exists(obj) and os.path.getmtime(obj) >= max(hdr_t, os.path.getmtime(path)):
            return obj
        cmd = [cc] + FLAGS + ["-c", path, "-o", obj]
        if verbose:
            print("[ngs_amd.build]", " ".join(cmd), flush=True)
        subprocess.run(cmd, check=True, cwd=CSRC)
        return obj

    with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    cmd = [cc, "--offload-arch=gfx950", "-fno-gpu-rdc", "-shared", "-fPIC"] + objs + ["-lz", "-lpthread", "-ldl", "-lrt", "-o", OUT + ".tmp"]
    if verbose:
        print("[ngs_amd.build]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, cwd=CSRC)
    os.replace(OUT + ".tmp", OUT)
    build_cli(True, verbose)
    return OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(OUT)
