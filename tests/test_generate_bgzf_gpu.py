"""`ngs generate` writing BGZF on the device (include/ngsq_generate.h: ngsq_generate_write_bgzf; DESIGN.md sections 16 and 17):
the decompressed files are the plain path's and the model's, whatever the batch size; every file passes the BGZF model and ends
with the EOF block; the command line's --gzip device is the library call."""
import gzip
import os
import subprocess

import pytest

from ngs_amd import build, ffi, host
from tests import bgzf_model as bm
from tests import generate_model as gm
from tests.test_generate_gpu import base_fa, clean_fa, first_difference  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def bgzf_files(gpu_lib, specs, tmp_path, seed, n, first=0, batch=0, tag="z"):
    p1, p2 = str(tmp_path / f"{tag}_1.fastq.gz"), str(tmp_path / f"{tag}_2.fastq.gz")
    rep = host.generate(specs, p1, p2, seed, n, first_pair=first, batch_pairs=batch, lib=gpu_lib, bgzf=True)
    return open(p1, "rb").read(), open(p2, "rb").read(), rep


def plain_files(gpu_lib, specs, tmp_path, seed, n, first=0, tag="p"):
    p1, p2 = str(tmp_path / f"{tag}_1.fastq"), str(tmp_path / f"{tag}_2.fastq")
    host.generate(specs, p1, p2, seed, n, first_pair=first, lib=gpu_lib)
    return open(p1, "rb").read(), open(p2, "rb").read()


@pytest.mark.parametrize("L", [1, 64, 150])
def test_decompresses_to_the_plain_files_and_the_model(gpu_lib, base_fa, tmp_path, L):
    specs = [(base_fa, 50, 10.0, 2.0, L, 1)]
    n, first = 1200, 7
    z1, z2, rep = bgzf_files(gpu_lib, specs, tmp_path, 200 + L, n, first)
    one, two = plain_files(gpu_lib, specs, tmp_path, 200 + L, n, first)
    want = gm.generate([gm.model_provider(s, gpu_lib) for s in specs], 200 + L, first, n)
    for z, plain, model in ((z1, one, want.one), (z2, two, want.two)):
        data, blocks = bm.walk(z)
        assert data == plain, first_difference(data, plain)
        assert data == model and gzip.decompress(z) == plain
        assert blocks[-1].eof and z.endswith(bm.EOF_BLOCK) and len(z) < len(plain)
        assert all(b.isize == bm.BLOCK_INPUT for b in blocks[:-2])
    assert rep["pairs"] == n and rep["text_bytes_one"] == len(one) and rep["text_bytes_two"] == len(two)
    assert rep["compressed_bytes_one"] == len(z1) and rep["compressed_bytes_two"] == len(z2)
    assert rep["blocks"] == len(bm.walk(z1)[1]) + len(bm.walk(z2)[1]) - 2 and rep["deflate_ms"] > 0


def test_pair_counts_and_batches(gpu_lib, base_fa, tmp_path):
    specs = [(base_fa, 50, 30.0, 5.0, 150, 1)]
    # no pair: the EOF block alone
    z1, z2, rep = bgzf_files(gpu_lib, specs, tmp_path, 5, 0, tag="e")
    assert z1 == bm.EOF_BLOCK and z2 == bm.EOF_BLOCK and gzip.decompress(z1) == b"" and rep["pairs"] == 0
    assert rep["compressed_bytes_one"] == 28 and rep["compressed_bytes_two"] == 28
    z1, z2, rep = bgzf_files(gpu_lib, specs, tmp_path, 5, 1, tag="s")
    one, two = plain_files(gpu_lib, specs, tmp_path, 5, 1, tag="s")
    assert bm.walk(z1)[0] == one and bm.walk(z2)[0] == two and len(bm.walk(z1)[1]) == 2
    # three batches, each of more than one block: the short last block of a batch is followed by more blocks
    n, batch = 1000, 400
    one, two = plain_files(gpu_lib, specs, tmp_path, 6, n, tag="b")
    assert len(one) > 3 * bm.BLOCK_INPUT
    sizes = {}
    for bp in (batch, 0, 333):
        z1, z2, rep = bgzf_files(gpu_lib, specs, tmp_path, 6, n, batch=bp, tag=f"b{bp}")
        d1, b1 = bm.walk(z1)
        d2, _ = bm.walk(z2)
        assert d1 == one and d2 == two                               # the decompressed bytes do not depend on batch_pairs
        assert rep["batches"] == (-(-n // bp) if bp else 1)
        sizes[bp] = [b.isize for b in b1]
    short = [k for k, s in enumerate(sizes[batch][:-1]) if s < bm.BLOCK_INPUT]
    assert len(short) == 3 and short[-1] == len(sizes[batch]) - 2 and short[0] + 1 < len(sizes[batch]) - 2
    assert sum(s < bm.BLOCK_INPUT for s in sizes[0][:-1]) == 1


def test_command_line_is_the_library_call(gpu_lib, base_fa, clean_fa, tmp_path):
    ngs = build.build_cli(verbose=False)
    specs = [(base_fa, 40, 12.0, 3.0, 90, 2), (clean_fa, 60, -10.0, 0.0, 33, 1)]
    strings = [f"{base_fa}:40:12:3:90:2", f"{clean_fa}:60:-10:0:33:1"]
    z1, z2, _ = bgzf_files(gpu_lib, specs, tmp_path, 16, 700, batch=256)
    c1, c2 = str(tmp_path / "c_1.fastq.gz"), str(tmp_path / "c_2.fq.gz")
    r = subprocess.run([ngs, "-q", "generate", "-n", "700", "--seed", "16", "--batch-pairs", "256", "--gzip", "device", c1, c2, *strings],
                       capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert open(c1, "rb").read() == z1 and open(c2, "rb").read() == z2
    h1, h2 = str(tmp_path / "h_1.fastq.gz"), str(tmp_path / "h_2.fq.gz")
    r = subprocess.run([ngs, "-q", "generate", "-n", "700", "--seed", "16", "--gzip", "host", h1, h2, *strings], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert gzip.decompress(open(h1, "rb").read()) == gzip.decompress(z1) and gzip.decompress(open(h2, "rb").read()) == gzip.decompress(z2)
    # one plain, one gzipped: the plain file is what it is without the flag
    m1, m2 = str(tmp_path / "m_1.fastq"), str(tmp_path / "m_2.fq.gz")
    r = subprocess.run([ngs, "-q", "generate", "-n", "700", "--seed", "16", "--batch-pairs", "256", "--gzip", "device", m1, m2, *strings],
                       capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(m1, "rb").read() == gzip.decompress(z1) and open(m2, "rb").read() == z2
    with host.Generator(specs, lib=gpu_lib) as g:
        fd1, fd2 = os.open(str(tmp_path / "l_1"), os.O_WRONLY | os.O_CREAT, 0o666), os.open(str(tmp_path / "l_2"), os.O_WRONLY | os.O_CREAT, 0o666)
        try:
            g.write_fds(fd1, fd2, 16, 700, batch_pairs=256, bgzf=True, plain=ffi.GENERATE_PLAIN_TWO)
        finally:
            os.close(fd1)
            os.close(fd2)
    assert open(str(tmp_path / "l_1"), "rb").read() == z1 and open(str(tmp_path / "l_2"), "rb").read() == gzip.decompress(z2)


def test_a_full_device_ends_with_the_write_message(gpu_lib, base_fa, tmp_path):
    ngs = build.build_cli(verbose=False)
    full = str(tmp_path / "full_1.fastq.gz")
    os.symlink("/dev/full", full)
    r = subprocess.run([ngs, "generate", "-n", "300", "--seed", "2", "--gzip", "device", full, str(tmp_path / "ok_2.fastq.gz"),
                        f"{base_fa}:50:10:2:100:1"], capture_output=True, timeout=120)
    assert r.returncode == 1
    assert b"Error: could not write record to read one file: No space left on device (os error 28)" in r.stderr
