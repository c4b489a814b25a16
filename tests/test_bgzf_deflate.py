"""The parts of the device BGZF writer that need no GPU (include/ngsq_bgzf.h): the bound, the test model
itself against members built by hand, the command line's --gzip option, the Python prototypes."""
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from ngs_amd import build, ffi
from tests import bgzf_model as bm
from tests import generate_model as gm


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def run(ngs, *args):
    return subprocess.run([ngs, *args], capture_output=True, timeout=120)


def test_bound(lib):
    assert lib.ngsq_bgzf_deflate_bound(0, 0) == 0 and lib.ngsq_bgzf_deflate_bound(0, ffi.BGZF_EOF) == 28
    for n, blocks in ((1, 1), (65280, 1), (65281, 2), (2 * 65280, 2), (2 * 65280 + 1, 3), (10 ** 12, -(-10 ** 12 // 65280))):
        assert lib.ngsq_bgzf_deflate_bound(n, 0) == n + 31 * blocks          # every block stored: 18 + 5 + n + 8
        assert lib.ngsq_bgzf_deflate_bound(n, ffi.BGZF_EOF) == n + 31 * blocks + 28
    assert ffi.BGZF_BLOCK_INPUT == bm.BLOCK_INPUT == 65280 and 65280 + 31 <= 65536   # a stored block fits BSIZE
    assert ffi.BGZF_EOF_BLOCK == bm.EOF_BLOCK and gzip.decompress(bm.EOF_BLOCK) == b""


def test_model_on_members_built_by_hand():
    rng = np.random.default_rng(1)
    a, b = rng.integers(0, 256, 1000, dtype=np.uint8).tobytes(), b"ACGT" * 5000
    stream = bm.stored_member(a) + bm.member(b) + bm.EOF_BLOCK
    data, blocks = bm.walk(stream)
    assert data == a + b and gzip.decompress(stream) == a + b
    assert [(x.isize, x.eof) for x in blocks] == [(1000, False), (20000, False), (0, True)] and blocks[0].btype == 0
    assert blocks[0].size == 1000 + 31 and blocks[1].btype in (1, 2) and blocks[2].eof and blocks[1].offset == blocks[0].size
    assert bm.walk(bm.stored_member(a), require_eof=False)[0] == a
    refusals = {
        "no EOF block": bm.stored_member(a),
        "does not land": stream[:len(stream) - 40],                                                  # truncated inside the second member
        "truncated header": stream + b"\x1f\x8b\x08",
        "BSIZE": None,
        "CRC32 mismatch": bm.stored_member(a)[:-8] + struct.pack("<II", 1, 1000) + bm.EOF_BLOCK,
        "ISIZE": bm.stored_member(a)[:-4] + struct.pack("<I", 999) + bm.EOF_BLOCK,
        "bad magic": b"\x1f\x8c" + stream[2:],
        "FLG": stream[:3] + b"\x00" + stream[4:],
        "no BC subfield": stream[:12] + b"BD" + stream[14:],
    }
    m = bytearray(bm.member(b))
    struct.pack_into("<H", m, 16, len(m) - 3)                                                        # BSIZE two short: the trailer is cut
    refusals["BSIZE"] = bytes(m) + bm.EOF_BLOCK
    for want, s in refusals.items():
        with pytest.raises(bm.BgzfError) as e:
            bm.walk(s)
        if want != "BSIZE":
            assert want in str(e.value), (want, str(e.value))
    # a payload with bytes behind its end of block, and one that stops short of it
    raw = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = raw.compress(b) + raw.flush()
    for bad in (raw + b"\x00", raw[:-2]):
        with pytest.raises(bm.BgzfError):
            bm.walk(bm.member(b, bad) + bm.EOF_BLOCK)
    assert bm.zlib_size(b"x" * 70000, 6) == sum(len(bm.member(p)) for p in (b"x" * 65280, b"x" * 4720))


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bgzf") / "r.fa")
    open(path, "wb").write(gm.fasta_text([(b"chr1", gm.random_letters(np.random.default_rng(2), 401))], 60))
    return path


def test_gzip_option_messages(ngs, fasta, tmp_path):
    o1, o2, prov = str(tmp_path / "a_1.fastq"), str(tmp_path / "a_2.fq"), fasta + ":100:10:2:20:1"
    r = run(ngs, "generate", "-n", "5", "--gzip", "x", o1, o2, prov)
    assert r.returncode == 1 and b"Error: invalid value 'x' for '--gzip <WHERE>' [possible values: host, device]" in r.stderr
    assert not os.path.exists(o1) and not os.path.exists(o2)
    r = run(ngs, "generate", "-n", "5", o1, o2, prov, "--gzip")
    assert r.returncode == 1 and b"a value is required for '--gzip <WHERE>' but none was supplied" in r.stderr
    assert not os.path.exists(o1)
    r = run(ngs, "generate", "--help")
    h = (r.stderr + r.stdout).decode()
    assert r.returncode == 0 and "--gzip <WHERE>" in h and "[default: host] [possible values: host, device]" in h
    assert "additive" in h[h.index("--gzip <WHERE>"):]


@pytest.mark.parametrize("where", ["host", "device"])
def test_gzip_option_is_accepted_where_no_gpu_is_touched(ngs, fasta, tmp_path, where):
    """No pair, so no device: plain outputs are not affected by the flag; a gzipped one is an empty stream either way (one
    empty member from the host, the EOF block from the device path)."""
    o1, o2, prov = str(tmp_path / "z_1.fastq"), str(tmp_path / "z_2.fq"), fasta + ":100:10:2:20:1"
    r = run(ngs, "generate", "-n", "0", "--seed", "1", "--gzip", where, o1, o2, prov)
    assert r.returncode == 0, r.stderr
    assert open(o1, "rb").read() == b"" and open(o2, "rb").read() == b""
    g1, g2 = str(tmp_path / "g_1.fastq.gz"), str(tmp_path / "g_2.fq")
    r = run(ngs, "generate", "-n", "0", "--seed", "1", "--gzip", where, g1, g2, prov)
    assert r.returncode == 0, r.stderr
    z = open(g1, "rb").read()
    assert gzip.decompress(z) == b"" and len(z) > 0 and open(g2, "rb").read() == b""
    if where == "device":
        assert z == bm.EOF_BLOCK


def test_prototypes_resolve(lib):
    for name in ("ngsq_bgzf_deflate_bound", "ngsq_bgzf_deflate_device", "ngsq_generate_write_bgzf"):
        assert getattr(lib, name).argtypes is not None
    assert ffi.C.sizeof(ffi.BgzfDeflateReport) == 11 * 8 and ffi.C.sizeof(ffi.GenerateBgzfReport) == ffi.C.sizeof(ffi.GenerateReport) + 5 * 8
    # null and unknown arguments are refused before any device is looked for
    n = ffi.C.c_uint64(7)
    assert lib.ngsq_bgzf_deflate_device(None, b"abc", 3, None, 0, ffi.C.byref(n), 0, None) == ffi.ERR_INVALID_ARGUMENT
