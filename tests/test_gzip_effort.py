"""`--gzip-effort` of `ngs convert` and `ngs generate` without a GPU: the command line's surface and the
refusals that come before any file is opened; and the token inflater the GPU tests read the encoder's matches with
(tests/deflate_tokens.py), held to zlib.  What the efforts write is tested on the GPU (tests/test_gzip_effort_gpu.py)."""
import os
import subprocess
import zlib

import numpy as np
import pytest

from ngs_amd import build
from tests import bam_text_model as tm
from tests import deflate_tokens as dt
from tests.test_bam_sort import REFS, TEXT, rec, stream
from tests.test_sam_to_bam import HEAD

NEEDS = "Error: --gzip-effort needs --gzip device"


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def run(ngs, *args):
    return subprocess.run([ngs, *args], capture_output=True, text=True, timeout=120)


@pytest.fixture()
def files(tmp_path):
    bam, sam, fa = str(tmp_path / "in.bam"), str(tmp_path / "in.sam"), str(tmp_path / "ref.fa")
    with open(bam, "wb") as f:
        f.write(tm.bam_file(stream(TEXT, REFS, [rec(1, 3), rec(0, 8), rec(-1, -1)])))
    with open(sam, "w") as f:
        f.write(HEAD + "r\t0\tchr1\t5\t60\t4M\t=\t9\t0\tACGT\tIIII\n")
    with open(fa, "w") as f:
        f.write(">chr1\n" + "ACGTTGCA" * 500 + "\n")
    return bam, sam, fa


@pytest.mark.parametrize("command", ["convert", "generate"])
def test_help_names_the_flag_and_its_values(ngs, command):
    r = run(ngs, command, "--help")
    h = r.stderr + r.stdout
    assert r.returncode == 0
    assert "--gzip-effort <EFFORT>" in h
    after = h[h.index("--gzip-effort <EFFORT>"):]
    assert "[default: normal] [possible values: normal, high]" in after and "(additive, this build)" in after
    assert h.index("--gzip <WHERE>") < h.index("--gzip-effort <EFFORT>")       # beside --gzip
    assert "[possible values: host, device]" in h                              # whose lines stay
    if command == "convert":
        assert "-c is checked and takes no part" in h and "--gzip-effort" in h[h.index("-c is checked and takes no part"):]


@pytest.mark.parametrize("value", ["best", "HIGH", "2", ""])
def test_other_values_are_refused(ngs, files, tmp_path, value):
    bam, sam, fa = files
    before = sorted(os.listdir(tmp_path))
    want = f"Error: invalid value '{value}' for '--gzip-effort <EFFORT>' [possible values: normal, high]"
    r = run(ngs, "convert", "--gzip", "device", "--gzip-effort", value, sam, str(tmp_path / "o.bam"))
    assert (r.returncode, r.stdout, r.stderr.strip()) == (1, "", want)
    r = run(ngs, "generate", "--gzip", "device", "--gzip-effort", value, "-n", "5", str(tmp_path / "a.fastq.gz"), str(tmp_path / "b.fastq.gz"),
            fa + ":0.01:200:30:50:1")
    assert (r.returncode, r.stdout, r.stderr.strip()) == (1, "", want)
    assert sorted(os.listdir(tmp_path)) == before


@pytest.mark.parametrize("effort", ["normal", "high"])
def test_the_flag_needs_a_device_compressed_output(ngs, files, tmp_path, effort):
    bam, sam, fa = files
    before = sorted(os.listdir(tmp_path))
    cases = [("convert", [], bam, "o.sam"),                                      # BAM to SAM
             ("convert", ["--gzip", "device"], bam, "o.sam"),
             ("convert", [], sam, "o.bam"),                                      # SAM to BAM without --gzip device
             ("convert", ["--gzip", "host"], sam, "o.bam"),
             ("convert", ["--gzip", "host", "--sort", "coordinate"], bam, "o.bam"),
             ("convert", ["--gzip", "device"], bam, "o.bam")]                    # BAM to BAM is converted with --sort coordinate only
    for command, args, frm, to in cases:
        r = run(ngs, command, "--gzip-effort", effort, *args, frm, str(tmp_path / to))
        assert (r.returncode, r.stdout, r.stderr.strip()) == (1, "", NEEDS), (args, frm, to)
    provider = fa + ":0.01:200:30:50:1"
    for args, one, two in [([], "a.fastq.gz", "b.fastq.gz"),                     # generate with host gzip
                           (["--gzip", "host"], "a.fastq.gz", "b.fastq.gz"),
                           (["--gzip", "device"], "a.fastq", "b.fastq")]:        # no gzipped output at all
        r = run(ngs, "generate", "--gzip-effort", effort, *args, "-n", "5", "--seed", "1", str(tmp_path / one), str(tmp_path / two), provider)
        assert (r.returncode, r.stdout, r.stderr.strip()) == (1, "", NEEDS), (args, one, two)
    assert sorted(os.listdir(tmp_path)) == before


# ---- tests/deflate_tokens.py against zlib

def corpus():
    rng = np.random.default_rng(1)
    words = [b"read", b"chr1", b"ACGT", b"TTGACCA", b"\t", b"\n", b"IIIIHHHGG#", b"0123"]
    text = b"".join(words[k] for k in rng.integers(0, len(words), 4000))
    return [b"", b"a", b"abcabcabcabcabc", b"J" * 1000, text, rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(),
            text + rng.integers(0, 4, 5000, dtype=np.uint8).tobytes() + text]


@pytest.mark.parametrize("level, strategy", [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY),
                                             (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY)])
def test_the_token_inflater_reads_what_zlib_writes(level, strategy):
    for data in corpus():
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        raw = co.compress(data[:len(data) // 2]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(data[len(data) // 2:]) + co.flush()
        assert zlib.decompress(raw, -15) == data
        got, toks = dt.tokens(raw)
        assert got == data
        # the tokens cover the data, every match copies what lies `distance` back, and its bytes are the data's
        at = 0
        for t in toks:
            if isinstance(t, dt.Match):
                assert t.start == at and 3 <= t.length <= 258 and 1 <= t.distance <= min(32768, at)
                assert all(data[at + k] == data[at + k - t.distance] for k in range(t.length))
                at += t.length
            else:
                assert data[at] == t
                at += 1
        assert at == len(data)
        if strategy == zlib.Z_HUFFMAN_ONLY or level == 0:
            assert not dt.matches(toks)
    assert dt.matches(dt.tokens(zlib.compress(b"J" * 1000, 6)[2:-4])[1])


def test_the_token_inflater_refuses_a_distance_too_far_back():
    # a fixed block: literal 'a', then length 3 at distance 2 with one byte of history
    bits = [1, 1, 0]                                                   # BFINAL, BTYPE 1 (least significant bit first)
    bits += [int(b) for b in format(0x30 + ord("a"), "08b")]          # literal 'a': an 8-bit code, most significant bit first
    bits += [int(b) for b in format(1, "07b")]                         # length symbol 257 (3 bytes): the 7-bit code 0000001
    bits += [int(b) for b in format(1, "05b")]                         # distance symbol 1: distance 2
    bits += [0] * 7                                                    # end of block
    raw = bytes(sum(b << k for k, b in enumerate(bits[i:i + 8])) for i in range(0, len(bits), 8))
    with pytest.raises(zlib.error):
        zlib.decompress(raw, -15)
    with pytest.raises(ValueError, match="invalid distance too far back"):
        dt.tokens(raw)
