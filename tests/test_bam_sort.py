"""`ngs convert --gzip device --sort coordinate <BAM> <BAM>` without a GPU: the test-side model
(tests/bam_sort_model.py) held to tests/golden/hand_spec.bam, to cases worked by hand and to tests/sort_model.py, and the
command line's surface and the refusals that come before any GPU work.

The tests named test_model_* run the model alone: they pin the yardstick the GPU tests (tests/test_bam_sort_gpu.py) hold the
library to and pass without the feature.  The command-line tests need it."""
import gzip
import os
import struct
import subprocess

import pytest

from ngs_amd import build
from tests import bam_sort_model as bsm
from tests import bam_text_model as tm
from tests import bamio
from tests import sort_model as som
from tests.test_sam_to_bam import HEAD, hand_spec_text, random_sam

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NOT_SUPPORTED = "Error: Conversion from BAM to BAM is not currently supported"


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def run(ngs, *args):
    return subprocess.run([ngs, *args], capture_output=True, text=True, timeout=120)


def rec(ref_id, pos, name=b"r", aux=b""):
    body = struct.pack("<iiBBHHHIiii", ref_id, pos, len(name) + 1, 0, 4680, 0, 4, 0, -1, -1, 0) + name + b"\0" + aux
    return struct.pack("<I", len(body)) + body


def stream(text: bytes, refs, recs, pad: int = 0) -> bytes:
    s = b"BAM\1" + struct.pack("<i", len(text) + pad) + text + b"\0" * pad + struct.pack("<i", len(refs))
    for n, l in refs:
        s += struct.pack("<i", len(n) + 1) + n + b"\0" + struct.pack("<i", l)
    return s + b"".join(recs)


REFS = [(b"chr1", 1000), (b"chr2", 500)]
TEXT = b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chr2\tLN:500\n"
TABLE = struct.pack("<i", 2) + struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", 1000) + struct.pack("<i", 5) + b"chr2\0" + struct.pack("<i", 500)


# ---- the model ---------------------------------------------------------------------------------------------------------------
def test_model_splits_a_stream_into_its_parts():
    recs = [rec(0, 5, b"a"), rec(1, 2, b"bb", b"XAAk"), rec(-1, -1, b"u")]
    assert bsm.split(stream(TEXT, REFS, recs)) == (TEXT, TABLE, recs)
    assert bsm.split(stream(b"", [], [])) == (b"", struct.pack("<i", 0), [])


def test_model_unplaced_last_in_input_order_and_ties():
    """Worked by hand: placed records by (refID, pos), equal keys in input order; behind them the records without a sequence or
    without a position, by pos + 1 and then input order (a refID with pos -1 counts as unplaced)."""
    names = [(b"u0", -1, -1), (b"c2p9", 1, 9), (b"c1p7", 0, 7), (b"nopos", 0, -1), (b"c1p7b", 0, 7), (b"u1", -1, -1), (b"c1p0", 0, 0),
             (b"u7", -1, 6), (b"c2p9b", 1, 9), (b"c1p7c", 0, 7)]
    recs = [rec(r, p, n) for n, r, p in names]
    out = bsm.split(bsm.stream_of(TEXT, TABLE, recs))[2]
    assert [x[36:x.index(b"\0", 36)] for x in out] == [b"c1p0", b"c1p7", b"c1p7b", b"c1p7c", b"c2p9", b"c2p9b", b"u0", b"nopos", b"u1", b"u7"]
    assert sorted(out) == sorted(recs)                                           # whole and unchanged


def test_model_header_cases():
    want_text = TEXT.replace(b"SO:unsorted", b"SO:coordinate")
    assert bsm.stream_of(TEXT, TABLE, []) == b"BAM\1" + struct.pack("<i", len(want_text)) + want_text + TABLE
    # no @HD line: one is put in front; NUL padding behind the text is no text
    sq = TEXT[TEXT.index(b"@SQ"):]
    assert bsm.bam_stream(tm.bam_file(stream(sq, REFS, [], pad=3))) == b"BAM\1" + struct.pack("<i", len(som.NEW_HD + sq)) + som.NEW_HD + sq + TABLE
    # no @SQ line in the text, but binary references: they stay, and the text gets its @HD line all the same
    s = bsm.bam_stream(tm.bam_file(stream(b"@CO\tno sequences here\n", REFS, [rec(1, 3), rec(0, 8)])))
    assert s == b"BAM\1" + struct.pack("<i", len(som.NEW_HD) + 22) + som.NEW_HD + b"@CO\tno sequences here\n" + TABLE + rec(0, 8) + rec(1, 3)
    # an empty text and no references
    assert bsm.bam_stream(tm.bam_file(stream(b"", [], []))) == b"BAM\1" + struct.pack("<i", len(som.NEW_HD)) + som.NEW_HD + struct.pack("<i", 0)
    # a reference table that is not what @SQ lines would give (another length, a name of another case) is copied as it is
    odd = [(b"CHR1", 77), (b"chr2", 500)]
    s = bsm.bam_stream(tm.bam_file(stream(TEXT, odd, [])))
    assert s.endswith(struct.pack("<i", 2) + struct.pack("<i", 5) + b"CHR1\0" + struct.pack("<i", 77) + struct.pack("<i", 5) + b"chr2\0" + struct.pack("<i", 500))


def test_model_on_the_hand_worked_file():
    raw = open(os.path.join(GOLDEN, "hand_spec.bam"), "rb").read()
    text, table, recs = bsm.split(gzip.decompress(raw))
    assert len(recs) >= 5 and sum(len(r) for r in recs) + 8 + len(text) + len(table) == len(gzip.decompress(raw))
    got_text, got_table, got = bsm.split(bsm.bam_stream(raw))
    assert got_text == som.sorted_header(text.rstrip(b"\0")) and b"SO:coordinate" in got_text.split(b"\n")[0] and got_table == table
    keys = [som.key(r) for r in got]
    assert keys == sorted(keys) and sorted(got) == sorted(recs)
    for a, b in zip(got, got[1:]):                                                # ties in input order
        if som.key(a) == som.key(b):
            assert recs.index(a) < recs.index(b)
    for n in (1, 3):
        assert bsm.split(bsm.bam_stream(raw, n))[2] == bsm.sorted_records(recs[:n])


def test_model_agrees_with_the_text_model(tmp_path):
    for sam in (hand_spec_text(), random_sam(91, 700, tmp_path), HEAD.encode(), b""):
        bam = tm.bam_file(tm.bam_stream(sam), 5000)
        assert bsm.bam_stream(bam) == som.bam_stream(sam)
        assert bsm.bam_stream(bam, 5) == som.bam_stream(sam, 5)


# ---- the command line ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_bam(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("b") / "in.bam")
    with open(path, "wb") as f:
        f.write(tm.bam_file(stream(TEXT, REFS, [rec(1, 3), rec(0, 8), rec(-1, -1)])))
    return path


def test_help_names_bam_to_bam(ngs):
    r = run(ngs, "convert", "--help")
    h = r.stderr + r.stdout
    assert r.returncode == 0
    for s in ("--sort <ORDER>", "[possible values: none, coordinate]", "--gzip <WHERE>", "[possible values: host, device]", "SAM to BAM",
              "-n, --num-records <USIZE>", "[default: balanced] [possible values: best, balanced, fastest]", "additive"):
        assert s in h, s
    assert "BAM to BAM" in h[h.index("--sort <ORDER>"):]


def test_without_both_flags_bam_to_bam_is_refused_as_before(ngs, small_bam, tmp_path):
    out = str(tmp_path / "o.bam")
    for args in ([], ["--sort", "coordinate"], ["--gzip", "device"], ["--sort", "none", "--gzip", "device"], ["--sort", "coordinate", "--gzip", "host"]):
        r = run(ngs, "convert", *args, small_bam, out)
        assert (r.returncode, r.stdout, r.stderr.strip()) == (1, "", NOT_SUPPORTED), args
        assert not os.path.exists(out)
    # flag values are validated first, as for every pair
    r = run(ngs, "convert", "--gzip", "device", "--sort", "queryname", small_bam, out)
    assert r.returncode == 1 and "invalid value 'queryname' for '--sort <ORDER>' [possible values: none, coordinate]" in r.stderr
    r = run(ngs, "convert", "--gzip", "gpu", "--sort", "coordinate", small_bam, out)
    assert r.returncode == 1 and "invalid value 'gpu' for '--gzip <WHERE>' [possible values: host, device]" in r.stderr


def test_the_output_must_be_another_file(ngs, small_bam, tmp_path):
    before = open(small_bam, "rb").read()
    link, sym = str(tmp_path / "hard.bam"), str(tmp_path / "sym.bam")
    os.link(small_bam, link)
    os.symlink(small_bam, sym)
    for to in (small_bam, link, sym, os.path.join(os.path.dirname(small_bam), ".", "in.bam")):
        r = run(ngs, "convert", "--gzip", "device", "--sort", "coordinate", small_bam, to)
        assert (r.returncode, r.stderr.strip()) == (1, f"Error: Conversion from BAM to BAM needs two files: {to} is the input"), to
        assert open(small_bam, "rb").read() == before                            # checked before <TO> is opened
    assert bamio.EOF_BLOCK in before


def test_refusals_of_the_files_come_before_any_gpu_work(ngs, small_bam, tmp_path):
    r = run(ngs, "convert", "--gzip", "device", "--sort", "coordinate", str(tmp_path / "missing.bam"), str(tmp_path / "o.bam"))
    assert r.returncode == 1 and "Error: opening BAM input file: " in r.stderr and "missing.bam" in r.stderr
    assert os.listdir(tmp_path) == []
    r = run(ngs, "convert", "--gzip", "device", "--sort", "coordinate", small_bam, str(tmp_path / "no_such_dir" / "o.bam"))
    assert (r.returncode, r.stderr.strip()) == (1, "Error: opening BAM output file: No such file or directory (os error 2)")
    assert os.listdir(tmp_path) == []
    # a <FROM> that is no BAM inside is the reader's refusal, and <TO> is not created
    bad = tmp_path / "text.bam"
    bad.write_bytes(b"not a BGZF file at all, only some text\n" * 4)
    r = run(ngs, "convert", "--gzip", "device", "--sort", "coordinate", str(bad), str(tmp_path / "o.bam"))
    assert r.returncode == 1 and "Error: opening BAM input file: " in r.stderr and sorted(os.listdir(tmp_path)) == ["text.bam"]
