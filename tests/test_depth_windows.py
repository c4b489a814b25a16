"""Mean depth per window or BED interval without a GPU: the test-side model (tests/depth_windows_model.py)
on a case worked by hand; its rounding rule against fractions.Fraction; its window sums against the per-base model's runs; its
regions; and the library's BED reader, ngsq_depth_read_bed, held to the model on every refusal and on an accepted file."""
from fractions import Fraction

import pytest

from ngs_amd import ffi, host
from tests import bamio
from tests import depth_model as dm
from tests import depth_windows_model as wm
from tests import test_depth as td
from tests.test_depth import rec, write_case


# ---- the model ----------------------------------------------------------------------------------------------------------------
def test_model_on_a_case_worked_by_hand(tmp_path):
    """a (10 positions): 3M at 2 covers 2..4, 2M1D1M at 3 covers 3..6, 5M at 8 is clipped to 8..9:
           position 0 1 2 3 4 5 6 7 8 9
           depth    0 0 1 2 2 1 1 0 1 1
       windows of 4: [0,4) sum 3 -> 0.75; [4,8) sum 4 -> 1.00; [8,10) sum 2 -> 1.00.
       b (5 positions): no record: [0,4) and [4,5) with 0.00.
       BED, in this order: b 1 3; a 3 9 (sum 2+2+1+1+0+1 = 7, 7/6 = 1.1666 -> 1.17); a 0 3 (sum 1, 1/3 -> 0.33); a 2 7 (sum 7,
       7/5 = 1.40): the lines come in header order, a's in the file's order.
       Region a:4-9 is [3, 9): the windows stay aligned to 0: [3,4) sum 2 -> 2.00; [4,8) -> 1.00; [8,9) sum 1 -> 1.00."""
    path = write_case(str(tmp_path / "h.bam"), ["a", "b"], [10, 5], [rec(0, 2, "3M"), rec(0, 3, "2M1D1M"), rec(0, 8, "5M")])
    got, info = wm.expected(path, window=4)
    assert got == b"a\t0\t4\t0.75\na\t4\t8\t1.00\na\t8\t10\t1.00\nb\t0\t4\t0.00\nb\t4\t5\t0.00\n"
    assert info == dict(records_scanned=3, records_counted=3, lines=5, sequences=2, depth_sum=9)
    iv = wm.read_bed(b"b\t1\t3\na\t3\t9\na\t0\t3\na\t2\t7\n", [b"a", b"b"], [10, 5])
    assert iv == [(1, 1, 3), (0, 3, 9), (0, 0, 3), (0, 2, 7)]
    got, info = wm.expected(path, intervals=iv)
    assert got == b"a\t3\t9\t1.17\na\t0\t3\t0.33\na\t2\t7\t1.40\nb\t1\t3\t0.00\n"
    assert info == dict(records_scanned=3, records_counted=3, lines=4, sequences=2, depth_sum=15)
    got, info = wm.expected(path, window=4, query="a:4-9")
    assert got == b"a\t3\t4\t2.00\na\t4\t8\t1.00\na\t8\t9\t1.00\n" and info["lines"] == 3 and info["depth_sum"] == 7
    assert wm.expected(path, window=4, query="a:11")[0] == b"" and wm.expected(path, window=100, query="b")[0] == b"b\t0\t5\t0.00\n"
    assert wm.expected(path, intervals=[])[0] == b""


def test_rounding_rule_against_fractions():
    """Every (sum, len) with len <= 64 and sum <= 4 len: the text equals the fraction rounded half up to hundredths."""
    for length in range(1, 65):
        for total in range(0, 4 * length + 1):
            hundredths = (Fraction(total, length) * 100 + Fraction(1, 2)).__floor__()
            assert wm.mean_text(total, length) == b"%d.%02d" % divmod(hundredths, 100), (total, length)
    assert wm.mean_text(1, 200) == b"0.01"
    assert wm.mean_text(199, 200) == b"1.00"
    assert wm.mean_text(1, 201) == b"0.00"
    assert wm.mean_text(2 ** 62, 1) == b"4611686018427387904.00"
    assert wm.mean_text(1999, 200) == b"10.00" and wm.mean_text(19999, 200) == b"100.00" and wm.mean_text(0, 7) == b"0.00"


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_window_sums_add_up_to_the_per_base_models_runs(tmp_path, seed):
    """The sum of all window sums equals the sum of depth times run length of the per-base model, for several window sizes."""
    names, lens, hb = td.case_random(seed)
    path = str(tmp_path / "r.bam")
    bamio.write_bam(path, hb, names, lens, with_index=False)
    text, _ = dm.expected(path)
    want = 0
    for ln in text.splitlines():
        _, s, e, d = ln.split(b"\t")
        want += (int(e) - int(s)) * int(d)
    assert want > 0
    for n in (1, 7, 1000, 10 ** 6):
        got, info = wm.expected(path, window=n)
        assert info["depth_sum"] == want and info["lines"] == sum(-(-L // n) for L in lens) == got.count(b"\n")


def test_model_on_regions(tmp_path):
    names, lens, recs = td.case_query()
    path = write_case(str(tmp_path / "q.bam"), names, lens, recs, block_payload=3000)
    assert wm.expected(path, window=100_000, query="q1:4500-5500")[0] == b"q1\t4499\t5500\t1.00\n"     # begins and ends inside one window
    assert wm.expected(path, window=1000, query="q1:4500-5500")[0] == b"q1\t4499\t5000\t1.00\nq1\t5000\t5500\t1.00\n"
    assert wm.expected(path, window=1000, query="q1:300001")[0] == b""
    assert wm.expected(path, window=37, query="q2:100-200")[0].startswith(b"q2\t99\t111\t0.00\nq2\t111\t148\t0.00\n")


# ---- the BED reader -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("by")
    names, lens, recs = td.case_query()
    good = write_case(str(d / "good.bam"), names, lens, recs[:50])
    return dict(d=str(d), good=good, names=[n.encode() for n in names], lens=lens)


BED_REFUSALS = [
    (b"q1\t5\t9\nq1\t7\n", "reading BED file: line 2: expected at least 3 tab-separated fields, found 2"),
    (b"q1 5 9\n", "reading BED file: line 1: expected at least 3 tab-separated fields, found 1"),
    (b"# c\n\nq1\tx\t9\n", "reading BED file: line 3: invalid start 'x': expected a decimal number of at most 2147483647"),
    (b"q1\t+5\t9\n", "reading BED file: line 1: invalid start '+5'"),
    (b"q1\t-1\t9\n", "reading BED file: line 1: invalid start '-1'"),
    (b"q1\t\t9\n", "reading BED file: line 1: invalid start ''"),
    (b"q1\t5\t9.0\n", "reading BED file: line 1: invalid end '9.0'"),
    (b"q1\t5\t2147483648\n", "reading BED file: line 1: invalid end '2147483648': expected a decimal number of at most 2147483647"),
    (b"q1\t99999999999999999999999\t9\n", "reading BED file: line 1: invalid start '99999999999999999999999'"),
    (b"q1\t5\t9\nq1\t9\t9\n", "reading BED file: line 2: start 9 is not below end 9"),
    (b"q1\t10\t9\n", "reading BED file: line 1: start 10 is not below end 9"),
    (b"track name=x\nq3\t5000\t5001\n", "reading BED file: line 2: start 5000 lies at or beyond the end of 'q3' (5000 positions)"),
    (b"q1\t1\t2\r\nchrZ\t1\t2\r\n", "reading BED file: line 2: sequence 'chrZ' is not in the header"),
    (b"q1\t1\t2\nq1 \t1\t2", "reading BED file: line 2: sequence 'q1 ' is not in the header"),
]


def read_bed_through_the_library(lib, bam_path, bed_path):
    try:
        return host.depth_read_bed(bam_path, bed_path, lib=lib), None
    except host.NgsqError as e:
        return None, e


def test_every_bed_refusal_names_its_line(lib, files, tmp_path):
    for k, (data, msg) in enumerate(BED_REFUSALS):
        p = str(tmp_path / ("bad%d.bed" % k))
        open(p, "wb").write(data)
        with pytest.raises(wm.BedError) as want:
            wm.read_bed(data, files["names"], files["lens"])
        assert msg in str(want.value), data
        got, err = read_bed_through_the_library(lib, files["good"], p)
        assert got is None and err.code == ffi.ERR_INVALID_ARGUMENT and err.message == str(want.value), (data, err.message)
    got, err = read_bed_through_the_library(lib, files["good"], str(tmp_path / "missing.bed"))
    assert got is None and err.message == "opening BED file: No such file or directory (os error 2)"


def test_an_accepted_bed_file(lib, files, tmp_path):
    """\\r\\n line ends, comments, track and browser lines, empty lines, extra columns, a clipped end, a last line without \\n."""
    data = (b"browser position q1:1-100\r\ntrack name=\"t\"\r\n# comment\tq1\t1\t2\r\n\r\n\nq3\t4990\t6000\tname\t0\t+\r\nq1\t0\t1\n"
            b"q2\t69999\t2147483647\textra\nq1\t007\t010\nq3\t0\t5000")
    want = [(2, 4990, 5000), (0, 0, 1), (1, 69999, 70000), (0, 7, 10), (2, 0, 5000)]
    assert wm.read_bed(data, files["names"], files["lens"]) == want
    p = str(tmp_path / "ok.bed")
    open(p, "wb").write(data)
    assert host.depth_read_bed(files["good"], p, lib=lib) == want
    for empty in (b"", b"\n\n", b"# nothing\ntrack\n"):
        open(p, "wb").write(empty)
        assert host.depth_read_bed(files["good"], p, lib=lib) == [] == wm.read_bed(empty, files["names"], files["lens"])


def test_overlapping_and_unsorted_intervals_keep_the_files_order(lib, files, tmp_path):
    """Identical, nested, overlapping, touching and descending intervals, and sequences named backwards: read as they stand."""
    iv = [(2, 10, 20), (0, 100, 200), (0, 100, 200), (0, 120, 150), (0, 150, 260), (0, 260, 300), (0, 50, 60), (0, 0, 1), (1, 5, 6), (0, 299_999, 300_000)]
    data = b"".join(b"%s\t%d\t%d\n" % (files["names"][r], s, e) for r, s, e in iv)
    p = str(tmp_path / "o.bed")
    open(p, "wb").write(data)
    assert host.depth_read_bed(files["good"], p, lib=lib) == iv == wm.read_bed(data, files["names"], files["lens"])
    # the reader is called with bad arguments
    C = ffi.C
    n, out = C.c_uint64(), C.POINTER(ffi.DepthInterval)()
    assert lib.ngsq_depth_read_bed(None, p.encode(), C.byref(out), C.byref(n)) == ffi.ERR_INVALID_ARGUMENT
    lib.ngsq_depth_free_intervals(None)
