"""`ngs derive instrument` without a GPU: the library's restatement of the two pattern tables held to
the recorded results of tests/golden/instrument_cases.json, the predictor on every outcome of the reference's resolve logic,
the exact document text, the test-side model (tests/derive_model.py), and the command line's surface and refusals, which
all come before any GPU work."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from ngs_amd import build, ffi, host
from tests import bamio
from tests import derive_model as dm
from tests.util import random_batch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["chr1", "chr2", "chr3"]
LENS = [300_000, 70_000, 5_000]


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def run(ngs, *args, cwd=None):
    return subprocess.run([ngs, *args], capture_output=True, text=True, timeout=120, cwd=cwd)


@pytest.mark.parametrize("which,table", [(ffi.DERIVE_INSTRUMENTS, "instruments"), (ffi.DERIVE_FLOWCELLS, "flowcells")])
def test_lookup_equals_every_recorded_case(lib, which, table):
    cases = json.load(open(os.path.join(GOLDEN, "instrument_cases.json")))["cases"][table]
    assert len(cases) > 1000 and sum(1 for _, m in cases if m) > 50
    wrong = [(q, m, got) for q, m in cases for got in [host.derive_lookup(which, q.encode(), lib)] if got != m]
    assert not wrong, wrong[:10]


def test_lookup_of_bytes_that_are_no_text(lib):
    """Bytes are not validated: a query with a NUL or a high byte is looked up as it is, and only a prefix pattern takes it."""
    assert host.derive_lookup(ffi.DERIVE_INSTRUMENTS, b"A0000\x000", lib) == []
    assert host.derive_lookup(ffi.DERIVE_INSTRUMENTS, b"A00000\x00", lib) == []
    assert host.derive_lookup(ffi.DERIVE_INSTRUMENTS, b"HWUSI\x00\xff", lib) == ["Genome Analyzer IIx"]
    assert host.derive_lookup(ffi.DERIVE_FLOWCELLS, b"H\xc30000RXX", lib) == []
    assert host.derive_lookup(ffi.DERIVE_INSTRUMENTS, b"", lib) == [] and host.derive_lookup(ffi.DERIVE_FLOWCELLS, b"", lib) == []


def result(succeeded, instruments, confidence, evidence, comment):
    return {"succeeded": succeeded, "instruments": instruments, "confidence": confidence, "evidence": evidence, "comment": comment}


MULTI_IID = "multiple instruments were detected in this file via the instrument id"
MULTI_FCID = "multiple instruments were detected in this file via the flowcell id"
TRIAGE = "Case needs triaging, results from instrument id and flowcell id are mutually exclusive."
BOTH = "instrument and flowcell id"
# (instrument ids, flowcell ids, the result): every outcome of resolve_instrument_prediction (compute.rs:157-267), the inputs
# of the reference's own unit tests (compute.rs:319-473) among them
PREDICTIONS = [
    ([b"A00000"], [b"H00000RXX"], result(True, ["NovaSeq"], "high", BOTH, None)),
    ([b"A00000", b"D00000"], [b"H00000RXX"], result(False, None, "unknown", "instrument id", MULTI_IID)),
    ([b"A00000"], [b"H00000RXX", b"B0000"], result(False, None, "unknown", "flowcell id", MULTI_FCID)),
    ([b"A00000"], [], result(True, ["NovaSeq"], "medium", "instrument id", None)),
    ([b"K00000"], [], result(True, ["HiSeq 3000", "HiSeq 4000"], "low", "instrument id", None)),
    ([], [b"H00000RXX"], result(True, ["NovaSeq"], "medium", "flowcell id", None)),
    ([], [b"H0000ADXX"], result(True, ["HiSeq 1500", "HiSeq 2000", "HiSeq 2500"], "low", "flowcell id", None)),
    ([b"K00000"], [b"H00000RXX"], result(False, None, "high", BOTH, TRIAGE)),
    ([b"QQQQQ"], [b"ZZZZZZ"], result(False, None, "unknown", None, "no matching instruments were found")),
    ([], [], result(False, None, "unknown", None, "no matching instruments were found")),
    # a name that matches no pattern contributes an empty set: beside a known one it reads as a conflict
    ([b"A00000", b"QQQQQ"], [b"H00000RXX"], result(False, None, "unknown", "instrument id", MULTI_IID)),
    ([b"A00000"], [b"ZZZZZZ", b"H00000RXX"], result(False, None, "unknown", "flowcell id", MULTI_FCID)),
    # an unknown instrument alone leaves the flowcell to decide; the instrument conflict is reported in front of the flowcell's
    ([b"QQQQQ"], [b"H00000RXX"], result(True, ["NovaSeq"], "medium", "flowcell id", None)),
    ([b"A00000", b"D00000"], [b"H00000RXX", b"B0000"], result(False, None, "unknown", "instrument id", MULTI_IID)),
    # intersections: HiSeq 2000 | 2500 with HiSeq 2500; three flowcell machines with one instrument machine
    ([b"HWI-D00000", b"D00000"], [], result(True, ["HiSeq 2500"], "medium", "instrument id", None)),
    ([b"HWI-D00000"], [b"H0000ADXX"], result(True, ["HiSeq 2000", "HiSeq 2500"], "high", BOTH, None)),
    ([b"", b"A00000"], [b""], result(False, None, "unknown", "instrument id", MULTI_IID)),
    # a string given twice counts once
    ([b"A00000", b"A00000"], [b"H00000RXX", b"H00000RXX"], result(True, ["NovaSeq"], "high", BOTH, None)),
]


@pytest.mark.parametrize("k", range(len(PREDICTIONS)))
def test_predict(lib, k):
    ins, fcs, want = PREDICTIONS[k]
    text = host.derive_predict(ins, fcs, lib)
    assert json.loads(text) == want
    assert list(json.loads(text)) == ["succeeded", "instruments", "confidence", "evidence", "comment"]
    assert text == json.dumps(want, indent=2)
    assert dm.predict(ins, fcs) == want      # the model says the same (its machines come from the fixture)


def test_document_text(lib):
    assert host.derive_predict([b"A00741"], [b"HG7WKDSXX"], lib) == (
        '{\n  "succeeded": true,\n  "instruments": [\n    "NovaSeq"\n  ],\n  "confidence": "high",\n'
        '  "evidence": "instrument and flowcell id",\n  "comment": null\n}')
    assert host.derive_predict([b"K00000"], [], lib) == (
        '{\n  "succeeded": true,\n  "instruments": [\n    "HiSeq 3000",\n    "HiSeq 4000"\n  ],\n  "confidence": "low",\n'
        '  "evidence": "instrument id",\n  "comment": null\n}')
    assert host.derive_predict([b"QQQQQ"], [b"ZZZZZZ"], lib) == (
        '{\n  "succeeded": false,\n  "instruments": null,\n  "confidence": "unknown",\n  "evidence": null,\n'
        '  "comment": "no matching instruments were found"\n}')


def test_buffers_that_are_too_small(lib):
    q = (C.c_char_p * 1)(b"A00000")
    n = (C.c_uint32 * 1)(6)
    need = C.c_size_t()
    assert lib.ngsq_derive_predict(q, n, 1, None, None, 0, None, 0, C.byref(need)) == ffi.ERR_BUFFER_TOO_SMALL
    want = host.derive_predict([b"A00000"], [], lib)
    assert need.value == len(want) + 1
    buf = C.create_string_buffer(b"\x7f" * need.value, need.value)
    assert lib.ngsq_derive_predict(q, n, 1, None, None, 0, buf, need.value - 1, C.byref(need)) == ffi.ERR_BUFFER_TOO_SMALL
    assert buf.raw == b"\x7f" * need.value                                    # nothing was written
    assert lib.ngsq_derive_predict(q, n, 1, None, None, 0, buf, need.value, None) == ffi.OK
    assert buf.value.decode() == want
    assert lib.ngsq_derive_lookup(ffi.DERIVE_INSTRUMENTS, b"K00000", 6, None, 0, C.byref(need)) == ffi.ERR_BUFFER_TOO_SMALL
    assert need.value == len("HiSeq 3000\nHiSeq 4000\n") + 1
    assert lib.ngsq_derive_lookup(ffi.DERIVE_INSTRUMENTS, b"K00000", 6, buf, need.value - 1, None) == ffi.ERR_BUFFER_TOO_SMALL
    assert lib.ngsq_derive_lookup(2, b"K00000", 6, buf, need.value, None) == ffi.ERR_INVALID_ARGUMENT
    assert lib.ngsq_derive_predict(None, None, 1, None, None, 0, buf, 8, None) == ffi.ERR_INVALID_ARGUMENT


def test_names_of_no_scan(lib):
    assert lib.ngsq_derive_names_count(None, 0) == 0 and lib.ngsq_derive_names_get(None, 0, 0, None) is None
    lib.ngsq_derive_names_free(None)


# ---- the model ---------------------------------------------------------------------------------------------------------
def test_model_splits_names():
    assert dm.split(b"A00741:215:HG7WKDSXX:1:1101:1000:2000") == (b"A00741", b"HG7WKDSXX")
    assert dm.split(b"HWI-ST123:1:1101:1000:2000") == (b"HWI-ST123", None)
    assert dm.split(b"::::") == (b"", None) and dm.split(b"::::::") == (b"", b"")
    for bad in (b"r1", b"", b"a:b:c:d:e:f", b"a:b:c:d:e:f:g:h", b"a:b:c:d"):
        with pytest.raises(dm.BadName):
            dm.split(bad)
    names = [b"*", b"A00000:1:2:3:4", b"A00000:1:H00000RXX:3:4:5:6", b"*", b"bad"]
    assert dm.collect(names[:4]) == ({b"A00000"}, {b"H00000RXX"}, 2)
    with pytest.raises(dm.BadName) as e:
        dm.collect(names)
    assert e.value.name == b"bad" and str(e.value) == "Could not parse Illumina-formatted query names for read: bad"
    assert list(dm.examined(names, 0)) == names and list(dm.examined(names, 1)) == names[:2]
    assert list(dm.examined(names, 3)) == names[:4] and list(dm.examined(names, 4)) == names and list(dm.examined(names, 99)) == names


def test_model_reads_the_names_of_a_file(tmp_path):
    rng = np.random.default_rng(3)
    hb = random_batch(rng, 500, LENS, max_len=60)
    names = [bamio.aligner_name(rng) if k % 7 else (b"*", b"::::", b"x" * 254)[k % 3] for k in range(hb.n)]
    path = str(tmp_path / "n.bam")
    bamio.write_bam(path, hb, NAMES, LENS, block_payload=3000, names=names)
    assert dm.read_names(path) == names
    ins, fcs, skipped, res = dm.expected(path, n=5)
    assert (ins, fcs, skipped) == ([b"A00741"], [b"HG7WKDSXX"], 1) and res == result(True, ["NovaSeq"], "high", BOTH, None)
    with pytest.raises(dm.BadName):
        dm.expected(path)
    sam = open(os.path.join(GOLDEN, "hand_spec.sam"), "rb").read().split(b"\n")[:-1]
    assert dm.read_names(os.path.join(GOLDEN, "hand_spec.bam")) == [x.split(b"\t")[0] for x in sam if not x.startswith(b"@")]


# ---- the command line, as far as it goes without a GPU --------------------------------------------------------------------
def test_cli_help(ngs):
    r = run(ngs, "derive", "instrument", "--help")
    assert r.returncode == 0 and r.stdout == ""
    for word in ("Usage: ngs derive instrument", "<BAM>", "-n, --num-records <USIZE>", "-t, --threads <USIZE>", "--device <N>"):
        assert word in r.stderr
    assert run(ngs, "derive", "-h").returncode == 0


def test_cli_refusals(ngs, tmp_path):
    def refused(*args):
        r = run(ngs, *args, cwd=str(tmp_path))
        assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("Error: "), (args, r)
        return r.stderr[len("Error: "):].rstrip("\n")

    assert "`ngs derive instrument`" in refused("derive")
    assert "unrecognized subcommand 'flowcell'" in refused("derive", "flowcell", "x.bam")
    assert refused("derive", "instrument") == "the following required arguments were not provided: <BAM>"
    assert refused("derive", "instrument", "a.bam", "b.bam") == "unexpected argument 'b.bam' found"
    assert refused("derive", "instrument", "--frobnicate", "a.bam") == "unexpected argument '--frobnicate' found"
    assert refused("derive", "instrument", "a.bam", "-n") == "a value is required for '--num-records <USIZE>' but none was supplied"
    assert refused("derive", "instrument", "a.bam", "-n", "x") == "invalid value 'x' for '--num-records <USIZE>': invalid digit found in string"
    assert refused("derive", "instrument", "a.bam", "-t", "-1") == "invalid value '-1' for '--threads <USIZE>': invalid digit found in string"
    assert refused("derive", "instrument", "reads.sam") == "incompatible formats: required BAM, found SAM"
    assert refused("-q", "derive", "instrument", "reads.cram", "-n", "5") == "incompatible formats: required BAM, found CRAM"
    assert refused("derive", "instrument", "reads.xyz") == "Not able to determine filetype for extension: xyz"
    assert "missing.bam" in refused("derive", "instrument", "missing.bam")


def test_cli_requires_the_index_before_any_gpu_work(ngs, lib, tmp_path):
    rng = np.random.default_rng(4)
    hb = random_batch(rng, 50, LENS, max_len=60)
    path = str(tmp_path / "noindex.bam")
    bamio.write_bam(path, hb, NAMES, LENS, with_index=False, names=[bamio.aligner_name(rng) for _ in range(hb.n)])
    r = run(ngs, "derive", "instrument", "-t", "4", path)
    assert r.returncode == 1 and r.stdout == ""
    assert lib.ngsq_bam_check_index(path.encode()) != ffi.OK
    assert r.stderr == "Error: " + lib.ngsq_bam_last_error().decode() + "\n" and "reading BAM index" in r.stderr
    with open(path + ".bai", "wb") as f:
        f.write(b"BAI\2garbage")
    r = run(ngs, "derive", "instrument", path)
    assert r.returncode == 1 and r.stdout == "" and "reading BAM index" in r.stderr
