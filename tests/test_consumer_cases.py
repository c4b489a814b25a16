"""The files of the consumers sweep (tools/fuzz_parity.py --consumers) without a GPU: the test-side models
alone hold what the sweep relies on for its first eight seeds, the slice tests/test_fuzz_gpu.py runs -- files of several ingest
chunks, the planted record where the seed says and nowhere else, an empty member right behind a record's last byte, a record
longer than a BGZF block."""
import struct

import pytest

from tests import bai_model as bm
from tests import derive_model as dm
from tests import sam_model as sm
from tools.fuzz_parity import NAME_PLANTS, SAM_PLANTS, consumer_case

SEEDS = range(8)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    td = str(tmp_path_factory.mktemp("consumers"))
    return [consumer_case(seed, td) for seed in SEEDS]


def record_ends(path):
    """The stream offsets behind every record, and the longest record's bytes."""
    _text, _names, s, p = sm.read_bam(path)
    ends, longest = set(), 0
    while p < len(s):
        bs = struct.unpack_from("<I", s, p)[0]
        p += 4 + bs
        longest = max(longest, 4 + bs)
        ends.add(p)
    return ends, longest


def test_parameters_follow_the_seed(cases):
    assert [c["chunk_mb"] for c in cases] == [1, 4, None, 1, 4, None, 1, 4]
    for seed, c in zip(SEEDS, cases):
        assert (c["sam_plant"] is not None) == (seed % 4 == 1) and (c["name_plant"] is not None) == (seed % 4 == 3)
        assert 1 <= c["n"] <= 30_000 and sm.count_records(c["path"]) == c["n"]
        assert c["inflated"] == len(bm.read_blocks(c["path"])[1])
        if c["chunk_mb"] == 1:
            assert c["inflated"] >= 3 << 20, (seed, c["inflated"])
    assert {c["sam_plant"][1] for c in cases if c["sam_plant"]} <= set(SAM_PLANTS)
    assert {c["name_plant"][1] for c in cases if c["name_plant"]} <= set(NAME_PLANTS)


def test_a_case_is_its_seed_s_alone(cases, tmp_path):
    again = consumer_case(3, str(tmp_path))
    assert open(again["path"], "rb").read() == open(cases[3]["path"], "rb").read()
    assert {k: v for k, v in again.items() if k != "path"} == {k: v for k, v in cases[3].items() if k != "path"}


def test_the_models_raise_exactly_on_the_planted_seeds(cases):
    for seed, c in zip(SEEDS, cases):
        if c["sam_plant"]:
            with pytest.raises(sm.SamError) as e:
                sm.expected_sam(c["path"])
            assert e.value.index == c["sam_plant"][0], seed
            assert len(sm.expected_sam(c["path"], e.value.index).split(b"\n")) >= e.value.index    # the records in front are fine
        else:
            assert sm.expected_sam(c["path"]).count(b"\n") >= c["n"]
        names = dm.read_names(c["path"])
        if c["name_plant"]:
            at, name = c["name_plant"]
            with pytest.raises(dm.BadName) as b:
                dm.collect(names)
            assert b.value.name == name == names[at] and names.index(name) == at, seed
            dm.collect(names[:at])
        else:
            ins, fcs, _skipped = dm.collect(names)
            assert ins
        assert any(len(x) == 254 for x in names) or c["name_plant"] or c["sam_plant"]
        bm.expected_bai(c["path"])                  # in coordinate order and inside the limits, whatever was planted


def test_an_empty_member_directly_behind_a_record_and_a_record_longer_than_64_kib(cases):
    behind, longest = 0, 0
    for c in cases:
        blocks, _, _ = bm.read_blocks(c["path"])
        ends, l = record_ends(c["path"])
        longest = max(longest, l)
        behind += sum(1 for k in range(1, len(blocks) - 1)
                      if blocks[k].isize == 0 and blocks[k - 1].isize and blocks[k].out in ends)
    assert behind >= 1
    assert longest > 65536
