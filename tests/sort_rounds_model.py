"""`ngs convert --gzip device --sort coordinate` in rounds, restated in Python, on top of
tests/bam_sort_model.py: the plan -- the sorted order cut greedily into consecutive ranges whose record bytes and a fixed number
of bytes per record fit the budget -- the walks the restart rule gives, what the survey counts, and where a round's records lie
in the ingest's view and in its slab.  The two per-record constants are the library's (ngsq_sort_resident_bytes_per_record,
ngsq_sort_survey_bytes_per_record): callers read them there and hand them in.  Nothing else here calls the library.  Also here:
the inputs that tests/test_sort_rounds.py checks on the CPU and tests/test_sort_rounds_gpu.py converts."""
import gzip
import random
import struct
from typing import List, NamedTuple

from tests import bam_sort_model as bsm
from tests import sort_model as som


class Round(NamedTuple):
    first: int      # sorted ranks [first, end)
    end: int
    bytes: int      # of its records

    def resident(self, per_record: int) -> int:
        return self.bytes + (self.end - self.first) * per_record


class RecordTooLarge(Exception):
    def __init__(self, rank: int, need: int):
        super().__init__(rank, need)
        self.rank, self.need = rank, need


def plan(sorted_lengths: List[int], budget: int, per_record: int) -> List[Round]:
    """A round takes records of the sorted order while their bytes and per_record each fit the budget; it ends at the last
    record that still fits.  A record that does not fit a round of its own: RecordTooLarge(its sorted rank, what it needs)."""
    out, first = [], 0
    while first < len(sorted_lengths):
        end, total = first, 0
        while end < len(sorted_lengths) and total + sorted_lengths[end] + (end + 1 - first) * per_record <= budget:
            total += sorted_lengths[end]
            end += 1
        if end == first:
            raise RecordTooLarge(first, sorted_lengths[first] + per_record)
        out.append(Round(first, end, total))
        first = end
    return out


def records_of(bam: bytes, max_records: int = 0) -> List[bytes]:
    recs = bsm.split(gzip.decompress(bam))[2]
    return recs[:max_records] if max_records else recs


def order_of(recs: List[bytes]) -> List[int]:
    """perm: the input ordinal of every sorted rank (equal keys in input order)."""
    return som.order([som.key(r) for r in recs])


def plan_of(bam: bytes, budget: int, per_record: int, max_records: int = 0) -> List[Round]:
    recs = records_of(bam, max_records)
    return plan([len(recs[i]) for i in order_of(recs)], budget, per_record)


def fits(recs: List[bytes], budget: int, per_record: int) -> bool:
    return sum(len(r) for r in recs) + len(recs) * per_record <= budget


def walks(rounds: int) -> int:
    """The restart rule: a file that fits is walked once; else the attempt that overflowed, the survey, and a walk per round."""
    return 1 if rounds == 1 else 2 + rounds


def budget_for(recs: List[bytes], per_record: int, rounds: int) -> int:
    """The smallest budget whose plan has at most `rounds` rounds (the greedy count never grows with the budget)."""
    lengths = [len(recs[i]) for i in order_of(recs)]
    lo, hi = max(lengths) + per_record, sum(lengths) + len(lengths) * per_record
    while lo < hi:
        mid = (lo + hi) // 2
        if len(plan(lengths, mid, per_record)) <= rounds:
            hi = mid
        else:
            lo = mid + 1
    return lo


def view_offsets(bam: bytes) -> List[int]:
    """Every record's offset in the decompressed input: its place in the ingest's view, whose first chunk begins on a 16-byte
    boundary (tests/test_bam_sort_gpu.batch_start_residues)."""
    text, table, recs = bsm.split(gzip.decompress(bam))
    at, out = 8 + len(text) + len(table), []
    for r in recs:
        out.append(at)
        at += len(r)
    return out


def kept(recs: List[bytes], rounds: List[Round]) -> List[List[int]]:
    """Per round, the input ordinals of its records in input order: the order they are compacted in."""
    perm = order_of(recs)
    return [sorted(perm[r.first:r.end]) for r in rounds]


def slab_offsets(recs: List[bytes], ordinals: List[int]) -> List[int]:
    """Where a round's kept records land behind the round's first (one slab, whose front is aligned)."""
    at, out = 0, []
    for i in ordinals:
        out.append(at)
        at += len(recs[i])
    return out


def batches_touched(ordinals: List[int], n: int, batch: int) -> int:
    return len({i // batch for i in ordinals}) if batch else 1


def boundary_keys(recs: List[bytes], rounds: List[Round]):
    """(key in front of the boundary, key behind it) for every boundary between two rounds."""
    keys = sorted(som.key(r) for r in recs)
    return [(keys[r.end - 1], keys[r.end]) for r in rounds[:-1]]


def piece_cuts(rounds: List[Round], piece_bytes: int):
    """The stream offsets of the boundaries between rounds, and which of them fall inside a piece."""
    at, cuts = 0, []
    for r in rounds[:-1]:
        at += r.bytes
        cuts.append(at)
    return cuts, [c for c in cuts if c % piece_bytes]


# ---- the inputs ---------------------------------------------------------------------------------------------------------------
def raw_record(ref: int, pos: int, name: bytes, filler: int = 0, flag: int = 0) -> bytes:
    """A whole BAM record without bases or CIGAR: `filler` bytes of an XZ:Z tag make it longer."""
    aux = (b"XZZ" + b"z" * (filler - 4) + b"\0") if filler >= 4 else b""
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name) + 1, 0, 4680, 0, flag, 0, -1, -1, 0) + name + b"\0" + aux
    return struct.pack("<I", len(body)) + body


def shuffled(recs: List[bytes], seed: int) -> List[bytes]:
    out = list(recs)
    random.Random(seed).shuffle(out)
    return out


def tie_group_records() -> List[bytes]:
    """150 records in front, 200 at one position whose names tell their input order, 150 behind; shuffled but for the ties'
    relative order, which the names record."""
    rng = random.Random(31)
    front = [raw_record(0, 10 + k, b"f%d" % k, rng.randrange(0, 40)) for k in range(150)]
    back = [raw_record(0, 9000 + k, b"b%d" % k, rng.randrange(0, 40)) for k in range(150)]
    slots = sorted(rng.sample(range(500), 200))
    others = shuffled(front + back, 32)
    out, t = [], 0
    for k in range(500):
        if t < 200 and k == slots[t]:
            out.append(raw_record(0, 5000, b"tie%03d" % t, (t * 7) % 23 + 4))
            t += 1
        else:
            out.append(others.pop())
    return out


def unplaced_records() -> List[bytes]:
    """The unplaced block of tests/test_bam_sort_gpu.test_unplaced_records_go_last_in_input_order, scaled up: 120 placed records,
    and 180 without a place of which every fifth has a sequence and no position (refID >= 0, pos -1)."""
    rng = random.Random(33)
    placed = [raw_record(k % 3, rng.randrange(0, 4000), b"p%d" % k, rng.randrange(0, 60)) for k in range(120)]
    un = [raw_record(k % 3 if k % 5 == 0 else -1, -1, (b"zero%d" if k % 5 == 0 else b"u%d") % k, rng.randrange(0, 60), flag=4) for k in range(180)]
    out = placed + un
    order = list(range(300))
    rng.shuffle(order)
    return [out[i] for i in order]


REFS3 = [(b"chr1", 300_000), (b"chr2", 70_000), (b"chr3", 5_000)]
TEXT3 = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n, l) for n, l in REFS3)


def bam_of_records(recs: List[bytes], payload: int = 65280) -> bytes:
    """A BAM file of these records in this order, three sequences in its header (zlib's blocks: tests/bam_text_model.py)."""
    from tests import bam_text_model as tm
    s = b"BAM\1" + struct.pack("<i", len(TEXT3)) + TEXT3 + struct.pack("<i", len(REFS3))
    for n, l in REFS3:
        s += struct.pack("<i", len(n) + 1) + n + b"\0" + struct.pack("<i", l)
    return tm.bam_file(s + b"".join(recs), payload)


def ramp_records(n: int) -> List[bytes]:
    """n records in coordinate order over the three sequences, of some 60 to 120 bytes."""
    return [raw_record(k * 3 // n, 1 + k * 7, b"q%d" % k, (k * 13) % 61) for k in range(n)]


def case_ties(per_record: int):
    recs = tie_group_records()
    return bam_of_records(recs), budget_for(recs, per_record, 2)


def case_unplaced(per_record: int):
    recs = unplaced_records()
    return bam_of_records(recs), budget_for(recs, per_record, 3)


def case_reversed(n: int, per_record: int):
    recs = list(reversed(ramp_records(n)))
    return bam_of_records(recs), budget_for(recs, per_record, 3)


def case_sorted(per_record: int):
    recs = ramp_records(1200)
    return bam_of_records(recs, 7000), budget_for(recs, per_record, 4)


def most_rounds_budget(recs: List[bytes], survey_per_record: int) -> int:
    """The smallest budget the survey allows: its arrays' count."""
    return len(recs) * survey_per_record


def spanning_records(recs: List[bytes], rounds: List[Round], piece_bytes: int):
    """The records next to a boundary between rounds that lie in two pieces: the first record of a round that begins in the piece
    the round in front of it ends in and ends in the next piece, so that it spans two pieces and the first of them two rounds."""
    lengths = [len(recs[i]) for i in order_of(recs)]
    cuts = piece_cuts(rounds, piece_bytes)[0]
    return [r.first for c, r in zip(cuts, rounds[1:]) if c % piece_bytes and c // piece_bytes != (c + lengths[r.first] - 1) // piece_bytes]


def alignment_budget(recs: List[bytes], per_record: int, piece_bytes: int = 1000) -> int:
    """The largest budget of three rounds or more at which a record spans two pieces and two rounds' piece (spanning_records)."""
    b = budget_for(recs, per_record, 3)
    lengths = [len(recs[i]) for i in order_of(recs)]
    while not spanning_records(recs, plan(lengths, b, per_record), piece_bytes):
        b -= 1
    return b
