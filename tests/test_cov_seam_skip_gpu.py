"""The teardown scan's pass over the chunks streamed Coverage has finished (k_cov_scan<*, SKIP>, next_live() in
cov_scan.hip): 64 flagged chunks at a time.

On the small headers of the other tests every wave of the scan owns a single chunk, so that path never runs there.
Here the header is so long that a wave owns 160 chunks or more, and a few thousand 50-base reads in a few batches
make streamed Coverage flag runs of chosen lengths at chosen places of a wave's range.  The result must equal the
difference-array path (sorted_input=False) of the same records integer for integer.  No case is small enough for
the CPU oracle: the header itself is what makes the path run, and the oracle would walk all of it.

The grid has 16 waves per CU (launch_cov_scan) and the library does not expose the CU count, so the header is sized
for 304 CUs: 160 x 4864 chunks (3.2 G positions, a depth block of 12.7 GB that is zeroed once per context).  A wave
then owns 160 chunks on 304 CUs and exactly 190 on the 256 of an MI355X, and every multiple of UNIT = lcm(160, 190)
chunks is where a wave's range begins on either: the cases are placed relative to those.  (The CU count is not asked
of another library in this process on purpose: one that brings its own copy of the collectives library would change
which copy the communicator tests further down the suite load.)

Which chunks a batch flags (cov_stream.hip): with the first 256 records (a tile) on one sequence and the 257th on the
same one, the chunks from chunk_ceil(start of the first) up to chunk_floor(start of the 257th).  The first and the
last chunk of a sequence are never flagged (starts are >= 1; the last chunk holds the sentinel), so a run cannot
cross into the next sequence: the nearest thing, a run up to the last chunk of one sequence and another from the
second chunk of the next, inside one group of 64, is what the two boundary batches build.
"""
import numpy as np
import pytest

from ngs_amd import ffi, host
from tests.util import batch_from_records

pytestmark = pytest.mark.gpu

CHUNK = 4096
UNIT = 3040          # chunks: a wave's range begins at every multiple, whether it owns 160 chunks or 190
TOTAL = 160 * 304 * 16
TILE = 256           # records of a tile of the streaming pass
GUARD = 40 * CHUNK + 100


class Layout:
    """Sequences A, E, B, C.  A ends 70 chunks into the range of a wave, E (three chunks, no record) and the head of B
    follow in the same range; B ends 50 chunks into the range of another wave, C takes the rest."""

    def __init__(self):
        self.total = TOTAL
        self.uA, self.uB = TOTAL // UNIT // 3, 2 * (TOTAL // UNIT) // 3
        cA = UNIT * self.uA + 70
        cE = 3
        cB = UNIT * self.uB + 50 - (cA + cE)
        cC = self.total - (cA + cE + cB)
        self.chunks = [cA, cE, cB, cC]
        self.first = np.concatenate([[0], np.cumsum(self.chunks)]).tolist()
        # ceil((L + 2) / 4096) chunks; the last chunk starts 2095 positions in front of the sentinel L + 1
        self.ref_len = [k * CHUNK - 2002 for k in self.chunks]
        assert max(self.ref_len) < 2**31 - 1

    def local(self, ref, g):
        assert self.first[ref] <= g <= self.first[ref + 1]
        return g - self.first[ref]


def rec(ref, start):
    """A 50-base read whose first covered position (1-based) is `start`."""
    return dict(flag=0, ref_id=ref, pos=int(start) - 1, cigar="50M", seq="ACGT", qual=[30] * 4)


def run_tile(lay, rng, ref, g0, g1, straddle=3):
    """One tile that makes the streaming pass flag the global chunks [g0, g1) of `ref`, given that the next record
    starts at tail_start(): `straddle` reads across the first streamed position (their -1 goes to the chunk sum of the
    first flagged chunk alone, which is then negative: the running carry wraps there), one across the last, the
    rest inside."""
    H, T = lay.local(ref, g0) * CHUNK, lay.local(ref, g1) * CHUNK
    inner = np.sort(rng.integers(H, T - 60, TILE - straddle - 1))
    return [rec(ref, H - 20)] * straddle + [rec(ref, s) for s in inner] + [rec(ref, T - 20)]


def tail(lay, ref, g1, count=4):
    T = lay.local(ref, g1) * CHUNK
    return [rec(ref, T + 10 + i) for i in range(count)]


def build_cases(lay):
    """(batches, flagged global chunks) in coordinate order."""
    rng = np.random.default_rng(25)
    A, B, C = 0, 2, 3
    batches, flagged = [], []

    def one_run(ref, g0, n):
        batches.append(run_tile(lay, rng, ref, g0, g0 + n) + tail(lay, ref, g0 + n))
        flagged.extend(range(g0, g0 + n))

    # ---- A: runs of every length around one and two groups of 64, behind a live first chunk of the wave's range:
    # the group starts at the run, so the live chunk behind it is met by lane n mod 64 (first, last and middle lanes)
    for i, n in enumerate((1, 31, 63, 64, 65, 127, 128, 129)):
        one_run(A, UNIT * (1 + i) + 1, n)
    one_run(A, UNIT * 10, 69)                    # the wave's range begins at the run's first chunk
    one_run(A, UNIT * 12 - 30, 400)              # a run over the whole ranges of one or two waves and into the next
    # ---- the end of A, E without a record, the head of B, all in the range of one wave
    gA = UNIT * lay.uA
    endA, headB = lay.first[1] - 1, lay.first[2] + 1      # last chunk of A (never flagged), second chunk of B
    batches.append(run_tile(lay, rng, A, gA + 2, endA) + tail(lay, A, endA, TILE)
                   + run_tile(lay, rng, B, headB, headB + 45) + tail(lay, B, headB + 45))
    flagged.extend(range(gA + 2, endA))
    flagged.extend(range(headB, headB + 45))
    # ---- B: runs that end exactly where a wave's range ends
    one_run(B, UNIT * (lay.uA + 5) - 60, 60)
    one_run(B, UNIT * (lay.uA + 7) - 140, 140)
    # ---- the end of B and the head of C in the range of one wave: two live chunks side by side inside a group
    gB = UNIT * lay.uB
    endB, headC = lay.first[3] - 1, lay.first[3] + 1
    batches.append(run_tile(lay, rng, B, gB + 1, endB) + tail(lay, B, endB, TILE)
                   + run_tile(lay, rng, C, headC, headC + 100) + tail(lay, C, headC + 100))
    flagged.extend(range(gB + 1, endB))
    flagged.extend(range(headC, headC + 100))
    one_run(C, UNIT * (lay.uB + 30) + 7, 64)
    return [batch_from_records(b) for b in batches], np.array(flagged, dtype=np.int64)


def coverage_of(gpu, n_refs):
    out = []
    for r in range(n_refs):
        seen, hist, ign, bins = gpu.coverage_sequence(r)
        out.append((seen, hist.copy(), ign, bins.copy()))
    return out, gpu.coverage_nonsensical()


def assert_same(got, want):
    (cov_g, non_g), (cov_w, non_w) = got, want
    assert non_g == non_w
    for r, (g, w) in enumerate(zip(cov_g, cov_w)):
        assert g[0] == w[0] and g[2] == w[2], f"sequence {r}: seen / ignored differ"
        assert np.array_equal(g[1], w[1]), f"sequence {r}: depth histogram differs"
        assert np.array_equal(g[3], w[3]), f"sequence {r}: bin totals differ"


KW = dict(facets=ffi.FACET_COVERAGE, bin_size=1_000_000, max_read_len=320)


@pytest.fixture(scope="module")
def cases(gpu_lib):
    """The layout, the batches, the chunks they should flag, and the difference-array path's result (computed once)."""
    lay = Layout()
    batches, flagged = build_cases(lay)
    with host.QcContext(lay.ref_len, lib=gpu_lib, sorted_input=False, **KW) as gpu:
        assert gpu.depth_layout()[1] == lay.total
        for hb in batches:
            gpu.process_batch(hb)
        gpu.finalize()
        want = coverage_of(gpu, 4)
    assert want[0][0][0] and not want[0][1][0] and want[0][2][0] and want[0][3][0]   # E has no entry, the others have
    return lay, batches, flagged, want


def test_flagged_runs_inside_a_waves_range(gpu_lib, cases):
    """Runs of 1, 31, 63, 64, 65, 127, 128 and 129 flagged chunks, runs that begin and end exactly at the ends of a
    wave's range, a run over whole ranges, the sequence boundaries (one with a sequence of no record in between), a
    negative chunk sum at the head of every run; twice through reset."""
    lay, batches, flagged, want = cases
    with host.QcContext(lay.ref_len, lib=gpu_lib, sorted_input=True, **KW) as gpu:
        for _ in range(2):
            gpu.reset()
            for hb in batches:
                gpu.process_batch(hb)
            gpu.finalize()
            assert_same(coverage_of(gpu, 4), want)
        flags = gpu.state_download(4)
    assert np.array_equal(np.flatnonzero(flags[:lay.total]), np.sort(flagged))   # the runs are the ones meant


def test_flagged_runs_with_a_head_guard(gpu_lib, cases):
    """cov_head_guard: the first 40 chunks and a bit behind each sequence's first record stay on the array, so the runs
    of the first batch of every sequence begin elsewhere (or vanish)."""
    lay, batches, flagged, want = cases
    with host.QcContext(lay.ref_len, lib=gpu_lib, sorted_input=True, cov_head_guard=GUARD, **KW) as gpu:
        for hb in batches:
            gpu.process_batch(hb)
        gpu.finalize()
        assert_same(coverage_of(gpu, 4), want)
        flags = gpu.state_download(4)
    got = np.flatnonzero(flags[:lay.total])
    assert 0 < got.size < flagged.size and np.isin(got, flagged).all()
