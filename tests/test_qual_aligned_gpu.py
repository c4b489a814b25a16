"""k_qual_perm on buffer-aligned 16-byte windows (qual_kernel.hip): Quality Score alone over fixed-pitch rows handed over as a raw
device pointer, against a numpy tally written here -- a per-cycle bincount over the rows, 0xFF skipped, values above 93 counted as
errors.  The shapes are the smallest at which the kernel can go wrong: pitches with W < 64, W = P, W = 16 and the first pitch whose
windows wrap into the next row; record counts around one period of the cycle pattern; a base that is not 16-byte aligned inside a
larger allocation; a buffer that ends in the middle of a window; a marked byte at every byte index of two periods.
Run on the GPU box with `pytest -m gpu`.
"""
import math

import numpy as np
import pytest

from ngs_amd import ffi, host

pytestmark = pytest.mark.gpu

PITCHES = (1, 15, 16, 17, 36, 100, 150, 151, 255, 256)
MISALIGN = (0, 1, 7, 8, 15)
PAD_SCORE = 5       # the bytes in front of a misaligned base: a valid score, so a kernel that tallies them fails
HIGH, INVALID = 70, 200


def rows_per_period(pitch):
    return 16 // math.gcd(pitch, 16)


def tally(rows):
    """(cycle x score counts, bad scores) of rows (n, pitch) uint8."""
    n, pitch = rows.shape
    want = np.zeros((pitch, ffi.MAX_SCORE + 1), dtype=np.uint64)
    bad = 0
    cols = np.ascontiguousarray(rows.T)
    for c in range(pitch):
        b = np.bincount(cols[c], minlength=256)
        want[c] = b[:ffi.MAX_SCORE + 1]
        bad += int(b[ffi.MAX_SCORE + 1:255].sum())
    return want, bad


class Runner:
    """One context per pitch (max_read_len == pitch); every run uploads m pad bytes + the rows into an allocation of exactly that size
    and hands the library the pointer m bytes behind its start."""

    def __init__(self, lib, pitch):
        self.pitch = pitch
        self.ctx = host.QcContext([1000], facets=ffi.FACET_QUALITY_SCORE, max_read_len=pitch, lib=lib)
        self.allocs = {}    # (column, bytes) -> device pointer: runs of one shape share their allocations

    def close(self):
        self.ctx.close()

    def run(self, rows, m):
        ctx, (n, pitch) = self.ctx, rows.shape
        assert pitch == self.pitch
        buf = np.concatenate([np.full(m, PAD_SCORE, np.uint8), rows.reshape(-1)])
        flag, l_seq = np.zeros(n, np.uint16), np.full(n, pitch, np.uint32)
        ptrs = {}
        for name, a in (("qual", buf), ("flag", flag), ("l_seq", l_seq)):
            if (name, a.nbytes) not in self.allocs:
                self.allocs[name, a.nbytes] = ctx.device_malloc(a.nbytes)
            ptrs[name] = self.allocs[name, a.nbytes]
            host._check(ctx.lib.ngsq_memcpy_h2d(ctx._ctx, ptrs[name], a.ctypes.data, a.nbytes), ctx._ctx, ctx.lib)
        assert ptrs["qual"] % 16 == 0
        db = host.DeviceBatch(n, dict(ptrs, qual=ptrs["qual"] + m), 0, pitch, 0, 0, 0, n * pitch, 0)
        ctx.reset()
        ctx.process_batch(db)
        ctx.finalize(allow_malformed=True)     # (an invalid score makes finalize report malformed records: the count is what is checked)
        q, bad = ctx.quality_scores(), ctx.error_counts()["bad_quality_score"]
        assert q.shape == (pitch, ffi.MAX_SCORE + 1)
        return q, bad

    def check(self, rows, m, what):
        want, want_bad = tally(rows)
        q, bad = self.run(rows, m)
        print("%s: pitch %d, %d rows, m %d: %d cells differ, bad %d / %d" % (what, self.pitch, rows.shape[0], m,
                                                                            int((q != want).sum()), bad, want_bad))
        assert np.array_equal(q, want), (what, self.pitch, rows.shape[0], m, np.argwhere(q != want)[:8].tolist())
        assert bad == want_bad, (what, self.pitch, rows.shape[0], m)


def contents(rng, n, pitch):
    """uniform: scores 0..63 (every window on the fast path); equal: all rows one score (the worst case for atomics on one word);
    marked: rows padded to the pitch with 0xFF, scores 64..93 and invalid bytes 94..254 sprinkled in."""
    uniform = rng.integers(0, 64, size=(n, pitch), dtype=np.uint8)
    yield "uniform", uniform
    yield "equal", np.full((n, pitch), 37, np.uint8)
    marked = uniform.copy()
    length = rng.integers(0, pitch + 1, size=n)
    length[rng.random(n) < 0.5] = pitch
    marked[np.arange(pitch)[None, :] >= length[:, None]] = 0xFF
    r = rng.random((n, pitch))
    marked[r < 0.02] = rng.integers(64, 94, size=int((r < 0.02).sum()), dtype=np.uint8)
    marked[r > 0.98] = rng.integers(94, 255, size=int((r > 0.98).sum()), dtype=np.uint8)
    yield "marked", marked


@pytest.mark.parametrize("pitch", PITCHES)
def test_counts_equal_the_numpy_tally(gpu_lib, pitch):
    rpp = rows_per_period(pitch)
    counts = sorted({n for n in (1, 2, rpp - 1, rpp, rpp + 1, 1021) if n >= 1})
    rng = np.random.default_rng(1000 + pitch)
    r = Runner(gpu_lib, pitch)
    try:
        for n in counts:
            for what, rows in contents(rng, n, pitch):
                for m in MISALIGN:
                    r.check(rows, m, what)
    finally:
        r.close()


@pytest.mark.parametrize("pitch,m", [(150, 0), (150, 7), (17, 15), (36, 1), (16, 8)])
def test_one_marked_byte_at_every_index_of_two_periods(gpu_lib, pitch, m):
    """A single 0xFF, score 70 or invalid byte at byte index i of a buffer of score 30: exactly one cell loses a count, and one cell
    (70) or the error count (invalid) or nothing (0xFF) gains one.  The kind cycles with i, so every kind meets every byte position
    of a window; the first and the last two windows of the buffer get all three kinds at every byte."""
    n = 2 * rows_per_period(pitch)
    size = n * pitch
    base = np.zeros((pitch, ffi.MAX_SCORE + 1), dtype=np.uint64)
    base[:, 30] = n
    kinds = (0xFF, HIGH, INVALID)
    r = Runner(gpu_lib, pitch)
    try:
        for i in range(size):
            for kind in (kinds if i < 32 or i >= size - 32 else (kinds[i % 3],)):
                rows = np.full((n, pitch), 30, np.uint8)
                rows.reshape(-1)[i] = kind
                q, bad = r.run(rows, m)
                want = base.copy()
                want[i % pitch, 30] -= 1
                if kind == HIGH:
                    want[i % pitch, HIGH] += 1
                assert np.array_equal(q, want), (pitch, m, i, kind, np.argwhere(q != want)[:8].tolist())
                assert bad == (1 if kind == INVALID else 0), (pitch, m, i, kind)
    finally:
        r.close()


@pytest.mark.parametrize("pitch,n,m", [(150, 1_000_003, 7), (160, 300_001, 8), (36, 1_500_001, 15)])
def test_a_full_grid_with_a_shorter_last_run(gpu_lib, pitch, n, m):
    """Enough windows that every working block of a full grid (two blocks of at most 1024 windows per pass on each of 256 CUs) gets
    more than three passes -- the prefetch depth plus one -- and the last one a shorter run that ends in the middle of a window."""
    assert (n * pitch + m + 15) // 16 > 5 * 512 * 1024 and (n * pitch + m) % 16 != 0
    rng = np.random.default_rng(pitch)
    rows = rng.integers(0, 64, size=(n, pitch), dtype=np.uint8)
    flat = rows.reshape(-1)
    at = rng.integers(0, flat.size, size=3 * 1024)
    flat[at[:1024]] = 0xFF
    flat[at[1024:2048]] = rng.integers(64, 94, size=1024, dtype=np.uint8)
    flat[at[2048:]] = rng.integers(94, 255, size=1024, dtype=np.uint8)
    rows[-1, pitch // 2:] = 0xFF
    r = Runner(gpu_lib, pitch)
    try:
        r.check(rows, m, "full grid")
    finally:
        r.close()
