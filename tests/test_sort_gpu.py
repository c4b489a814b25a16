"""The sort of `ngs convert --sort coordinate` alone on the GPU: host.sort_u64 (ngsq_sort_u64_device)
against numpy.argsort(kind="stable").  Sizes at the edges of a wave (64), of the other kernels' blocks (256) and of the ranking
tile T = ngsq_sort_tile_keys(); key patterns for every way a pass can go: skipped, one bin nearly full, every bin in use,
ties across waves and tiles."""
import numpy as np
import pytest

from ngs_amd import host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T(gpu_lib):
    return int(gpu_lib.ngsq_sort_tile_keys())


def sizes(T):
    return [0, 1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 7]


def check(lib, keys):
    keys = np.asarray(keys, dtype=np.uint64)
    perm, rep = host.sort_u64(keys, lib=lib)
    want = np.argsort(keys, kind="stable").astype(np.uint32)
    assert perm.dtype == np.uint32 and perm.shape == want.shape
    bad = np.nonzero(perm != want)[0]
    assert bad.size == 0, f"n {len(keys)}: perm differs at {bad[:5]}: got {perm[bad[:5]]} want {want[bad[:5]]}"
    assert rep["passes_run"] + rep["passes_skipped"] == 8
    return perm, rep


def test_all_keys_equal_skip_every_pass(gpu_lib, T):
    for n in sizes(T):
        for v in (0, 0xFFFFFFFF00000000, 0x0123456789ABCDEF):
            perm, rep = check(gpu_lib, np.full(n, v, np.uint64))
            assert (rep["passes_run"], rep["passes_skipped"]) == (0, 8)
            assert np.array_equal(perm, np.arange(n, dtype=np.uint32))


@pytest.mark.parametrize("shift", [56, 0])
def test_keys_that_differ_in_one_byte_alone(gpu_lib, T, shift):
    rng = np.random.default_rng(70 + shift)
    base = np.uint64(0x00A1B2C3D4E5F600 if shift == 0 else 0x00A1B2C3D4E5F6A7)
    for n in sizes(T):
        keys = base | (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(shift))
        _, rep = check(gpu_lib, keys)
        assert rep["passes_run"] == (1 if len(set(keys.tolist())) > 1 else 0), n


def test_random_keys_use_all_eight_digits(gpu_lib, T):
    rng = np.random.default_rng(71)
    for n in sizes(T):
        _, rep = check(gpu_lib, rng.integers(0, 2 ** 64, n, dtype=np.uint64))
        if n >= 63:
            assert rep["passes_run"] == 8


def test_ascending_and_descending(gpu_lib, T):
    for n in sizes(T):
        up = np.arange(n, dtype=np.uint64) * np.uint64(0x0001000100010001)
        perm, _ = check(gpu_lib, up)
        assert np.array_equal(perm, np.arange(n, dtype=np.uint32))
        perm, _ = check(gpu_lib, up[::-1].copy())
        assert np.array_equal(perm, np.arange(n, dtype=np.uint32)[::-1])


def test_sixteen_values_over_five_tiles_keep_input_order(gpu_lib, T):
    """Ties across waves and tiles: every value's indices come out ascending."""
    rng = np.random.default_rng(72)
    values = rng.integers(0, 2 ** 64, 16, dtype=np.uint64)
    keys = values[rng.integers(0, 16, 5 * T)]
    perm, _ = check(gpu_lib, keys)
    for v in values:
        own = perm[keys[perm] == v]
        assert np.all(np.diff(own.astype(np.int64)) > 0)


def test_one_digit_value_holds_all_but_one_key(gpu_lib, T):
    for n in (2, 65, 257, T + 1, 3 * T + 7):
        for at in (0, n // 2, n - 1):
            for odd in (0x00, 0xFF):                                   # the odd key sorts in front or behind
                for shift in (0, 24, 56):
                    keys = np.full(n, 0x5A5A5A5A5A5A5A5A, np.uint64)
                    keys[at] = (int(keys[at]) & ~(0xFF << shift)) | (odd << shift)
                    _, rep = check(gpu_lib, keys)
                    assert rep["passes_run"] == 1


def test_the_same_input_gives_the_same_permutation(gpu_lib, T):
    rng = np.random.default_rng(73)
    for n in (257, 3 * T + 7):
        keys = rng.integers(0, 1 << 20, n, dtype=np.uint64) << np.uint64(7)   # many ties
        a, _ = check(gpu_lib, keys)
        b, _ = check(gpu_lib, keys)
        assert np.array_equal(a, b)


def test_coordinate_shaped_keys_skip_the_passes_the_design_names(gpu_lib, T):
    """One sequence with positions below 2^24: three passes.  25 sequences, positions below 2^28: five."""
    rng = np.random.default_rng(74)
    n = 2 * T + 5
    _, rep = check(gpu_lib, rng.integers(1, 1 << 24, n, dtype=np.uint64))
    assert rep["passes_run"] == 3
    keys = rng.integers(0, 25, n, dtype=np.uint64) << np.uint64(32) | rng.integers(1, 1 << 28, n, dtype=np.uint64)
    _, rep = check(gpu_lib, keys)
    assert rep["passes_run"] == 5
