"""Streamed Coverage beside k_gc (context.cpp launch_all: k_cov_stream forked to the context's side stream, joined in front of the
quality kernel; cov_stream.hip: runs of tiles handed out through a counter).  Every case is checked against the oracle and against
a context on the difference-array path: the integers do not depend on which stream a kernel ran on, on how the tiles were split
into runs, or on how many batches were in flight."""
import numpy as np
import pytest

from ngs_amd import ffi, host
from tests.util import batch_from_records, compare_contexts, coordinate_sorted, json_equal, random_batch, take_records

pytestmark = pytest.mark.gpu

CS_RUN = 48          # kernels.h: tiles of 256 records per run, once a batch gives every wave of the grid more than that
EDGE_REF_LEN = [60_000, 1, 777, 30_000, 9_000]
EDGE_PRIMARY = [1, 1, 0, 1, 1]
SIZES = [1, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]


def names(ref_len):
    return [f"chr{i + 1}" for i in range(len(ref_len))]


def oracle_of(oracle_mod, batches, ref_len, primary, kw):
    orc = oracle_mod.Oracle(ref_len, primary, **kw)
    for hb in batches:
        orc.process_batch(hb)
    return orc, orc.finalize(allow_malformed=True)


def array_results(lib, batches, ref_len, primary, kw):
    with host.QcContext(ref_len, primary, lib=lib, sorted_input=False, **kw) as gpu:
        for hb in batches:
            gpu.process_batch(hb)
        gpu.finalize(allow_malformed=True)
        return gpu.results(names(ref_len))


def check(gpu, orc, rc_o, arrays, ref_len, kw):
    assert gpu.finalize(allow_malformed=True) == rc_o
    compare_contexts(gpu, orc, len(ref_len), kw["facets"], kw["bin_size"], ref_len)
    doc = gpu.results(names(ref_len))
    json_equal(doc, orc.results(names(ref_len)))
    json_equal(doc, arrays)


def run_case(oracle_mod, lib, batches, ref_len, primary=None, facets=ffi.FACETS_DEFAULT, bin_size=1000, max_read_len=320,
             on_device=False, passes=1, cov_cap=0, **ctx_kw):
    kw = dict(facets=facets, bin_size=bin_size, max_read_len=max_read_len, gc_seed=7, cov_cap=cov_cap)
    orc, rc_o = oracle_of(oracle_mod, batches, ref_len, primary, kw)
    arrays = array_results(lib, batches, ref_len, primary, kw)
    with host.QcContext(ref_len, primary, lib=lib, sorted_input=True, **kw, **ctx_kw) as gpu:
        for p in range(passes):
            if p:
                gpu.reset()
            dev = [gpu.upload(hb) for hb in batches] if on_device else batches
            for b in dev:                       # back to back: nothing waits for the device between the batches
                gpu.process_batch(b)
            check(gpu, orc, rc_o, arrays, ref_len, kw)
        return gpu.kernel_timing()


def cut(hb, sizes):
    out, lo = [], 0
    for s in sizes:
        out.append(take_records(hb, np.arange(lo, lo + s)))
        out[-1].first_record_index = lo
        lo += s
    assert lo == hb.n
    return out


@pytest.fixture(scope="module")
def forty_batches():
    rng = np.random.default_rng(41)
    sizes = [int(s) for s in rng.choice(SIZES, 40)]
    sizes[:10] = SIZES                                         # every size at least once
    return cut(coordinate_sorted(random_batch(rng, sum(sizes), EDGE_REF_LEN)), sizes)


@pytest.mark.parametrize("on_device", [False, True])
def test_forty_batches_back_to_back(gpu_lib, oracle_mod, forty_batches, on_device):
    """The cross-batch hazards (the cov_end column, the two largest-span words, the plan words, the run counter, end_acc): forty
    batches of every awkward size with no host synchronisation between them, finalize at once, twice through reset."""
    t = run_case(oracle_mod, gpu_lib, forty_batches, EDGE_REF_LEN, EDGE_PRIMARY, on_device=on_device, passes=2)
    assert t["cov_stream"]["launches"] == 80 and t["gc"]["launches"] == 80


@pytest.mark.parametrize("n", [256 * CS_RUN - 1, 256 * CS_RUN, 256 * CS_RUN + 1, 256 * 7 + 3, 300_000])
def test_small_batches_synthetic(gpu_lib, oracle_mod, n):
    """Batches too small for runs of CS_RUN tiles, against the oracle: the launcher gives every wave its even share instead (here one
    tile per run: 48 or 49 runs, 8 runs, 1172 runs, each on a grid with a wave per run), taken from the counter all the same.  Runs of
    CS_RUN tiles and waves that take several of them need tens of millions of records: test_runs_of_cs_run_tiles."""
    L = 60 * n + 10_000 if n < 100_000 else 700_000
    hb = host.synth_host_batch(host.synth_config(n, ref_len=L, n_refs=2), 0, n, gpu_lib)
    run_case(oracle_mod, gpu_lib, [hb], [L, 300_000], bin_size=50_000, max_read_len=150, on_device=True)


def test_walk_back_at_every_run_start(gpu_lib, oracle_mod):
    """120 000 mixed 50-300 bp records with 1.5 Mb skips and a pile deeper than the list of open ends: a run that starts behind
    them has to walk back through all of it."""
    n, L = 118_000, 3_000_000
    cfg = host.synth_config(n, mode=ffi.SYNTH_MIXED, ref_len=L, n_refs=1)
    recs = []
    for p in range(100_000, 2_900_000, 70_000):                # long skips that cross thousands of tiles
        recs.append(dict(flag=0, ref_id=0, pos=p, cigar="20M1500000N20M" if p < 1_400_000 else "20M90000N20M", seq="ACGT", qual=[30] * 4))
    for _ in range(2000 - len(recs)):                          # a pile of 300+ open ends (the list holds 232)
        recs.append(dict(flag=0, ref_id=0, pos=1_500_000 + len(recs) % 7, cigar="60M5000N60M", seq="ACGT", qual=[30] * 4))
    syn = host.synth_host_batch(cfg, 0, n, gpu_lib)
    extra = batch_from_records(recs)
    # one batch of both, in coordinate order (the columns of the two are concatenated record by record)
    order_key = np.concatenate([syn.cols["ref_id"].astype(np.int64) << 32 | syn.cols["pos"].astype(np.int64),
                                extra.cols["ref_id"].astype(np.int64) << 32 | extra.cols["pos"].astype(np.int64)])
    if syn.cols.get("seq_off") is None or extra.cols.get("seq_off") is None:
        pytest.fail("both batches are expected in the offsets layout")
    merged = merge_offsets_batches(syn, extra)
    hb = take_records(merged, np.argsort(order_key, kind="stable"))
    assert hb.n == 120_000
    run_case(oracle_mod, gpu_lib, [hb], [L], facets=ffi.FACETS_DEFAULT, bin_size=50_000, max_read_len=300, on_device=True)


def merge_offsets_batches(a, b):
    cols = {}
    for k in ("flag", "mapq", "ref_id", "pos", "mate_ref_id", "tlen", "l_seq", "n_cigar", "seq", "qual", "cigar"):
        cols[k] = np.concatenate([a.cols[k], b.cols[k].astype(a.cols[k].dtype)])
    for k in ("seq_off", "qual_off", "cigar_off"):
        cols[k] = np.concatenate([a.cols[k], b.cols[k][1:] + a.cols[k][-1]]).astype(np.uint64)
    return host.HostBatch(a.n + b.n, cols, 0, 0, 0, 0)


def test_runs_longer_than_one_tile(gpu_lib):
    """More tiles than waves of the grid, fewer than CS_RUN per wave: runs of five tiles (the even share), about one per wave, with a
    partial last tile.  The two Coverage paths agree (no oracle at this size)."""
    n, L = 3_200_001, 40_000_000
    cfg = host.synth_config(n, ref_len=L, n_refs=2)
    docs = []
    for sorted_input in (False, True):
        with host.QcContext([L, 300_000], lib=gpu_lib, sorted_input=sorted_input, bin_size=50_000, max_read_len=150, gc_seed=7) as gpu:
            gpu.process_batch(gpu.synth_device_batch(cfg, 0, n))
            gpu.finalize()
            docs.append(gpu.results(["chr1", "chr2"]))
    json_equal(docs[1], docs[0])


def test_runs_of_cs_run_tiles(gpu_lib):
    """The path the benchmark runs: runs of exactly CS_RUN tiles, more runs than waves.  A run is CS_RUN tiles once the even share
    of a wave exceeds that: more than CS_RUN x 12 waves x 256 records per CU, 37.7 M records on 256 CUs, 44.8 M on 304.  At 60 M
    records there are 4883 or 4884 runs for the 3072 waves of the grid (2048 of them resident while k_gc runs), so waves take
    several runs from the counter and the blocks that become resident late take what is left.  Three prefixes of one device batch:
    the partial last tile inside a run of 48, no partial tile and a last run that is full, a last run that is the partial tile
    alone.  Checked against a context on the array path (no oracle at this size)."""
    L = 248_956_422
    runs = 4883
    sizes = [60_000_001, 256 * CS_RUN * runs, 256 * CS_RUN * runs + 1]
    assert 256 * CS_RUN * (runs - 1) < sizes[0] < sizes[1]
    n_max = max(sizes)
    cfg = host.synth_config(n_max, ref_len=L, n_refs=2)
    kw = dict(lib=gpu_lib, bin_size=50_000, max_read_len=150, gc_seed=7, timing=True)
    with host.QcContext([L, 300_000], sorted_input=True, **kw) as streamed, host.QcContext([L, 300_000], sorted_input=False, **kw) as arrays:
        db = streamed.synth_device_batch(cfg, 0, n_max)
        for n in sizes:
            part = host.DeviceBatch(n, db.ptrs, db.seq_stride, db.qual_stride, db.cigar_stride, 0, n * db.seq_stride, n * db.qual_stride,
                                    n * db.cigar_stride)
            docs = []
            for gpu in (streamed, arrays):
                gpu.reset()
                gpu.process_batch(part)
                gpu.finalize()
                docs.append(gpu.results(["chr1", "chr2"]))
            json_equal(docs[0], docs[1])
        streamed.synchronize()
        t = streamed.kernel_timing()
        assert t["cov_stream"]["launches"] == 3 and t["gc"]["launches"] == 3 and t["cov_stream"]["total_ms"] > 0


@pytest.mark.parametrize("facets,corun,gc_launches", [
    (ffi.FACET_COVERAGE | ffi.FACET_GC_CONTENT, True, 3),
    (ffi.FACET_COVERAGE | ffi.FACET_GENERAL, False, 0),
    (ffi.FACETS_DEFAULT, True, 3),
])
def test_facet_masks(gpu_lib, oracle_mod, forty_batches, facets, corun, gc_launches):
    t = run_case(oracle_mod, gpu_lib, forty_batches[7:10], EDGE_REF_LEN, EDGE_PRIMARY, facets=facets)
    assert t["cov_stream"]["launches"] == 3 and t["gc"]["launches"] == gc_launches


def test_all_seven_facets_keep_one_stream(gpu_lib, oracle_mod):
    """GC Content tallied by the Edits kernel (fixed-pitch rows): no k_gc of its own, so nothing to run beside."""
    from tests.util import make_edit_friendly, random_ref_bases, to_fixed_stride
    rng = np.random.default_rng(3)
    ref_len = [50_000, 20_000]
    bases = random_ref_bases(rng, ref_len)
    hb = to_fixed_stride(coordinate_sorted(make_edit_friendly(random_batch(rng, 6000, ref_len, weird=False, min_len=60, max_len=160), rng, bases, ref_len)))
    assert hb.cols["seq_off"] is None
    facets = ffi.FACETS_DEFAULT | ffi.FACET_EDITS
    kw = dict(facets=facets, bin_size=1000, max_read_len=160, gc_seed=7)
    orc = oracle_mod.Oracle(ref_len, None, ref_bases=bases, **kw)
    orc.process_batch(hb)
    rc_o = orc.finalize(allow_malformed=True)
    with host.QcContext(ref_len, lib=gpu_lib, sorted_input=True, ref_bases=bases, **kw) as gpu:
        gpu.process_batch(hb)
        assert gpu.finalize(allow_malformed=True) == rc_o
        compare_contexts(gpu, orc, 2, facets, 1000, ref_len)
        json_equal(gpu.results(["chr1", "chr2"]), orc.results(["chr1", "chr2"]))
        t = gpu.kernel_timing()
        assert t["gc"]["launches"] == 0 and t["edits"]["launches"] == 1 and t["cov_stream"]["launches"] == 1


@pytest.mark.parametrize("timing", [True, False])
def test_timing_brackets_on_both_streams(gpu_lib, oracle_mod, forty_batches, timing):
    k = 5
    t = run_case(oracle_mod, gpu_lib, forty_batches[3:3 + k], EDGE_REF_LEN, EDGE_PRIMARY, timing=timing)
    for name in ("cov_stream", "gc"):
        assert t[name]["launches"] == k
        assert (t[name]["total_ms"] > 0) == timing, t[name]


def test_timing_leaves_no_event_pending(gpu_lib, forty_batches):
    """What finalize resolved stays resolved: a second reading adds nothing, a reset of the table leaves it empty (an event still
    pending on either stream would be added then), and a second pass counts its own launches and time only."""
    batches = forty_batches[3:8]
    with host.QcContext(EDGE_REF_LEN, EDGE_PRIMARY, lib=gpu_lib, sorted_input=True, max_read_len=320, gc_seed=7, timing=True) as gpu:
        for b in batches:
            gpu.process_batch(b)
        gpu.finalize(allow_malformed=True)
        first = gpu.kernel_timing()
        assert gpu.kernel_timing() == first
        gpu.synchronize()
        assert gpu.kernel_timing() == first
        gpu.kernel_timing_reset()
        empty = gpu.kernel_timing()
        assert all(v["launches"] == 0 and v["total_ms"] == 0 for v in empty.values()), empty
        gpu.reset()
        for b in batches[:2]:
            gpu.process_batch(b)
        gpu.finalize(allow_malformed=True)
        second = gpu.kernel_timing()
        for name in ("cov_stream", "gc"):
            assert second[name]["launches"] == 2 and second[name]["total_ms"] > 0
    with host.QcContext(EDGE_REF_LEN, EDGE_PRIMARY, lib=gpu_lib, sorted_input=True, max_read_len=320, gc_seed=7, timing=False) as gpu:
        for b in batches:
            gpu.process_batch(b)
        gpu.finalize(allow_malformed=True)
        gpu.kernel_timing_reset()
        assert all(v["launches"] == 0 and v["total_ms"] == 0 for v in gpu.kernel_timing().values())


def test_two_contexts_interleaved(gpu_lib, oracle_mod, forty_batches):
    a_b, b_b = renumber(forty_batches[:6]), renumber(forty_batches[6:12])
    kw = dict(facets=ffi.FACETS_DEFAULT, bin_size=1000, max_read_len=320, gc_seed=7, cov_cap=0)
    sides = [(bs, *oracle_of(oracle_mod, bs, EDGE_REF_LEN, EDGE_PRIMARY, kw), array_results(gpu_lib, bs, EDGE_REF_LEN, EDGE_PRIMARY, kw))
             for bs in (a_b, b_b)]
    with host.QcContext(EDGE_REF_LEN, EDGE_PRIMARY, lib=gpu_lib, sorted_input=True, **kw) as ga, \
            host.QcContext(EDGE_REF_LEN, EDGE_PRIMARY, lib=gpu_lib, sorted_input=True, **kw) as gb:
        for x, y in zip(a_b, b_b):
            ga.process_batch(x)
            gb.process_batch(y)
        for g, (bs, orc, rc_o, arrays) in zip((ga, gb), sides):
            check(g, orc, rc_o, arrays, EDGE_REF_LEN, kw)


def renumber(batches):
    lo = 0
    for b in batches:
        b.first_record_index = lo
        lo += b.n
    return batches


def test_context_on_a_callers_stream(gpu_lib, oracle_mod, forty_batches):
    """The side stream is the context's own also when its stream is not: here the stream of another context."""
    with host.QcContext([1000], lib=gpu_lib) as owner:
        run_case(oracle_mod, gpu_lib, renumber(forty_batches[12:18]), EDGE_REF_LEN, EDGE_PRIMARY, stream=owner.stream)


def test_unsorted_refused_and_close_without_finalize(gpu_lib, forty_batches):
    rng = np.random.default_rng(5)
    ref_len = [50_000, 20_000]
    hb = coordinate_sorted(random_batch(rng, 5000, ref_len, weird=False))
    swapped = np.arange(hb.n)
    swapped[[1000, 3000]] = [3000, 1000]
    with host.QcContext(ref_len, lib=gpu_lib, sorted_input=True, max_read_len=320) as gpu:
        gpu.process_batch(take_records(hb, swapped))
        with pytest.raises(host.NgsqError) as ei:
            gpu.finalize()
        assert ei.value.code == ffi.ERR_UNSORTED
    for _ in range(3):                         # closed with both streams busy: neither a leak nor a hang, and the next one works
        gpu = host.QcContext(ref_len, lib=gpu_lib, sorted_input=True, max_read_len=320)
        gpu.process_batch(hb)
        gpu.close()
