"""`ngs generate` on the GPU: the two files the device writes held byte for byte against the model
(tests/generate_model.py) -- at the read lengths, fragment lengths and sequence lengths where a lane, a 64-byte step of the
fragment scan or an eligibility bound changes; the substitution rate and the sequences' shares against the binomial; and the
invariance of the output under the batch size and the split into calls."""
import gzip
import math
import os
import subprocess

import numpy as np
import pytest

from ngs_amd import build, host
from tests import generate_model as gm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def base_fa(tmp_path_factory):
    """A few hundred kilobytes: three sequences, lower-case stretches, N runs, \\r\\n lines in one of them."""
    rng = np.random.default_rng(21)
    d = tmp_path_factory.mktemp("gen")
    recs = [(b"chr1 the first", gm.random_letters(rng, 200_000, lower=[(5_000, 60_000)], n_runs=[(0, 1_000), (90_000, 90_500), (150_000, 150_001)])),
            (b"chr2", gm.random_letters(rng, 100_003, lower=[(0, 100_003)], n_runs=[(40_000, 40_010)])),
            (b"chr3\tx", gm.random_letters(rng, 50_001, n_runs=[(49_000, 50_001)]))]
    path = str(d / "base.fa")
    open(path, "wb").write(gm.fasta_text(recs[:1], 60) + gm.fasta_text(recs[1:2], 70, b"\r\n") + gm.fasta_text(recs[2:], 61))
    return path


@pytest.fixture(scope="module")
def clean_fa(tmp_path_factory):
    rng = np.random.default_rng(22)
    path = str(tmp_path_factory.mktemp("gen") / "clean.fasta")
    open(path, "wb").write(gm.fasta_text([(b"a", gm.random_letters(rng, 200_000)), (b"b", gm.random_letters(rng, 100_000)),
                                          (b"c", gm.random_letters(rng, 50_000))], 80))
    return path


def device_files(gpu_lib, specs, tmp_path, seed, n, first=0, batch=0, tag="d"):
    p1, p2 = str(tmp_path / f"{tag}_1.fastq"), str(tmp_path / f"{tag}_2.fastq")
    rep = host.generate(specs, p1, p2, seed, n, first_pair=first, batch_pairs=batch, lib=gpu_lib)
    return open(p1, "rb").read(), open(p2, "rb").read(), rep


def check_against_model(gpu_lib, specs, tmp_path, seed, n, first=0, batch=0):
    """The device's two files and its rejection counters equal the model's; returns (model result, report)."""
    one, two, rep = device_files(gpu_lib, specs, tmp_path, seed, n, first, batch)
    want = gm.generate([gm.model_provider(s, gpu_lib) for s in specs], seed, first, n)
    assert want.failed_pair is None
    assert len(one) == len(want.one) and len(two) == len(want.two)
    assert one == want.one, first_difference(one, want.one)
    assert two == want.two, first_difference(two, want.two)
    assert rep["pairs"] == n and rep["text_bytes_one"] == len(one) and rep["text_bytes_two"] == len(two)
    assert (rep["rejected_start"], rep["rejected_end"], rep["rejected_base"]) == (want.rejected["start"], want.rejected["end"], want.rejected["base"])
    return want, rep


def first_difference(a, b):
    k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    lo = a.rfind(b"@ngs:", 0, k + 1)
    return f"byte {k}: device {a[max(lo, 0):k + 40]!r} model {b[max(lo, 0):k + 40]!r}"


@pytest.mark.parametrize("L", [1, 63, 64, 65, 129, 150])
def test_read_lengths_around_the_wave(gpu_lib, base_fa, tmp_path, L):
    want, rep = check_against_model(gpu_lib, [(base_fa, 50, 10.0, 2.0, L, 1)], tmp_path, seed=100 + L, n=1500)
    assert rep["rejected_base"] > 0                                                    # the N runs were met
    assert {p[1] for p in want.picks} == {0, 1, 2}


@pytest.mark.parametrize("L,mu,sigma", [
    (32, -1.0, 0.0), (32, 0.0, 0.0), (32, 1.0, 0.0),            # fragments of 63, 64 and 65 bases: the scan's last step
    (64, -1.0, 0.0), (64, 0.0, 0.0), (64, 1.0, 0.0),            # 127, 128, 129
    (64, -64.0, 0.0),                                           # a fragment of exactly L: the mates overlap fully
    (50, -40.0, 3.0),                                           # negative inner distances, 51 .. 69 bases
    (100, -100.0, 0.0),
])
def test_fragment_lengths_around_the_scan_step(gpu_lib, base_fa, tmp_path, L, mu, sigma):
    want, _ = check_against_model(gpu_lib, [(base_fa, 20, mu, sigma, L, 1)], tmp_path, seed=7, n=1200)
    lens = {p[3] for p in want.picks}
    if sigma == 0:
        assert lens == {2 * L + int(mu)}
    else:
        assert min(lens) < 2 * L - 40 < max(lens)


def test_wide_sigma_meets_the_clamps_and_the_sequence_ends(gpu_lib, clean_fa, tmp_path):
    """inner distances 1000 .. 199000 on sequences of 200, 100 and 50 kb: most attempts run past the end, and the two tails
    fold onto the bounds."""
    want, rep = check_against_model(gpu_lib, [(clean_fa, 1000, 100_000.0, 33_000.0, 50, 1)], tmp_path, seed=8, n=2500)
    assert rep["rejected_end"] > 2500 and rep["rejected_base"] == 0
    inner = [p[3] - 100 for p in want.picks]
    assert min(inner) == 1000                                                          # the lower clamp was drawn (0.13 % of the attempts,
                                                                                       # and the shortest fragments are the ones that fit)


def test_sequence_edges(gpu_lib, tmp_path):
    rng = np.random.default_rng(23)
    L = 30
    window = b"N" * 1200 + gm.random_letters(rng, 600) + b"N" * 1200
    recs = [(b"exact", gm.random_letters(rng, 2 * L + 2)), (b"short", gm.random_letters(rng, 2 * L + 1)), (b"window", window),
            (b"lower", gm.random_letters(rng, 500, lower=[(0, 500)])), (b"x", gm.random_letters(rng, 300)),
            (b"n" * 200 + b" a name of 200 bytes", gm.random_letters(rng, 300))]
    path = str(tmp_path / "edges.fa")
    open(path, "wb").write(gm.fasta_text(recs, 50))
    want, rep = check_against_model(gpu_lib, [(path, 10 ** 9, 0.0, 0.0, L, 1)], tmp_path, seed=9, n=3000)
    by_seq = {}
    for p in want.picks:
        by_seq.setdefault(p[1], []).append(p[2])
    assert set(by_seq) == {0, 2, 3, 4, 5}                                              # 2 L + 1 bases: never chosen
    assert set(by_seq[0]) == {1}                                                       # 2 L + 2 bases: the only start is 1
    assert min(by_seq[2]) >= 1201 and max(by_seq[2]) + 2 * L - 1 <= 1800               # found inside the window, after rejections
    assert rep["rejected_base"] > 1000 and rep["rejected_start"] > 0
    one = gm.parse_fastq(open(str(tmp_path / "d_1.fastq"), "rb").read())
    assert any(b.islower() for n, b, _ in one if b":lower:" in n) and all(len(n.split(b":")[2]) in (1, 5, 6, 200) for n, _, _ in one)


@pytest.mark.parametrize("error_freq", [1, 2, 10 ** 9])
def test_error_frequencies(gpu_lib, base_fa, tmp_path, error_freq):
    L = 70
    want, _ = check_against_model(gpu_lib, [(base_fa, error_freq, 0.0, 0.0, L, 1)], tmp_path, seed=10, n=800)
    P = gm.model_provider((base_fa, error_freq, 0.0, 0.0, L, 1), gpu_lib)
    one = gm.parse_fastq(open(str(tmp_path / "d_1.fastq"), "rb").read())
    two = gm.parse_fastq(open(str(tmp_path / "d_2.fastq"), "rb").read())
    comp = bytes(gm.COMPLEMENT)
    differ = total = 0
    for (pi, s, start, flen), (_, b1, _), (_, b2, _) in zip(want.picks, one, two):
        frag = P.seqs[s][1][start - 1:start - 1 + flen]
        for got, ref in ((b1, frag[:L]), (b2, frag[::-1].translate(comp)[:L])):
            differ += sum(g != r for g, r in zip(got, ref))
            total += L
    if error_freq == 1:
        assert differ == total                                                         # every base differs from the reference
    elif error_freq == 2:
        assert abs(differ - total / 2) < 5 * math.sqrt(total / 4)
    else:
        assert differ == 0


def test_substitutions_and_sequence_shares_against_the_binomial(gpu_lib, clean_fa, tmp_path):
    """2 * 10^5 pairs, ERROR_FREQ 50, sigma 0 (so that a name states its whole fragment).  The seed is fixed; the bounds are
    five binomial standard deviations."""
    n, L, mu, E = 200_000, 50, 30, 50
    one, two, rep = device_files(gpu_lib, [(clean_fa, E, float(mu), 0.0, L, 1)], tmp_path, seed=11, n=n)
    assert rep["pairs"] == n
    seqs = gm.parse_fasta(open(clean_fa, "rb").read())
    flat = np.frombuffer(b"".join(s for _, s in seqs), dtype=np.uint8)
    off = dict(zip((nm for nm, _ in seqs), np.concatenate([[0], np.cumsum([len(s) for _, s in seqs])])))
    l1, l2 = one.split(b"\n"), two.split(b"\n")
    names = [x.split(b":") for x in l1[0:4 * n:4]]
    first = np.array([off[x[2]] + int(x[3]) - 1 for x in names], dtype=np.int64)
    j = np.arange(L, dtype=np.int64)
    got1 = np.frombuffer(b"".join(l1[1:4 * n:4]), dtype=np.uint8).reshape(n, L)
    got2 = np.frombuffer(b"".join(l2[1:4 * n:4]), dtype=np.uint8).reshape(n, L)
    ref1 = flat[first[:, None] + j]
    ref2 = gm.COMPLEMENT[flat[(first + 2 * L + mu - 1)[:, None] - j]]
    subs, bases = int((got1 != ref1).sum() + (got2 != ref2).sum()), 2 * n * L
    print(f"substitutions {subs} of {bases} bases: expected {bases / E:.0f}, sd {math.sqrt(bases * (1 / E) * (1 - 1 / E)):.0f}")
    assert abs(subs - bases / E) < 5 * math.sqrt(bases * (1 / E) * (1 - 1 / E))
    total = sum(len(s) for _, s in seqs)                                               # every sequence is eligible
    for nm, s in seqs:
        share, cnt = len(s) / total, sum(1 for x in names if x[2] == nm)
        print(f"sequence {nm.decode()}: {cnt} pairs, expected {n * share:.0f}, sd {math.sqrt(n * share * (1 - share)):.0f}")
        assert abs(cnt - n * share) < 5 * math.sqrt(n * share * (1 - share))


def test_three_providers_with_weights_0_1_3(gpu_lib, base_fa, clean_fa, tmp_path):
    rng = np.random.default_rng(24)
    third = str(tmp_path / "third.fna")
    open(third, "wb").write(gm.fasta_text([(b"only", gm.random_letters(rng, 30_000, lower=[(100, 20_000)]))], 100))
    specs = [(base_fa, 30, 5.0, 1.0, 40, 0), (clean_fa, 30, -3.0, 2.0, 101, 1), (third, 30, 50.0, 10.0, 64, 3)]
    n = 2000
    want, _ = check_against_model(gpu_lib, specs, tmp_path, seed=12, n=n)
    cnt = [sum(1 for p in want.picks if p[0] == k) for k in range(3)]
    assert cnt[0] == 0 and abs(cnt[2] - 0.75 * n) < 5 * math.sqrt(n * 0.75 * 0.25)      # a weight of 0 is never chosen
    one = open(str(tmp_path / "d_1.fastq"), "rb").read()
    assert b"@ngs:clean.fasta:" in one and b"@ngs:third.fna:only:" in one and b"base.fa" not in one


def test_output_does_not_depend_on_the_batch_size_or_the_calls(gpu_lib, base_fa, tmp_path):
    specs = [(base_fa, 25, 10.0, 4.0, 75, 1)]
    n, k = 300, 113
    base = device_files(gpu_lib, specs, tmp_path, 13, n, tag="b0")[:2]
    for bp in (1, 7, 64, 65):
        one, two, rep = device_files(gpu_lib, specs, tmp_path, 13, n, batch=bp, tag=f"b{bp}")
        assert (one, two) == base, bp
        assert rep["batches"] == -(-n // bp)
    p1, p2 = str(tmp_path / "s_1.fq"), str(tmp_path / "s_2.fq")
    with host.Generator(specs, lib=gpu_lib) as g:                                        # two calls of one generator, appended
        g.write(p1, p2, 13, k)
        g.write(p1, p2, 13, n - k, first_pair=k, append=True)
    assert (open(p1, "rb").read(), open(p2, "rb").read()) == base
    assert base[0] == gm.generate([gm.model_provider(specs[0], gpu_lib)], 13, 0, n).one


@pytest.mark.parametrize("first,n", [(0, 120), (2 ** 32 - 5, 10)])
def test_pair_numbers_gain_a_digit(gpu_lib, base_fa, tmp_path, first, n):
    """9 -> 10, 99 -> 100, and 4294967295 -> 4294967296."""
    check_against_model(gpu_lib, [(base_fa, 100, 10.0, 2.0, 36, 1)], tmp_path, seed=14, n=n, first=first)
    names = [x[0] for x in gm.parse_fastq(open(str(tmp_path / "d_2.fastq"), "rb").read())]
    assert [int(x.split(b":")[4][:-2]) for x in names] == list(range(first + 1, first + n + 1))


def test_a_run_longer_than_one_ring_slot(gpu_lib, base_fa, tmp_path):
    """10^5 pairs of 150 bases: each file passes a 32 MiB slot of its writer's ring."""
    want, rep = check_against_model(gpu_lib, [(base_fa, 10_000, 200.0, 30.0, 150, 1)], tmp_path, seed=15, n=100_000)
    assert len(want.one) > (32 << 20) and rep["batches"] == 1


def test_a_job_longer_than_the_whole_ring(gpu_lib, base_fa, tmp_path):
    """420 000 pairs of 150 bases in one batch: each file's single job passes the writer's four 32 MiB slots, so a slot of
    the ring is filled again while the job is still being copied.  Held by SHA-256 against the same pairs in batches of
    2^15, the path the model tests pin (the Python model over 420 000 pairs would take minutes)."""
    import hashlib
    specs, n = [(base_fa, 10_000, 200.0, 30.0, 150, 1)], 420_000

    def digests(batch, tag):
        p1, p2 = str(tmp_path / f"{tag}_1.fastq"), str(tmp_path / f"{tag}_2.fastq")
        rep = host.generate(specs, p1, p2, 17, n, batch_pairs=batch, lib=gpu_lib)
        out = []
        for p in (p1, p2):
            h = hashlib.sha256()
            with open(p, "rb") as f:
                for piece in iter(lambda: f.read(1 << 24), b""):
                    h.update(piece)
            out.append((os.path.getsize(p), h.hexdigest()))
            os.remove(p)
        return out, rep

    big, rep = digests(0, "whole")
    assert rep["batches"] == 1 and rep["pairs"] == n
    assert all(size > 4 * (32 << 20) for size, _ in big), big
    small, rep = digests(1 << 15, "small")
    assert rep["batches"] == -(-n // (1 << 15))
    assert big == small


def test_no_pairs(gpu_lib, base_fa, tmp_path):
    one, two, rep = device_files(gpu_lib, [(base_fa, 100, 10.0, 2.0, 36, 1)], tmp_path, seed=1, n=0)
    assert one == b"" and two == b"" and rep["pairs"] == 0 and rep["batches"] == 0


def test_a_genome_of_n_ends_with_the_attempts_message(gpu_lib, tmp_path):
    path = str(tmp_path / "n.fa")
    open(path, "wb").write(gm.fasta_text([(b"chrN", b"N" * 5000)], 60))
    with pytest.raises(host.NgsqError) as e:
        host.generate([(path, 100, 0.0, 0.0, 50, 1)], str(tmp_path / "n_1.fq"), str(tmp_path / "n_2.fq"), 3, 40, first_pair=1000, lib=gpu_lib)
    assert "no read pair could be drawn from n.fa for pair 1000 in 1024 attempts" in str(e.value)
    assert "almost all N" in str(e.value) and "inner distances are too long" in str(e.value)


def test_command_line_writes_what_the_library_writes(gpu_lib, base_fa, clean_fa, tmp_path):
    ngs = build.build_cli(verbose=False)
    specs = [(base_fa, 40, 12.0, 3.0, 90, 2), (clean_fa, 60, -10.0, 0.0, 33, 1)]
    strings = [f"{base_fa}:40:12:3:90:2", f"{clean_fa}:60:-10:0:33:1"]
    one, two, _ = device_files(gpu_lib, specs, tmp_path, 16, 700)
    o1, o2 = str(tmp_path / "c_1.fq"), str(tmp_path / "c_2.fastq")
    r = subprocess.run([ngs, "generate", "-n", "700", "--seed", "16", "--batch-pairs", "256", o1, o2, *strings], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert b"Generating 700 reads..." in r.stderr
    assert open(o1, "rb").read() == one and open(o2, "rb").read() == two
    z1, z2 = str(tmp_path / "z_1.fastq.gz"), str(tmp_path / "z_2.fq.gz")
    r = subprocess.run([ngs, "-q", "generate", "-n", "700", "--seed", "16", z1, z2, *strings], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert open(z1, "rb").read()[:2] == b"\x1f\x8b" and gzip.decompress(open(z1, "rb").read()) == one
    assert gzip.decompress(open(z2, "rb").read()) == two
    # -c: C * (total bases of the FIRST provider / its read length)
    total = sum(len(s) for _, s in gm.parse_fasta(open(base_fa, "rb").read()))
    r = subprocess.run([ngs, "generate", "-c", "2", "--seed", "16", o1, o2, *strings], capture_output=True, timeout=120)
    want_n = 2 * (total // 90)
    assert r.returncode == 0 and f"Generating {want_n} reads...".encode() in r.stderr, r.stderr
    assert open(o1, "rb").read().count(b"\n") == 4 * want_n and open(o1, "rb").read().startswith(one)
