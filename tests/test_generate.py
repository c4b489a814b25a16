"""`ngs generate` without a GPU: the test-side model (tests/generate_model.py) held to the reference's
rules on a small FASTA, the library's inner-distance table against math.erf, the host side of opening a generator (the bases
of every record counted on the host, the up-front refusals), the gzip pipe, every message of the command line, and the
provider-string parser and the table builder under the sanitizers, driven by a stand-alone C program."""
import gzip
import math
import os
import subprocess

import numpy as np
import pytest

from ngs_amd import build, ffi, host
from tests import generate_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def ngs(lib):
    return build.build_cli(verbose=False)


def run(ngs, *args):
    return subprocess.run([ngs, *args], capture_output=True, timeout=120)


def small_fasta(rng):
    """Several sequences with lower-case stretches, N runs and \\r\\n lines; one too short to be eligible for 20-base reads."""
    recs = [
        (b"chrA first", gm.random_letters(rng, 900, lower=[(100, 260)], n_runs=[(400, 430), (700, 701)])),
        (b"chrB", gm.random_letters(rng, 333, lower=[(0, 333)])),
        (b"tiny", gm.random_letters(rng, 41)),
        (b"chrC\tlast", gm.random_letters(rng, 1500, n_runs=[(0, 50), (1450, 1500)])),
    ]
    return recs, gm.fasta_text(recs[:2], 60, b"\r\n") + gm.fasta_text(recs[2:], 70, b"\n")


# ---- the model obeys the reference's rules -------------------------------------------------------------------------------------
@pytest.mark.parametrize("error_freq,mu,sigma", [(10 ** 9, 30.0, 10.0), (7, -5.0, 4.0), (1, 0.0, 0.0)])
def test_model_obeys_the_rules(lib, error_freq, mu, sigma):
    rng = np.random.default_rng(11)
    recs, text = small_fasta(rng)
    L = 20
    lower, table = host.generate_inner_table(mu, sigma, lib=lib)
    P = gm.Provider(text, "small.fa", error_freq, L, 1, lower, table)
    assert [(n, s) for n, s in P.seqs] == [(h.split()[0], s) for h, s in recs]        # the FASTA as the library reads it
    res = gm.generate([P], seed=5, first_pair=0, n_pairs=1500)
    one, two = gm.parse_fastq(res.one), gm.parse_fastq(res.two)
    assert len(one) == len(two) == 1500 and res.failed_pair is None
    seqs = dict(P.seqs)
    comp = bytes(gm.COMPLEMENT)
    subs = total = 0
    seen = set()
    for i, ((n1, b1, q1), (n2, b2, q2)) in enumerate(zip(one, two)):
        prefix, name, start, number = n1[:-2].split(b":")[0:2], n1.split(b":")[2], int(n1.split(b":")[3]), n1.split(b":")[4]
        assert prefix == [b"ngs", b"small.fa"] and number == b"%d/1" % (i + 1) and n2 == n1[:-1] + b"2"
        assert q1 == q2 == b"J" * L and len(b1) == len(b2) == L
        ref = seqs[name]
        seen.add(name)
        flen = res.picks[i][3]
        assert start >= 1 and res.picks[i][2] == start                                 # no start is 0
        assert lower <= flen - 2 * L <= lower + len(table) - 1
        frag = ref[start - 1:start - 1 + flen]
        assert len(frag) == flen >= L                                                  # every fragment ends within its sequence
        assert set(frag) <= set(b"ACGTacgt")                                           # no fragment touches another byte
        want1, want2 = frag[:L], frag[::-1].translate(comp)[:L]
        for got, want in ((b1, want1), (b2, want2)):
            for g, w in zip(got, want):
                total += 1
                if g != w:                                                             # a substituted base: one of ACGT that differs
                    subs += 1
                    assert g in b"ACGT"
            if error_freq == 1:
                assert all(g != w for g, w in zip(got, want))
            if error_freq == 10 ** 9:
                assert got == want                                                     # (case kept: lower case stays lower case)
    assert b"tiny" not in seen and seen == {b"chrA", b"chrB", b"chrC"}                 # 41 < 2 L + 2; the others by length
    if error_freq == 7:
        assert abs(subs - total / 7) < 5 * math.sqrt(total * (1 / 7) * (6 / 7))
    assert res.rejected["base"] > 0                                                    # the N runs were met and stepped over


def test_model_draws_are_a_pure_function_of_the_pair(lib):
    rng = np.random.default_rng(12)
    _, text = small_fasta(rng)
    lower, table = host.generate_inner_table(10.0, 3.0, lib=lib)
    P = gm.Provider(text, "s.fa", 5, 20, 1, lower, table)
    whole = gm.generate([P], 9, 0, 300)
    a, b = gm.generate([P], 9, 0, 120), gm.generate([P], 9, 120, 180)
    assert a.one + b.one == whole.one and a.two + b.two == whole.two
    assert gm.generate([P], 10, 0, 300).one != whole.one
    for args in ((1, 2, 3, 4), (0, 0, 0, 0), (2 ** 64 - 1, 2 ** 56, 7, 2 ** 24)):
        assert lib.ngsq_generate_draw(*args) == gm.draw(gm.pair_key(args[0], args[1]), args[2], args[3])


# ---- the inner-distance table against math.erf ---------------------------------------------------------------------------------
def phi(x):
    return 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))


@pytest.mark.parametrize("mu,sigma,lower,upper", [
    (50.0, 10.0, 20, 80),
    (10.3, 2.2, 4, 17),            # floor(6.6) = 6, ceil(6.6) = 7, trunc(4.3) = 4, trunc(17.3) = 17: the three differ
    (-10.3, 2.2, -16, -3),         # negative mu: trunc(-16.3) = -16 (towards zero), trunc(-3.3) = -3
    (-0.5, 0.3, 0, 0),             # trunc(-0.5) = -0 and trunc(0.5) = 0: one entry
    (0.0, 1.0, -3, 3),
])
def test_inner_table_is_the_clamped_rounded_normal(lib, mu, sigma, lower, upper):
    lo, table = host.generate_inner_table(mu, sigma, lib=lib)
    assert lo == lower and len(table) == upper - lower + 1
    t = [int(x) for x in table]
    assert t[-1] == 2 ** 64 - 1 and all(a <= b for a, b in zip(t, t[1:]))
    for j, x in enumerate(t[:-1]):
        # P(round(X) <= lower + j) = P(X < lower + j + 0.5); the lower tail is folded onto entry 0, the upper one onto the last
        assert abs(x / 2.0 ** 64 - phi((lower + j + 0.5 - mu) / sigma)) < 1e-12, j
    # tail folding: entry 0 holds everything below lower + 0.5, the last everything above upper - 0.5
    if len(t) > 1:
        assert abs(t[0] / 2.0 ** 64 - phi((lower + 0.5 - mu) / sigma)) < 1e-12
        assert abs(1 - t[-2] / 2.0 ** 64 - (1 - phi((upper - 0.5 - mu) / sigma))) < 1e-12


def test_inner_table_of_sigma_zero_and_refusals(lib):
    for mu, want in ((7.0, 7), (2.7, 2), (-2.7, -2), (0.0, 0)):                        # round(mu) clamped to [trunc(mu), trunc(mu)]
        lo, table = host.generate_inner_table(mu, 0.0, lib=lib)
        assert lo == want and [int(x) for x in table] == [2 ** 64 - 1]
    for mu, sigma in ((0.0, -1.0), (0.0, math.nan), (0.0, math.inf), (math.nan, 1.0), (math.inf, 1.0)):
        with pytest.raises(host.NgsqError):
            host.generate_inner_table(mu, sigma, lib=lib)
    with pytest.raises(host.NgsqError) as e:
        host.generate_inner_table(0.0, 1e6, lib=lib)                                   # 6 * 10^6 entries
    assert e.value.code == ffi.ERR_LIMIT
    lo, table = host.generate_inner_table(0.0, 174762.0, lib=lib)                      # 2 * 524286 + 1 entries: inside the limit
    assert len(table) == 2 * 524286 + 1 <= ffi.GENERATE_MAX_TABLE


# ---- the host side of a generator ----------------------------------------------------------------------------------------------
def test_open_counts_the_bases_of_every_record_on_the_host(lib, tmp_path):
    rng = np.random.default_rng(13)
    recs, text = small_fasta(rng)
    text += b">empty\n>cr_inside\nAC\rGT\r\n>last_without_newline\nACGT\r"               # a '\r' inside a line stays a byte
    path = str(tmp_path / "h.fa")
    open(path, "wb").write(text)
    with host.Generator([(path, 100, 0.0, 0.0, 20, 1)], lib=lib) as g:
        got = g.sequences()
        want = [(n, len(s)) for n, s in gm.parse_fasta(text)]
        assert got == want and want[-3:] == [(b"empty", 0), (b"cr_inside", 5), (b"last_without_newline", 4)]
        total = sum(n for _, n in want)
        assert g.reads_for_coverage(3) == 3 * (total // 20)
        assert g.reads_for_coverage(0) == 0


def provider_refusals(d):
    fa = os.path.join(d, "r.fa")
    return [
        ([(fa, 0, 0.0, 0.0, 20, 1)], "error frequency must be at least 1"),
        ([(fa, 2 ** 32, 0.0, 0.0, 20, 1)], "error frequency must be below 2^32"),
        ([(fa, 5, 0.0, -1.0, 20, 1)], "std deviation of the inner distance distribution must be finite and not negative"),
        ([(fa, 5, 0.0, math.inf, 20, 1)], "std deviation of the inner distance distribution must be finite and not negative"),
        ([(fa, 5, math.nan, 1.0, 20, 1)], "mean of the inner distance distribution must be finite"),
        ([(fa, 5, 0.0, 0.0, 0, 1)], "read length must be at least 1"),
        ([(fa, 5, -21.0, 0.0, 20, 1)], "fragment is too short for the specified read length"),
        ([(fa, 5, -15.0, 2.0, 20, 1)], "fragment is too short for the specified read length"),      # -15 - 6 < -20
        ([(fa, 5, 0.0, 0.0, 20, 0)], "every reference provider has a weight of 0"),
        ([(fa, 5, 0.0, 0.0, 20, 0), (fa, 5, 0.0, 0.0, 20, 0)], "every reference provider has a weight of 0"),
        ([(fa, 5, 0.0, 0.0, 150, 1)], "r.fa: no sequence holds the 302 bases"),                       # the longest has 301
        ([(fa, 5, 0.0, 0.0, 20, 1), (fa, 5, 0.0, 0.0, 150, 0)], "r.fa: no sequence holds the 302 bases"),
        ([(os.path.join(d, "dup.fa"), 5, 0.0, 0.0, 20, 1)], "dup.fa: the sequence name chr1 stands in front of more than one record"),
        ([(os.path.join(d, "missing.fa"), 5, 0.0, 0.0, 20, 1)], "No such file or directory (os error 2)"),
    ]


@pytest.fixture(scope="module")
def refusal_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("refuse"))
    rng = np.random.default_rng(14)
    open(os.path.join(d, "r.fa"), "wb").write(gm.fasta_text([(b"chr1", gm.random_letters(rng, 301)), (b"chr2", gm.random_letters(rng, 100))]))
    open(os.path.join(d, "dup.fa"), "wb").write(gm.fasta_text([(b"chr1 a", gm.random_letters(rng, 100)), (b"chr1 b", gm.random_letters(rng, 100))]))
    return d


def test_open_refuses_up_front(lib, refusal_dir):
    for provs, msg in provider_refusals(refusal_dir):
        with pytest.raises(host.NgsqError) as e:
            host.Generator(provs, lib=lib)
        assert msg in str(e.value), (provs, str(e.value))
    with host.Generator([(os.path.join(refusal_dir, "r.fa"), 5, -20.0, 0.0, 20, 0), (os.path.join(refusal_dir, "r.fa"), 5, 0.0, 0.0, 149, 3)], lib=lib) as g:
        assert g.sequences(1) == [(b"chr1", 301), (b"chr2", 100)]                      # 301 >= 2 * 149 + 2: eligible, just


def test_gzip_pipe_gives_members_any_reader_joins(lib, tmp_path):
    rng = np.random.default_rng(15)
    for n in (0, 1, (1 << 20) - 1, 1 << 20, (3 << 20) + 12345):
        data = np.frombuffer(b"ACGTJ\n", dtype=np.uint8)[rng.integers(0, 6, n)].tobytes()
        path = str(tmp_path / f"p{n}.gz")
        fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
        p, wfd = ffi.C.c_void_p(), ffi.C.c_int()
        assert lib.ngsq_gzip_pipe_open(fd, 3, ffi.C.byref(p), ffi.C.byref(wfd)) == 0
        with os.fdopen(wfd.value, "wb", closefd=True) as f:
            for k in range(0, n, 700001):
                f.write(data[k:k + 700001])
        assert lib.ngsq_gzip_pipe_close(p) == 0
        os.close(fd)
        raw = open(path, "rb").read()
        assert raw[:2] == b"\x1f\x8b" and gzip.decompress(raw) == data
        assert raw.count(b"\x1f\x8b\x08") >= max(1, -(-n >> 20)) - 0                    # a member per piece of at most 1 MiB
    fd = os.open("/dev/full", os.O_WRONLY)
    p, wfd = ffi.C.c_void_p(), ffi.C.c_int()
    assert lib.ngsq_gzip_pipe_open(fd, 2, ffi.C.byref(p), ffi.C.byref(wfd)) == 0
    os.write(wfd.value, b"x" * 100000)
    os.close(wfd.value)
    assert lib.ngsq_gzip_pipe_close(p) == 28                                           # ENOSPC, reported, not lost
    os.close(fd)


# ---- the command line ------------------------------------------------------------------------------------------------------------
PARSE = "parsing reference providers: "
WIKI = "invalid format for reference genome sequence provider, please check the wiki for the correct format."


def cli_refusals(d):
    fa = os.path.join(d, "r.fa")
    ok = fa + ":100:10:2:20:1"
    o1, o2 = os.path.join(d, "o_1.fastq"), os.path.join(d, "o_2.fq.gz")
    n = ["-n", "5"]
    return [
        # the record count
        ([o1, o2, ok], "the following required arguments were not provided: <--num-records <USIZE>|--coverage <USIZE>>"),
        (["-n", "5", "-c", "2", o1, o2, ok], "the argument '--num-records <USIZE>' cannot be used with '--coverage <USIZE>'"),
        (["--coverage", "2", "--num-records", "5", o1, o2, ok], "the argument '--num-records <USIZE>' cannot be used with '--coverage <USIZE>'"),
        (["-n", "x", o1, o2, ok], "invalid value 'x' for '--num-records <USIZE>': invalid digit found in string"),
        (["-n", "-1", o1, o2, ok], "invalid value '-1' for '--num-records <USIZE>': invalid digit found in string"),
        (["-c", "1.5", o1, o2, ok], "invalid value '1.5' for '--coverage <USIZE>': invalid digit found in string"),
        ([o1, o2, ok, "-n"], "a value is required for '--num-records <USIZE>' but none was supplied"),
        # the positionals
        (n, "the following required arguments were not provided: <READ_ONES_FILE> <READ_TWOS_FILE> <REFERENCE_PROVIDERS>..."),
        (n + [o1], "the following required arguments were not provided: <READ_TWOS_FILE> <REFERENCE_PROVIDERS>..."),
        (n + [o1, o2], "the following required arguments were not provided: <REFERENCE_PROVIDERS>..."),
        (n + ["--nope", o1, o2, ok], "unexpected argument '--nope' found"),
        # --error-rate
        (n + ["-e", "abc", o1, o2, ok], "invalid value 'abc' for '--error-rate <F32>': abc isn't a float"),
        (n + ["--error-rate", "", o1, o2, ok], "invalid value '' for '--error-rate <F32>':  isn't a float"),
        (n + ["-e", "1.5", o1, o2, ok], "invalid value '1.5' for '--error-rate <F32>': Error rate must be between 0.0 and 1.0"),
        (n + ["-e", "-0.1", o1, o2, ok], "invalid value '-0.1' for '--error-rate <F32>': Error rate must be between 0.0 and 1.0"),
        (n + ["-e", "nan", o1, o2, ok], "invalid value 'nan' for '--error-rate <F32>': Error rate must be between 0.0 and 1.0"),
        # the seven messages of a provider string
        (n + [o1, o2, fa + ":100:10:2:20"], PARSE + WIKI),
        (n + [o1, o2, fa + ":100:10:2:20:1:9"], PARSE + WIKI),
        (n + [o1, o2, fa], PARSE + WIKI),
        (n + [o1, o2, fa + ":x:10:2:20:1"], PARSE + f"could not parse the error frequency for reference provider: {fa}:x:10:2:20:1."),
        (n + [o1, o2, fa + ":100:m:2:20:1"], PARSE + f"could not parse the mean for inner distance distribution for reference provider: {fa}:100:m:2:20:1."),
        (n + [o1, o2, fa + ":100:10::20:1"], PARSE + f"could not parse the std deviation for inner distance distribution for reference provider: {fa}:100:10::20:1."),
        (n + [o1, o2, fa + ":100:10:2:-20:1"], PARSE + f"could not parse the read length for reference provider: {fa}:100:10:2:-20:1."),
        (n + [o1, o2, fa + ":100:10:2:20:1.0"], PARSE + f"could not parse the weight for reference provider: {fa}:100:10:2:20:1.0."),
        (n + [o1, o2, ok, fa + ":100:10:2:20:w"], PARSE + f"could not parse the weight for reference provider: {fa}:100:10:2:20:w."),
        # the FASTA's own errors
        (n + [o1, o2, os.path.join(d, "missing.fa") + ":100:10:2:20:1"], PARSE + "No such file or directory (os error 2)"),
        (n + [o1, o2, os.path.join(d, "r.fa.gz") + ":100:10:2:20:1"], PARSE + "This command does not yet support gzipped FASTA files. Please unzip your FASTA file and try again."),
        (n + [o1, o2, os.path.join(d, "r.bam") + ":100:10:2:20:1"], PARSE + "incompatible formats: required FASTA, found BAM"),
        (n + [o1, o2, os.path.join(d, "r.txt") + ":100:10:2:20:1"], PARSE + "Not able to determine filetype for extension: txt"),
        # the up-front refusals of the rules
        (n + [o1, o2, fa + ":100:10:2:20:0"], PARSE + "every reference provider has a weight of 0"),
        (n + [o1, o2, fa + ":100:10:2:150:1"], PARSE + "r.fa: no sequence holds the 302 bases"),
        (n + [o1, o2, fa + ":100:-21:0:20:1"], "fragment is too short for the specified read length"),
        (n + [o1, o2, fa + ":0:10:2:20:1"], "error frequency must be at least 1"),
        (n + [o1, o2, fa + ":100:10:-2:20:1"], "std deviation of the inner distance distribution must be finite and not negative"),
        (n + [o1, o2, fa + ":100:10:inf:20:1"], "std deviation of the inner distance distribution must be finite and not negative"),
        (n + [o1, o2, os.path.join(d, "dup.fa") + ":100:10:2:20:1"], PARSE + "dup.fa: the sequence name chr1 stands in front of more than one record"),
        # the outputs: read ones first
        (n + [os.path.join(d, "o.bam"), o2, ok], f"opening reads one file: {os.path.join(d, 'o.bam')}: incompatible formats: required FASTQ, found BAM"),
        (n + [os.path.join(d, "o.fa.gz"), o2, ok], f"opening reads one file: {os.path.join(d, 'o.fa.gz')}: incompatible formats: required FASTQ, found Gzipped FASTA"),
        (n + [os.path.join(d, "o.txt"), os.path.join(d, "p.txt"), ok], f"opening reads one file: {os.path.join(d, 'o.txt')}: Not able to determine filetype for extension: txt"),
        (n + [os.path.join(d, "o.txt.gz"), o2, ok], f"opening reads one file: {os.path.join(d, 'o.txt.gz')}: Not able to determine filetype for extension: gz"),
        (n + [os.path.join(d, "no", "o.fq"), o2, ok], f"opening reads one file: {os.path.join(d, 'no', 'o.fq')}: No such file or directory (os error 2)"),
    ]


def test_every_refusal_prints_its_message_and_creates_no_file(ngs, refusal_dir):
    before = sorted(os.listdir(refusal_dir))
    for args, msg in cli_refusals(refusal_dir):
        r = run(ngs, "generate", *args)
        assert r.returncode == 1, (args, r.stderr)
        assert b"Error: " in r.stderr and msg.encode() in r.stderr, (args, r.stderr)
        assert r.stdout == b"" and sorted(os.listdir(refusal_dir)) == before, args


def test_second_output_is_refused_after_the_first_is_created(ngs, refusal_dir, tmp_path):
    o1, o2 = str(tmp_path / "a.fastq"), str(tmp_path / "b.sam")
    r = run(ngs, "generate", "-n", "5", o1, o2, os.path.join(refusal_dir, "r.fa") + ":100:10:2:20:1")
    assert r.returncode == 1 and f"Error: opening reads two file: {o2}: incompatible formats: required FASTQ, found SAM".encode() in r.stderr
    assert os.path.exists(o1) and not os.path.exists(o2)                               # read ones first, as the reference opens them


def test_zero_records_need_no_device(ngs, refusal_dir, tmp_path):
    """-n 0 writes two empty files, or two empty gzip streams, and says so at info level; -q says nothing."""
    o1, o2 = str(tmp_path / "z_1.fq"), str(tmp_path / "z_2.fastq.gz")
    r = run(ngs, "generate", "--num-records", "0", "--seed", "1", o1, o2, os.path.join(refusal_dir, "r.fa") + ":100:10:2:20:1")
    assert r.returncode == 0, r.stderr
    assert open(o1, "rb").read() == b"" and gzip.decompress(open(o2, "rb").read()) == b"" and os.path.getsize(o2) > 0
    assert b"Starting generate command..." in r.stderr and b"Generating 0 reads..." in r.stderr
    r = run(ngs, "-q", "generate", "-n", "0", o1, o2, os.path.join(refusal_dir, "r.fa") + ":100:10:2:20:1")
    assert r.returncode == 0 and r.stderr == b""
    r = run(ngs, "generate", "-c", "0", o1, o2, os.path.join(refusal_dir, "r.fa") + ":100:10:2:20:1")
    assert r.returncode == 0 and b"Generating 0 reads..." in r.stderr and b"Seed: " in r.stderr     # without --seed the seed is logged


def test_records_need_the_device_after_the_files(ngs, lib, refusal_dir, tmp_path):
    """The device is acquired last: on a box without one, exit 1 with both files created (with one, the pairs)."""
    o1, o2 = str(tmp_path / "d_1.fq"), str(tmp_path / "d_2.fq")
    r = run(ngs, "generate", "-c", "2", "--seed", "3", o1, o2, os.path.join(refusal_dir, "r.fa") + ":100:10:2:20:1")
    assert b"Generating 40 reads..." in r.stderr                                       # 2 * (401 / 20)
    assert os.path.exists(o1) and os.path.exists(o2)
    if lib.ngsq_device_count() > 0:
        assert r.returncode == 0 and open(o1, "rb").read().count(b"\n") == 160
    else:
        assert r.returncode == 1 and b"Error: " in r.stderr


def test_help_lists_the_command(ngs):
    r = run(ngs, "generate", "--help")
    assert r.returncode == 0
    h = (r.stderr + r.stdout).decode()
    for s in ("<READ_ONES_FILE>", "<READ_TWOS_FILE>", "<REFERENCE_PROVIDERS>...", "-e, --error-rate <F32>", "[default: 0.0001]", "unused",
              "-n, --num-records <USIZE>", "-c, --coverage <USIZE>", "--seed <U64>", "--device <N>", "--batch-pairs <N>",
              "PATH:ERROR_FREQ:MU:SIGMA:READ_LENGTH:WEIGHT"):
        assert s in h, s
    r = run(ngs, "--help")
    assert b"generate" in r.stderr + r.stdout
    r = run(ngs, "nosuchcommand")
    assert r.returncode == 1 and b"`generate`" in r.stderr


def test_library_refuses_bad_arguments(lib, refusal_dir):
    g = ffi.C.c_void_p()
    assert lib.ngsq_generate_open(None, 1, ffi.C.byref(g)) != 0
    arr = (ffi.GenerateProvider * 1)()
    assert lib.ngsq_generate_open(arr, 0, ffi.C.byref(g)) != 0
    assert lib.ngsq_generate_open(arr, 1, ffi.C.byref(g)) != 0                         # no path
    with host.Generator([(os.path.join(refusal_dir, "r.fa"), 5, 0.0, 0.0, 20, 1)], lib=lib) as gen:
        assert lib.ngsq_generate_write(gen._g, 1, 2, 0, 0, 1, 0, None) == ffi.ERR_STATE       # not on a device yet
        assert b"ngsq_generate_load was not called" in lib.ngsq_generate_last_error()
        assert lib.ngsq_generate_write(gen._g, -1, 2, 0, 0, 1, 0, None) != 0
        assert lib.ngsq_generate_load(gen._g, None) != 0
    lib.ngsq_generate_close(None)


# ---- the parser and the table builder under the sanitizers -----------------------------------------------------------------------
def test_provider_parser_and_table_builder_on_hostile_input_under_sanitizers(tmp_path):
    """tests/c/generate_args_drive.c: empty parts, 5 and 7 parts, overflowing integers, nan, inf, a huge sigma, a table at the
    limit, buffers too small.  The code under test and the driver are compiled with -fsanitize=address,undefined into one
    program that runs here, on the CPU."""
    src = os.path.join(ROOT, "ngs_amd", "csrc", "generate_args.cpp")
    drv = os.path.join(ROOT, "tests", "c", "generate_args_drive.c")
    o1, o2, exe = str(tmp_path / "ga.o"), str(tmp_path / "drive.o"), str(tmp_path / "generate_args_drive")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-c", src, "-o", o1], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", *SAN, "-c", drv, "-o", o2], check=True)
    subprocess.run(["g++", *SAN, o1, o2, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["parse", "ok", "check", "ok", "table", "ok"]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
