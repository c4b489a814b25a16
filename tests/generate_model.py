"""A restatement of `ngs generate` for the tests: the rules of one read pair as the reference has them
(src/generate/providers/reference_provider.rs:291-393, src/generate/providers.rs:29-48) with this build's decisions, over this
build's draw function.  The choices of a pair are made one pair at a time with Python integers; the per-base substitution draws,
which are many, are the same arithmetic on numpy arrays.  The inner-distance tables are the library's (they come from erf in
double; tests/test_generate.py holds them to math.erf), everything else is computed here.

    providers: [Provider(fasta_bytes, file_name, error_freq, read_length, weight, lower, table)]
    generate(providers, seed, first_pair, n_pairs) -> Result(one, two, picks, rejected)
"""
from __future__ import annotations

import bisect
import re
from dataclasses import dataclass, field
from typing import List, Sequence, Tuple

import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
PROVIDER, SEQUENCE, START, INNER, HIT_ONE, BASE_ONE, HIT_TWO, BASE_TWO = range(8)
MAX_ATTEMPTS = 1024


# ---- the draws ---------------------------------------------------------------------------------------------------------------
def mix(z: int) -> int:
    """the splitmix64 finaliser"""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def pair_key(seed: int, pair: int) -> int:
    return mix(seed ^ mix((pair + GOLDEN) & M64))


def draw(key: int, purpose: int, index: int) -> int:
    return mix((key + GOLDEN * (((purpose << 32) | index) + 1)) & M64)


def below(u: int, n: int) -> int:
    """an integer in [0, n): the high half of u * n"""
    return (u * n) >> 64


def mix_np(z: np.ndarray) -> np.ndarray:
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draw_np(keys: np.ndarray, purpose: int, n_index: int) -> np.ndarray:
    """draw(key, purpose, j) for every key and j < n_index: [len(keys), n_index]"""
    with np.errstate(over="ignore"):
        idx = (np.uint64(purpose << 32) | np.arange(n_index, dtype=np.uint64)) + np.uint64(1)
        return mix_np(keys[:, None] + np.uint64(GOLDEN) * idx[None, :])


# ---- the FASTA ---------------------------------------------------------------------------------------------------------------
def parse_fasta(data: bytes) -> List[Tuple[bytes, bytes]]:
    """[(name, letters)] in file order: a record starts at a line whose first byte is '>', its name is the text up to the first
    blank, its sequence every byte of the following lines without the line terminators ("\\n", "\\r\\n", a final "\\r")."""
    out = []
    starts = [m.start() for m in re.finditer(rb"(?m)^>", data)]
    for k, s in enumerate(starts):
        end = starts[k + 1] if k + 1 < len(starts) else len(data)
        nl = data.find(b"\n", s, end)
        head = data[s + 1:nl if nl >= 0 else end]
        text = data[nl + 1:end] if nl >= 0 else b""
        name = re.split(rb"[ \t\r]", head, maxsplit=1)[0]
        if text.endswith(b"\r"):
            text = text[:-1]
        out.append((name, text.replace(b"\r\n", b"").replace(b"\n", b"")))
    return out


@dataclass
class Provider:
    fasta: bytes
    file_name: str
    error_freq: int
    read_length: int
    weight: int
    lower: int
    table: Sequence[int]                     # ngsq_generate_inner_table: cumulative thresholds, the last 2^64 - 1
    seqs: List[Tuple[bytes, bytes]] = field(default_factory=list)

    def __post_init__(self):
        self.seqs = parse_fasta(self.fasta)
        self.table = [int(t) for t in self.table]
        L = self.read_length
        self.cum = [0]
        for _, s in self.seqs:                                            # eligible: len >= 2 L + 2
            self.cum.append(self.cum[-1] + (len(s) if len(s) >= 2 * L + 2 else 0))
        self.arr = [np.frombuffer(s, dtype=np.uint8) for _, s in self.seqs]
        ok = np.zeros(256, dtype=bool)
        ok[list(b"ACGTacgt")] = True
        self.bad_before = [np.concatenate([[0], np.cumsum(~ok[a])]) for a in self.arr]   # bytes outside ACGTacgt in front of i


COMPLEMENT = np.arange(256, dtype=np.uint8)
for a, b in zip(b"ACGTacgt", b"TGCAtgca"):
    COMPLEMENT[a] = b


@dataclass
class Result:
    one: bytes
    two: bytes
    picks: list                               # (provider, sequence, start, fragment length) per pair
    rejected: dict                            # attempts rejected by cause: start, end, base
    failed_pair: int | None = None            # the first pair without a fragment after MAX_ATTEMPTS (nothing is returned behind it)


def pick_pair(providers: Sequence[Provider], seed: int, pair: int, rejected: dict):
    key = pair_key(seed, pair)
    total_w = sum(p.weight for p in providers)
    x = below(draw(key, PROVIDER, 0), total_w)
    pi, end = 0, 0
    for pi, p in enumerate(providers):                                    # a weight of 0 is never chosen
        end += p.weight
        if end > x:
            break
    P = providers[pi]
    L = P.read_length
    for a in range(MAX_ATTEMPTS):
        xs = below(draw(key, SEQUENCE, a), P.cum[-1])
        s = bisect.bisect_right(P.cum, xs) - 1                            # cum[s] <= xs < cum[s + 1]: an eligible sequence
        n = len(P.seqs[s][1])
        start = below(draw(key, START, a), n - 2 * L)
        u = draw(key, INNER, a)
        j = bisect.bisect_right(P.table, u, 0, len(P.table) - 1)          # the entries in front of the last that are <= u
        flen = 2 * L + P.lower + j
        if start == 0:                                                    # Position is 1-based
            rejected["start"] += 1
            continue
        if start - 1 + flen > n:                                          # chr.get(start..end) is None
            rejected["end"] += 1
            continue
        if P.bad_before[s][start - 1 + flen] - P.bad_before[s][start - 1]:  # reverse_compliment is None
            rejected["base"] += 1
            continue
        return pi, s, start, flen
    return None


def substitute(reads: np.ndarray, keys: np.ndarray, hit: int, base: int, error_freq: int) -> np.ndarray:
    """providers.rs:29-48 on every base of every read: with probability 1 / error_freq one of A C G T that differs from it."""
    out = reads.copy()
    hits = draw_np(keys, hit, reads.shape[1]) <= np.uint64(M64 // error_freq)     # below(u, E) == 0  <=>  u * E < 2^64
    for r, j in zip(*np.nonzero(hits)):
        c = int(reads[r, j])
        v = draw(int(keys[r]), base, int(j))
        ci = b"ACGT".find(bytes([c]))
        if ci >= 0:
            k = below(v, 3)
            k += k >= ci
        else:                                                             # lower case: all four differ
            k = below(v, 4)
        out[r, j] = b"ACGT"[k]
    return out


def generate(providers: Sequence[Provider], seed: int, first_pair: int, n_pairs: int) -> Result:
    rejected = {"start": 0, "end": 0, "base": 0}
    picks, failed = [], None
    for i in range(n_pairs):
        pk = pick_pair(providers, seed, first_pair + i, rejected)
        if pk is None:
            failed = first_pair + i
            break
        picks.append(pk)
    n = len(picks)
    bases_one: list = [None] * n
    bases_two: list = [None] * n
    for pi, P in enumerate(providers):
        rows = [i for i in range(n) if picks[i][0] == pi]
        if not rows:
            continue
        L = P.read_length
        flat = np.concatenate(P.arr) if P.arr else np.zeros(0, np.uint8)
        off = np.concatenate([[0], np.cumsum([len(a) for a in P.arr])]).astype(np.int64)
        first = np.array([off[picks[i][1]] + picks[i][2] - 1 for i in rows], dtype=np.int64)
        last = first + np.array([picks[i][3] - 1 for i in rows], dtype=np.int64)
        j = np.arange(L, dtype=np.int64)
        keys = np.array([pair_key(seed, first_pair + i) for i in rows], dtype=np.uint64)
        one = substitute(flat[first[:, None] + j[None, :]], keys, HIT_ONE, BASE_ONE, P.error_freq)
        two = substitute(COMPLEMENT[flat[last[:, None] - j[None, :]]], keys, HIT_TWO, BASE_TWO, P.error_freq)
        for r, i in enumerate(rows):
            bases_one[i], bases_two[i] = one[r].tobytes(), two[r].tobytes()
    out = ([], [])
    for i, (pi, s, start, _) in enumerate(picks):
        P = providers[pi]
        name = b"@ngs:" + P.file_name.encode() + b":" + P.seqs[s][0] + b":" + str(start).encode() + b":" + str(first_pair + i + 1).encode()
        tail = b"\n+\n" + b"J" * P.read_length + b"\n"
        out[0].append(name + b"/1\n" + bases_one[i] + tail)
        out[1].append(name + b"/2\n" + bases_two[i] + tail)
    return Result(b"".join(out[0]), b"".join(out[1]), picks, rejected, failed)


# ---- what the tests of both files share -----------------------------------------------------------------------------------------
def model_provider(spec, lib) -> Provider:
    """The model's provider for a host.Generator provider tuple (path, error_freq, mu, sigma, read_length, weight): the file's
    bytes, its file name, the library's inner-distance table."""
    import os

    from ngs_amd import host
    path, error_freq, mu, sigma, read_length, weight = spec
    lower, table = host.generate_inner_table(mu, sigma, lib=lib)
    return Provider(open(path, "rb").read(), os.path.basename(path), error_freq, read_length, weight, lower, table)


def fasta_text(records, width=60, eol=b"\n") -> bytes:
    """records: [(definition line without '>', letters)] as FASTA text of `width` letters a line."""
    out = []
    for head, seq in records:
        out.append(b">" + head + eol)
        out.extend(seq[k:k + width] + eol for k in range(0, len(seq), width))
    return b"".join(out)


def random_letters(rng, n, lower=(), n_runs=()) -> bytes:
    """n random letters of ACGT; [a, b) of `lower` in lower case; [a, b) of n_runs as N."""
    a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
    for lo, hi in lower:
        a[lo:hi] |= 0x20
    for lo, hi in n_runs:
        a[lo:hi] = ord("N")
    return a.tobytes()


def parse_fastq(data: bytes):
    """[(name, bases, quality)] of FASTQ text whose records are four lines each."""
    lines = data.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    out = []
    for k in range(0, len(lines) - 1, 4):
        assert lines[k].startswith(b"@") and lines[k + 2] == b"+", lines[k:k + 4]
        out.append((lines[k][1:], lines[k + 1], lines[k + 3]))
    return out
