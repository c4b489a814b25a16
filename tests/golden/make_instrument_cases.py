#!/usr/bin/env python3
"""Record what the reference's two lookup tables of `ngs derive instrument` answer for a list of query strings, as a fixture
(tests/golden/instrument_cases.json).  The tables (src/derive/instrument/instruments.rs, flowcells.rs) map anchored patterns
to machine names; possible_instruments_for_query (compute.rs:103-119) returns the union of the machines of every pattern
that matches.  This script reads the tables at generation time, makes queries around every pattern -- matching ones at every
length the pattern allows, and near misses: one character short or long, lower case, a trailing character, a trailing
newline, a leading character, the prefix alone, the comma inside a class, a prefix-only pattern with a tail -- and
evaluates them.  The fixture holds the queries and the machine names each yields: recorded results, no pattern and no
text of the reference.  tests/test_derive.py holds the library's own restatement of the tables to it.

    python tests/golden/make_instrument_cases.py <reference checkout> tests/golden/instrument_cases.json
"""
import itertools
import json
import os
import re
import sys

TABLES = {"instruments": "src/derive/instrument/instruments.rs", "flowcells": "src/derive/instrument/flowcells.rs"}


def read_table(path):
    """[(pattern, [machine, ...])] of one table; commented-out entries are not part of it."""
    src = "\n".join(line for line in open(path).read().splitlines() if not line.lstrip().startswith("//"))
    out = []
    for m in re.finditer(r'"(\^[^"]*)"\s*,\s*HashSet::from\(\[([^\]]*)\]\)', src, re.S):
        out.append((m.group(1), re.findall(r'"([^"]*)"', m.group(2))))
    assert out, path
    return out


def matcher(pattern):
    """Rust's regex crate without flags: ^ is the start and $ the END of the text (Python's $ also matches in front of a
    final newline: \\Z does not); a pattern without $ matches any text that starts with it."""
    return re.compile(pattern.replace("$", r"\Z"))


def evaluate(table, query):
    got = set()
    for pattern, machines in table:
        if matcher(pattern).match(query):
            got |= set(machines)
    return sorted(got)


TOKEN = re.compile(r"\[(?P<cls>[^\]]+)\](?:\{(?P<lo>\d+)(?:,(?P<hi>\d+))?\})?|\((?P<grp>[^)]*)\)\?|(?P<end>\$)|(?P<start>\^)|(?P<lit>.)")


def class_samples(cls):
    """A few members of a character class, every kind of member it names among them."""
    out = []
    for m in re.finditer(r"(.)-(.)|(.)", cls):
        if m.group(1):
            a, b = ord(m.group(1)), ord(m.group(2))
            out += [chr(a), chr((a + b) // 2), chr(b)]
        else:
            out.append(m.group(3))
    return out


def expansions(pattern):
    """Matching strings of the pattern: every allowed count of every counted class, an optional group present and absent;
    and the pattern's literal prefix."""
    parts, prefix, in_prefix = [], "", True
    for m in TOKEN.finditer(pattern):
        if m.group("start") or m.group("end"):
            continue
        if m.group("lit") is not None:
            parts.append([m.group("lit")])
            if in_prefix:
                prefix += m.group("lit")
            continue
        in_prefix = False
        if m.group("cls"):
            lo = int(m.group("lo") or 1)
            hi = int(m.group("hi") or lo)
            s = class_samples(m.group("cls"))
            parts.append(["".join(s[(k + j) % len(s)] for j in range(n)) for n in range(lo, hi + 1) for k in range(len(s))])
        else:
            inner = [e for e in expansions(m.group("grp"))[0]]
            parts.append([""] + inner[:2])
    out = ["".join(c) for c in itertools.islice(itertools.product(*parts), 400)]
    return out, prefix


def queries_around(pattern):
    full, prefix = expansions(pattern)
    # (the first and the last expansion of every length, so that the list stays short)
    by_len = {}
    for s in full:
        by_len.setdefault(len(s), []).append(s)
    keep = []
    for n in sorted(by_len):
        keep += [by_len[n][0], by_len[n][-1]]
    out = []
    for s in dict.fromkeys(keep):
        out += [s, s[:-1], s + s[-1], s + "0", s + "X", s + "\n", s.lower(), "x" + s, s[1:], s[:len(prefix)] + s[len(prefix) + 1:],
                s[:len(prefix)] + "0" + s[len(prefix):], s[:len(prefix)] + "a" + s[len(prefix) + 1:], s + "_123456789", s + "_12345678",
                s + "_1234567890", s + "_12345678a", s[:-1] + ",", s[:-1] + "-", s[:-1] + "a", s + ":tail"]
    out += [prefix, prefix + " and a tail", prefix.lower(), ""]
    return out


def main(reference, out_path):
    tables = {name: read_table(os.path.join(reference, rel)) for name, rel in TABLES.items()}
    queries = ["NoMatchingName", "A00000", "H00000RXX", "D00000", "B0000", "K00000", "H0000ADXX", "QQQQQ", "ZZZZZZ", "A00741", "HG7WKDSXX", "HWI-D00000"]
    for table in tables.values():
        for pattern, _ in table:
            queries += queries_around(pattern)
    queries = list(dict.fromkeys(queries))
    doc = {"description": "queries and the machine names the reference's instrument and flowcell tables yield for them; "
                          "see make_instrument_cases.py",
           "cases": {name: [[q, evaluate(table, q)] for q in queries] for name, table in tables.items()}}
    for name, cases in doc["cases"].items():
        assert sum(1 for _, m in cases if m) >= 2 * len(tables[name]), name  # every pattern has matching queries
    with open(out_path, "w") as f:
        f.write('{"description": ' + json.dumps(doc["description"]) + ',\n "cases": {\n')
        for k, (name, cases) in enumerate(doc["cases"].items()):
            f.write('  ' + json.dumps(name) + ': [\n' + ",\n".join("   " + json.dumps(c) for c in cases) + '\n  ]' +
                    (",\n" if k + 1 < len(doc["cases"]) else "\n"))
        f.write(" }\n}\n")
    print(out_path, {name: len(c) for name, c in doc["cases"].items()}, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
