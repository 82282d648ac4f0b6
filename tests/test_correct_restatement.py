"""The correction rule (include/dskgpu.h: "substitution errors in reads corrected against the count"), restated on STRINGS and checked on
the CPU before tests/test_gpu_correct.py trusts the restatement on the device.  The trusted set is a Python set of canonical strings in
the LEXICOGRAPHIC canonical form -- min(s, reverse complement of s) as strings, which is not the order of the device's 2-bit code -- and
only membership is asked of it.  States, gaps, shapes, trials and the output bytes follow the definition literally.  The pinned numbers
are what this restatement gave on the CPU for these inputs; they were never read off a device.  All of it fails before the feature only
through the GPU file; this file checks the yardstick itself."""
import os

import numpy as np
import pytest

pytest.importorskip("torch")          # (the GPU modules import it at the top)
from tests.byte_streams import upper_bases      # noqa: E402
from tests.test_gpu_unitigs import GOLDEN, revcomp_str      # noqa: E402
from tests.test_unitigs_restatement import solid_rows      # noqa: E402

_BASES = frozenset(b"ACGTacgt")
STATS = ("n_valid", "n_trusted", "n_gaps", "n_interior", "n_head", "n_tail", "n_skipped", "n_corrected", "n_ambiguous", "n_unfixable")
KS = [15, 31, 32, 33, 63, 64, 65, 96, 127, 128]


def canon(s):
    r = revcomp_str(s)
    return s if s < r else r


class Corrected:
    """what one stream gives: state per position, the gaps (a, b, shape, e, outcome, letter), the output bytes, the stats"""

    def summary(self):
        return tuple(self.stats[n] for n in STATS)

    def gaps_in(self, first, nbytes):
        return [g for g in self.gaps if first <= g[0] < first + nbytes]


class CorrectRestatement:
    def __init__(self, values, ab, k, trust_min=0):
        from dsk_amd.engine import kmer_to_string
        self.k = k
        self.trusted = {canon(kmer_to_string(v, k)) for v, a in zip(values, ab) if a >= max(trust_min, 1)}

    def is_trusted(self, window):
        return canon(window) in self.trusted

    def states(self, raw):
        k, n = self.k, len(raw)
        text = upper_bases(raw)
        state = np.zeros(n, dtype=np.uint8)
        run = 0
        for p in range(n):
            run = run + 1 if raw[p] in _BASES else 0
            if run >= k:
                state[p] = 2 if self.is_trusted(text[p - k + 1: p + 1]) else 1
        return text, state

    def correct(self, stream):
        k = self.k
        raw = bytes(stream)
        n = len(raw)
        text, state = self.states(raw)
        R = Corrected()
        R.state, R.gaps = state, []
        out = bytearray(raw)
        st = dict.fromkeys(STATS, 0)
        st["n_valid"], st["n_trusted"] = int((state >= 1).sum()), int((state == 2).sum())
        p = 0
        while p < n:
            if state[p] != 1:
                p += 1
                continue
            a = p
            while p + 1 < n and state[p + 1] == 1:
                p += 1
            b = p
            p += 1
            m = b - a + 1
            left = int(state[a - 1]) if a > 0 else 0
            right = int(state[b + 1]) if b + 1 < n else 0
            st["n_gaps"] += 1
            if left == 2 and right == 2 and m == k:
                shape, e = "interior", a
            elif left == 0 and right == 2 and m <= k:
                shape, e = "head", b - k + 1
            elif left == 2 and right == 0 and m <= k:
                shape, e = "tail", a
            else:
                st["n_skipped"] += 1
                R.gaps.append((a, b, "skipped", -1, "skipped", ""))
                continue
            st["n_" + shape] += 1
            lo = a - k + 1                                                     # the first byte of the first window of the gap
            assert lo <= e <= a and all(raw[q] in _BASES for q in range(lo, b + 1))
            region = text[lo: b + 1]
            works = []
            for x in "ACGT":
                if x == text[e]:
                    continue
                trial = region[: e - lo] + x + region[e - lo + 1:]
                if all(self.is_trusted(trial[i: i + k]) for i in range(m)):
                    works.append(x)
            if len(works) == 1:
                outcome = "corrected"
                out[e] = ord(works[0]) | (raw[e] & 0x20)
            else:
                outcome = "ambiguous" if works else "unfixable"
            st["n_" + outcome] += 1
            R.gaps.append((a, b, shape, e, outcome, works[0] if len(works) == 1 else ""))
        assert st["n_gaps"] == st["n_interior"] + st["n_head"] + st["n_tail"] + st["n_skipped"]
        assert st["n_interior"] + st["n_head"] + st["n_tail"] == st["n_corrected"] + st["n_ambiguous"] + st["n_unfixable"]
        R.stats = st
        R.out = np.frombuffer(bytes(out), dtype=np.uint8).copy()
        return R

    def check_facts(self, stream, R):
        """every corrected gap is all-trusted afterwards; no byte outside the candidate positions differs; the second application corrects
        nothing and keeps the ambiguous, the unfixable and the skipped"""
        raw = np.frombuffer(bytes(stream), dtype=np.uint8)
        cand = [g[3] for g in R.gaps if g[4] == "corrected"]
        diff = np.nonzero(raw != R.out)[0]
        assert sorted(cand) == [int(p) for p in diff], "exactly the corrected candidate bytes differ"
        again = self.correct(R.out)
        for a, b, _, _, outcome, _ in R.gaps:
            if outcome == "corrected":
                assert (again.state[a: b + 1] == 2).all(), (a, b)
        assert again.stats["n_corrected"] == 0 and (again.out == R.out).all()
        for name in ("n_ambiguous", "n_unfixable", "n_skipped"):
            assert again.stats[name] == R.stats[name], name
        return again


# ------------------------------------------------------------------ streams (computed once, shared, never changed)
def _letters(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _other(rng, c):
    return "ACGT"[("ACGT".index(c.upper()) + int(rng.integers(1, 4))) & 3]


_planted = {}


def planted_stream(k):
    """-> (the stream with the planted errors, the error-free stream, the number of plants): a circular genome of 3000 uniform bases, reads
    of L = max(150, 3k) bases at uniform starts, 40 x 3000 / L of them, joined by a newline; every third read carries one substitution, at
    read offset 0, 1, k - 2, k - 1, k, L / 2, L - k - 1, L - k, L - 2, L - 1 in turn."""
    if k not in _planted:
        rng = np.random.default_rng(500 + k)
        genome = _letters(rng, 3000)
        L = max(150, 3 * k)
        nreads = 40 * 3000 // L
        starts = rng.integers(0, 3000, nreads)
        offsets = [0, 1, k - 2, k - 1, k, L // 2, L - k - 1, L - k, L - 2, L - 1]
        truth, reads, plants = [], [], 0
        for i, s in enumerate(starts):
            r = (genome + genome)[int(s): int(s) + L]
            truth.append(r)
            if i % 3 == 0:
                o = offsets[plants % len(offsets)]
                r = r[:o] + _other(rng, r[o]) + r[o + 1:]
                plants += 1
            reads.append(r)
        as_np = lambda rs: np.frombuffer("\n".join(rs).encode(), dtype=np.uint8).copy()      # noqa: E731
        _planted[k] = (as_np(reads), as_np(truth), plants)
    return _planted[k]


_handmade = {}


def handmade_correct(k):
    """-> (the stream to count: three copies of a genome of 8 k + 400 uniform bases and of the two alleles of a site; the stream to correct;
    {name: (first byte, bytes)} of its reads).  The reads reach every branch of the rule: see EXPECTED."""
    if k in _handmade:
        return _handmade[k]
    rng = np.random.default_rng(900 + k)
    G = _letters(rng, 8 * k + 400)
    site = _letters(rng, 2 * k + 1)
    mid = site[k]
    alleles = [c for c in "ACGT" if c != mid]
    site_a, site_b = site, site[:k] + alleles[0] + site[k + 1:]
    counted = np.frombuffer(("\n".join([G, site_a, site_b] * 3) + "\n").encode(), dtype=np.uint8).copy()

    def sub(r, *at):
        for o in at:
            r = r[:o] + {"A": "C", "C": "G", "G": "T", "T": "A", "a": "c", "c": "g", "g": "t", "t": "a"}[r[o]] + r[o + 1:]
        return r
    L = 4 * k + 50
    i = k + 5
    j = k + 10                                                                 # the N of "beside_n"
    bn = G[100: 100 + 3 * k + 20]
    glue = [c for c in "ACGT" if c not in (G[k + 9], G[5 * k - 1])][0]             # a base that continues neither side of the junction
    parts = [
        ("first_byte", sub(G[3: 3 + 2 * k + 9], 0), "\n"),                      # an error in the first byte of the stream: a head gap of one window
        ("two_k1", sub(G[:L], i, i + k + 1), ">"),                             # two errors k + 1 apart: two interior gaps, both corrected
        ("two_k", sub(G[:L], i, i + k), " "),                                  # exactly k apart: one gap of 2 k, skipped
        ("two_km1", sub(G[:L], i, i + k - 1), "\r\n"),                         # k - 1 apart: one gap of 2 k - 1, skipped
        ("beside_n", sub(bn[:j], j - 2) + "N" + sub(bn[j + 1:], 1), "\t"),     # tail and head against a base run, not a line: two windows each
        ("lower", sub(G[200: 220 + 3 * k].lower(), k + 7), "x"),               # a lower-case letter is written
        ("short", G[7: 7 + k - 1], "@"),                                       # shorter than k: no valid window
        ("exact_k", sub(G[20: 20 + k], k // 2), "-"),                          # one window, no trusted neighbour: skipped
        ("head_k", sub(G[50: 50 + 3 * k], k - 1), "\n\n"),                     # a head gap of k windows
        ("tail_k", sub(G[60: 60 + 3 * k], 2 * k), ";"),                        # a tail gap of k windows
        ("two_allele", site[:k] + alleles[1] + site[k + 1:], "\n"),            # both alleles work: ambiguous
        ("junction", G[:k + 9] + glue + G[5 * k: 6 * k + 9], "|"),              # k windows over a junction that no single base mends: unfixable
        ("chimera", G[:k + 9] + G[5 * k: 6 * k + 9], "\n"),                    # k - 1 windows over a junction: an interior gap shorter than k, skipped
        ("nowhere", _letters(rng, 3 * k), "n"),                                # a read from nowhere: one gap longer than k
        ("clean", G[300: 300 + 2 * k + 30], ","),                              # nothing to do
        ("last_byte", sub(G[9: 9 + 2 * k + 9], 2 * k + 8), ""),                # an error in the last byte of the stream, no separator behind it
    ]
    where, out = {}, ""
    for name, read, sep in parts:
        where[name] = (len(out), len(read))
        out += read + sep
    _handmade[k] = (counted, np.frombuffer(out.encode(), dtype=np.uint8).copy(), where)
    return _handmade[k]


# name -> the (shape, outcome) of the gaps inside the read, in order; asserted from k = 15 on, where k-mers do not repeat by chance
EXPECTED = {
    "first_byte": [("head", "corrected")], "two_k1": [("interior", "corrected")] * 2, "two_k": [("skipped", "skipped")],
    "two_km1": [("skipped", "skipped")], "beside_n": [("tail", "corrected"), ("head", "corrected")], "lower": [("interior", "corrected")],
    "short": [], "exact_k": [("skipped", "skipped")], "head_k": [("head", "corrected")], "tail_k": [("tail", "corrected")],
    "two_allele": [("interior", "ambiguous")], "junction": [("interior", "unfixable")], "chimera": [("skipped", "skipped")],
    "nowhere": [("skipped", "skipped")], "clean": [], "last_byte": [("tail", "corrected")],
}


def check_handmade(k, stream, where, R):
    """the branches by name"""
    for name, want in EXPECTED.items():
        got = [(g[2], g[4]) for g in R.gaps_in(*where[name])]
        assert got == want, (name, got, want)
    a, n = where["first_byte"]
    assert R.gaps[0][3] == 0 == a and R.gaps[0][:2] == (k - 1, k - 1)
    assert R.gaps[-1][3] == len(stream) - 1 and R.gaps[-1][1] == len(stream) - 1
    a, n = where["two_k"]
    assert [g[1] - g[0] + 1 for g in R.gaps_in(a, n)] == [2 * k]
    a, n = where["two_km1"]
    assert [g[1] - g[0] + 1 for g in R.gaps_in(a, n)] == [2 * k - 1]
    a, n = where["nowhere"]
    assert [g[1] - g[0] + 1 for g in R.gaps_in(a, n)] == [2 * k + 1]
    a, n = where["chimera"]
    assert [g[1] - g[0] + 1 < k for g in R.gaps_in(a, n)] == [True]
    a, n = where["beside_n"]
    assert [g[1] - g[0] + 1 for g in R.gaps_in(a, n)] == [2, 2]
    a, n = where["lower"]
    (g,) = R.gaps_in(a, n)
    assert chr(R.out[g[3]]).islower() and chr(R.out[g[3]]).upper() == g[5] and bytes(R.out[a: a + n]).decode().islower()


def restate(oracle, stream, k, amin, trust_min=0):
    values, ab = solid_rows(oracle, stream, k, amin)
    return CorrectRestatement(values, ab, k, trust_min)


# (n_valid, n_trusted, n_gaps, n_interior, n_head, n_tail, n_skipped, n_corrected, n_ambiguous, n_unfixable), computed by this restatement
# on the CPU
CORRECT_PINNED = {
    ("golden", 15): (430000, 370859, 4309, 2577, 656, 599, 477, 3720, 0, 112),
    ("golden", 31): (350000, 257037, 3821, 1022, 1113, 1094, 592, 2914, 0, 315),
    ("golden", 63): (190000, 101071, 3314, 0, 994, 954, 1366, 1603, 0, 345),
    ("planted", 15): (108800, 106253, 267, 81, 108, 78, 0, 267, 0, 0),
    ("planted", 31): (96000, 90877, 267, 81, 108, 78, 0, 267, 0, 0),
    ("planted", 32): (95200, 89916, 267, 81, 108, 78, 0, 267, 0, 0),
    ("planted", 33): (94400, 88955, 267, 81, 108, 78, 0, 267, 0, 0),
    ("planted", 63): (80518, 72472, 212, 63, 86, 63, 0, 212, 0, 0),
    ("planted", 64): (80625, 72457, 209, 63, 84, 62, 0, 209, 0, 0),
    ("planted", 65): (80565, 72468, 205, 61, 84, 60, 0, 205, 0, 0),
    ("planted", 96): (80288, 72155, 139, 42, 56, 41, 0, 139, 0, 0),
    ("planted", 127): (80070, 72017, 105, 31, 44, 30, 0, 105, 0, 0),
    ("planted", 128): (80184, 72196, 104, 30, 44, 30, 0, 104, 0, 0),
    ("hand", 1): (315, 315, 0, 0, 0, 0, 0, 0, 0, 0),
    ("hand", 4): (387, 384, 3, 0, 1, 0, 2, 0, 1, 0),
    ("hand", 15): (651, 435, 16, 5, 3, 3, 5, 9, 1, 1),
    ("hand", 31): (1035, 596, 16, 5, 3, 3, 5, 9, 1, 1),
    ("hand", 32): (1059, 606, 16, 5, 3, 3, 5, 9, 1, 1),
    ("hand", 33): (1083, 615, 16, 5, 3, 3, 5, 9, 1, 1),
    ("hand", 63): (1803, 916, 16, 5, 3, 3, 5, 9, 1, 1),
    ("hand", 64): (1827, 925, 16, 5, 3, 3, 5, 9, 1, 1),
    ("hand", 65): (1851, 935, 16, 5, 3, 3, 5, 9, 1, 1),
    ("hand", 96): (2595, 1245, 16, 5, 3, 3, 5, 9, 1, 1),
    ("hand", 127): (3339, 1555, 16, 5, 3, 3, 5, 9, 1, 1),
    ("hand", 128): (3363, 1565, 16, 5, 3, 3, 5, 9, 1, 1),
}


# ------------------------------------------------------------------ (a) the golden reads
@pytest.mark.parametrize("k", [15, 31, 63])
def test_golden_reads(oracle, golden_dir, k):
    stream = np.ascontiguousarray(oracle.load_bank(os.path.join(golden_dir, GOLDEN))[0])
    exp = restate(oracle, stream, k, 3)
    R = exp.correct(stream)
    print("correct", "golden", k, R.summary())
    assert R.summary() == CORRECT_PINNED[("golden", k)]
    exp.check_facts(stream, R)


# ------------------------------------------------------------------ (b) the planted stream
@pytest.mark.parametrize("k", KS)
def test_planted_stream(oracle, k):
    stream, truth, plants = planted_stream(k)
    exp = restate(oracle, stream, k, 3)
    R = exp.correct(stream)
    print("correct", "planted", k, R.summary())
    assert (R.out == truth).all(), "every planted error comes back to the truth and no other byte changes"
    assert R.stats["n_gaps"] == R.stats["n_corrected"] == plants
    assert R.summary() == CORRECT_PINNED[("planted", k)]
    exp.check_facts(stream, R)
    # trust_min on a count of every k-mer: the same trusted set, the same answer
    R1 = restate(oracle, stream, k, 1, trust_min=3).correct(stream)
    assert R1.summary() == R.summary() and (R1.out == R.out).all()


# ------------------------------------------------------------------ (c) the handmade stream
@pytest.mark.parametrize("k", [1, 4] + KS)
def test_handmade_stream(oracle, k):
    counted, stream, where = handmade_correct(k)
    exp = restate(oracle, counted, k, 1)
    R = exp.correct(stream)
    print("correct", "hand", k, R.summary())
    assert R.summary() == CORRECT_PINNED[("hand", k)]
    exp.check_facts(stream, R)
    if k >= 15:
        check_handmade(k, stream, where, R)
    R3 = restate(oracle, counted, k, 1, trust_min=3).correct(stream)          # three copies of everything: abundance >= 3
    assert R3.summary() == R.summary() and (R3.out == R.out).all()
    none = restate(oracle, counted, k, 1, trust_min=10 ** 6).correct(stream)  # nothing is trusted: every valid window is state 1
    assert none.stats["n_trusted"] == none.stats["n_corrected"] == 0 and none.stats["n_gaps"] == none.stats["n_skipped"] > 0
