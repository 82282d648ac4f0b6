"""The restatement of the per-read summaries, the rule and the selection (tests/read_summary_model.py) checked on the CPU before
tests/test_gpu_read_summaries.py trusts it on the device: hand-worked streams whose expected tables are written out here, the properties
that follow from the definitions, and pinned digests of the golden reads' table.  The pinned digests are what the model gave on the CPU;
they were never read off a device."""
import hashlib
import os
from collections import Counter

import numpy as np
import pytest

pytest.importorskip("torch")          # (the modules the helpers come from import it at the top)
from tests import read_summary_model as M      # noqa: E402
from tests.byte_streams import upper_bases      # noqa: E402
from tests.test_correct_restatement import _BASES, canon      # noqa: E402
from tests.test_gpu_unitigs import GOLDEN      # noqa: E402
from tests.test_unitigs_restatement import solid_rows      # noqa: E402


# ------------------------------------------------------------------ the hand-worked streams (computed once, shared, never changed)
# k = 4.  Trusted from 3 on.  ACGT and GTAC are their own reverse complements; CCCC, GCCC and GGCC are no rows.
HAND4_TABLE = {"ACGT": 7, "CGTA": 2, "AAAA": 5, "GTAC": 9}
HAND4 = (b"\n"                  # 0  a '\n' at byte 0: an empty record
         b"\n"                  # 1  "\n\n": another
         b"ACG\n"               # 2  k - 1 letters: no window
         b"ACGT\n"              # 3  k letters: one window
         b"ACGTA\n"             # 4  k + 1: [7, 2], even n_valid -> the upper of the two
         b"ACGTNACGTA\n"        # 5  an N in the middle: [7 | 7, 2], a tie at the median
         b"acgta\r\n"           # 6  lower case, '\r' inside the record
         b"AAAAAAA\n"           # 7  four times the same k-mer
         b"GGGGCCCC\n"          # 8  every k-mer absent: five valid windows of value 0
         b"ACGTAC")             # 9  no final '\n'
# (start, sum, len, n_valid, n_solid, median)
HAND4_EXPECTED = [(0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0), (2, 0, 3, 0, 0, 0), (6, 7, 4, 1, 1, 7), (11, 9, 5, 2, 1, 7), (17, 16, 10, 3, 2, 7),
                  (28, 9, 6, 2, 1, 7), (35, 20, 7, 4, 4, 5), (43, 0, 8, 5, 0, 0), (52, 18, 6, 3, 2, 7)]
HAND4_STATS = dict(n_records=10, n_empty=3, n_valid=20, n_solid=11, max_len=10)

# k = 21.  Trusted from 5 on.  The ten windows of S have the abundances W, in order; poly-T is no row.
S21 = "ACGTTGCATGCCGATAGCTTAGGCTAACGT"
W21 = [4, 9, 1, 9, 6, 3, 8, 2, 7, 5]
HAND21_TABLE = {canon(S21[i: i + 21]): W21[i] for i in range(10)}
HAND21 = "\n".join([S21[:20],                              # 0  k - 1 letters
                    S21[:21],                              # 1  k: [4], below the threshold
                    S21[:22],                              # 2  k + 1: [4, 9]
                    S21[:24],                              # 3  [4, 9, 1, 9]: even, a tie above the median
                    S21[:10] + "N" + S21[:23],             # 4  an N: ten letters without a window, then [4, 9, 1]
                    S21[2:25].lower() + "\r",              # 5  lower case and '\r': [1, 9, 6]
                    "T" * 25,                              # 6  five absent k-mers
                    S21]).encode()                         # 7  all ten, no final '\n'
HAND21_EXPECTED = [(0, 0, 20, 0, 0, 0), (21, 4, 21, 1, 0, 4), (43, 13, 22, 2, 1, 9), (66, 23, 24, 4, 2, 9), (91, 14, 34, 3, 1, 4),
                   (126, 16, 24, 3, 2, 6), (151, 0, 25, 5, 0, 0), (177, 54, 30, 10, 6, 6)]
HAND21_STATS = dict(n_records=8, n_empty=1, n_valid=28, n_solid=12, max_len=34)

HAND = {4: (HAND4, HAND4_TABLE, 3, HAND4_EXPECTED, HAND4_STATS), 21: (HAND21, HAND21_TABLE, 5, HAND21_EXPECTED, HAND21_STATS)}
RULES = [None, dict(min_valid=3), dict(median_min=7), dict(median_max=5), dict(solid_num=1, solid_den=2), dict(solid_num=1, solid_den=1),
         dict(min_valid=1, median_min=4, median_max=7, solid_num=1, solid_den=2), dict(min_valid=2, invert=True), dict(invert=True)]


def expected_array(rows):
    return np.array(rows, dtype=M.SUMMARY_DTYPE)


@pytest.mark.parametrize("k", [4, 21])
def test_hand_worked_streams(k):
    stream, table, tmin, want, want_stats = HAND[k]
    assert len(table) == (4 if k == 4 else 10)
    got, st = M.summaries(stream, table, k, tmin)
    assert got.dtype.itemsize == 32 and got.dtype.names == M.FIELDS
    assert [tuple(int(x) for x in r) for r in got] == want
    assert st == want_stats
    assert M.records(stream) == [(r[0], r[2]) for r in want]


def test_hand_worked_rules_and_selection():
    got, _ = M.summaries(HAND4, HAND4_TABLE, 4, 3)
    # n_valid: 0 0 0 1 2 3 2 4 5 3; median: 0 0 0 7 7 7 7 5 0 7; n_solid: 0 0 0 1 1 2 1 4 0 2
    assert list(M.marks(got)) == [1] * 10
    assert list(M.marks(got, dict(min_valid=3))) == [0, 0, 0, 0, 0, 1, 0, 1, 1, 1]
    assert list(M.marks(got, dict(median_min=7))) == [0, 0, 0, 1, 1, 1, 1, 0, 0, 1]
    assert list(M.marks(got, dict(median_max=5))) == [1, 1, 1, 0, 0, 0, 0, 1, 1, 0]
    assert list(M.marks(got, dict(solid_num=2, solid_den=3))) == [1, 1, 1, 1, 0, 1, 0, 1, 0, 1]      # 0 / 0 passes: 0 * 3 >= 2 * 0
    assert list(M.marks(got, dict(min_valid=1, solid_num=2, solid_den=3, invert=True))) == [1, 1, 1, 0, 1, 0, 1, 0, 1, 0]
    keep = M.marks(got, dict(median_min=7))
    assert bytes(M.select(HAND4, keep)) == b"ACGT\nACGTA\nACGTNACGTA\nacgta\r\nACGTAC\n"
    assert M.mark_stats(got, keep) == dict(n_records=10, n_kept=5, kept_bytes=36, kept_valid=11)
    assert bytes(M.select(HAND4, np.ones(10, dtype=np.uint8))) == HAND4 + b"\n"
    assert len(M.select(HAND4, np.zeros(10, dtype=np.uint8))) == 0
    assert bytes(M.select(b"\n\n", [1, 1])) == b"\n\n" and bytes(M.select(b"\n\n", [0, 1])) == b"\n" and M.records(b"") == []


# ------------------------------------------------------------------ properties
def golden_part(oracle, golden_dir, n_records=600):
    stream = np.ascontiguousarray(oracle.load_bank(os.path.join(golden_dir, GOLDEN))[0])
    ends = np.flatnonzero(stream == M.NL)
    return stream, stream[: int(ends[n_records - 1]) + 1].copy()


def kmer_counts(raw, k):
    """Counter of the canonical strings of the valid windows"""
    c, run, text = Counter(), 0, upper_bases(raw)
    for p in range(len(raw)):
        run = run + 1 if raw[p] in _BASES else 0
        if run >= k:
            c[canon(text[p - k + 1: p + 1])] += 1
    return c


@pytest.mark.parametrize("k", [15, 31, 63])
def test_properties(oracle, golden_dir, k):
    whole, part = golden_part(oracle, golden_dir)
    values, ab = solid_rows(oracle, whole, k, 2)
    table = M.table_of(values, ab, k)
    T, st = M.summaries(part, table, k, 0)
    assert st["n_records"] == 600 == len(T) and int(T["n_valid"].sum()) == st["n_valid"] == oracle.count(part, k).total
    valid, a = M.values(bytes(part), table, k)
    for s in T[:200]:
        v = a[int(s["start"]): int(s["start"]) + int(s["len"])][valid[int(s["start"]): int(s["start"]) + int(s["len"])]]
        if len(v):
            assert v.min() <= s["median"] <= v.max() and int(v.sum()) == s["sum"] and (np.sort(v)[len(v) // 2] == s["median"])
    solid = [M.summaries(part, table, k, t)[0]["n_solid"] for t in (0, 1, 2, 5, 50)]
    assert (solid[0] == solid[1]).all()
    for lo, hi in zip(solid[1:], solid[2:]):
        assert (hi <= lo).all()
    assert (solid[1] <= T["n_valid"]).all() and solid[-1].sum() < solid[1].sum()
    # the selection
    assert (M.select(part, np.ones(600, dtype=np.uint8)) == part).all()
    rule = dict(median_min=int(np.median(T["median"])), min_valid=1)
    keep = M.marks(T, rule)
    assert 0 < keep.sum() < 600
    inv = M.marks(T, dict(rule, invert=True))
    assert (keep + inv == 1).all()
    sel = M.select(part, keep)
    assert len(sel) == M.mark_stats(T, keep)["kept_bytes"]
    assert (M.select(sel, np.ones(int(keep.sum()), dtype=np.uint8)) == sel).all()      # selecting everything from a selection: the selection
    T2, _ = M.summaries(sel, table, k, 0)
    for f in ("sum", "len", "n_valid", "n_solid", "median"):
        assert (T2[f] == T[keep != 0][f]).all(), f
    assert (M.marks(T2, rule) == 1).all()                                    # the rule is idempotent on what it kept
    # counting the selection gives the k-mers of the kept records only
    want = Counter()
    raw = bytes(part)
    for (s, n), kp in zip(M.records(raw), keep):
        if kp:
            want.update(kmer_counts(raw[s: s + n], k))
    back = oracle.count(sel, k)
    got = {canon(M.value_to_string(int(v), k)): int(c) for v, c in zip(back.values(), back.ab)}
    assert got == dict(want)


# ------------------------------------------------------------------ pinned digests of the golden reads' table
GOLDEN_PINNED = {
    15: ("9305f72e87b0377a0b8fe2d2dbce9f7af70bfc3a", (600, 0, 51600, 44441, 100)),
    31: ("0e53a7c014cfbdd679e5d51acb9929340d51f90c", (600, 0, 42000, 30609, 100)),
}


def digest(table):
    return hashlib.sha1(np.ascontiguousarray(table).tobytes()).hexdigest()


@pytest.mark.parametrize("k", [15, 31])
def test_golden_digests(oracle, golden_dir, k):
    whole, part = golden_part(oracle, golden_dir)
    values, ab = solid_rows(oracle, whole, k, 3)
    T, st = M.summaries(part, M.table_of(values, ab, k), k, 5)
    print("read summaries golden", k, digest(T), tuple(st[n] for n in M.STATS))
    assert (digest(T), tuple(st[n] for n in M.STATS)) == GOLDEN_PINNED[k]
