"""Reads threaded through the compacted de Bruijn graph (include/dskgpu.h: "reads threaded through the compacted graph"), restated on
STRINGS and checked on the CPU before tests/test_gpu_thread.py trusts the restatement on the device.  The restatement never looks at
unitig[] / pos[]: it cuts every k-letter substring out of the text of every oriented unitig, keeps them in a dictionary substring -> (U, j)
(the smaller U winning, which names the even reading of a palindrome's unitig), and looks every window of a stream up in it.  Walks, steps
and supports then follow the definition.  check_facts asserts, for every walk, the inside / edge-step facts, the window-count identity and
the text identity.  (n_valid, n_placed, n_walks, n_steps, max_steps, sum of edge_support) are the numbers this restatement gave on the CPU
for these inputs; they were never read off the device."""
import os

import numpy as np
import pytest

pytest.importorskip("torch")          # (the GPU modules import it at the top)
from tests.byte_streams import upper_bases      # noqa: E402
from tests.test_gpu_unitigs import GOLDEN, circles_stream, handmade_stream, revcomp_str      # noqa: E402
from tests.test_unitig_edges_restatement import EdgeRestatement      # noqa: E402
from tests.test_unitigs_restatement import solid_rows      # noqa: E402

_BASES = frozenset(b"ACGTacgt")


class Threaded:
    """what one stream gives: per position U and j (-1 / 0 = not placed), the walks, the steps, the supports, the stats"""


class ThreadRestatement(EdgeRestatement):
    def __init__(self, values, ab, k):
        super().__init__(values, ab, k)
        nu = len(self.paths)
        self.L = [len(path) for path, _ in self.paths]
        self.where = {}
        for U in range(2 * nu - 1, -1, -1):                                  # descending: the smaller U wins
            t = self.text_of(U)
            assert len(t) == self.L[U >> 1] + k - 1
            for j in range(self.L[U >> 1]):
                self.where[t[j: j + k]] = (U, j)
        assert len(self.where) == 2 * self.n - sum(self.pal)

    def thread(self, stream):
        k = self.k
        raw = bytes(stream)
        text = upper_bases(raw)
        n = len(raw)
        T = Threaded()
        T.U = np.full(n, -1, dtype=np.int64)
        T.j = np.zeros(n, dtype=np.int64)
        run, n_valid = 0, 0
        for p in range(n):
            run = run + 1 if raw[p] in _BASES else 0
            if run >= k:
                n_valid += 1
                hit = self.where.get(text[p - k + 1: p + 1])
                if hit is not None:
                    T.U[p], T.j[p] = hit
        placed = T.U >= 0
        before = np.concatenate([[False], placed[:-1]])
        after = np.concatenate([placed[1:], [False]])
        T.first = np.nonzero(placed & ~before)[0]
        T.last = np.nonzero(placed & ~after)[0]
        step = placed & (~before | (T.j == 0))
        T.steps = T.U[step]
        T.offsets = np.concatenate([np.cumsum(step)[T.first] - 1, [int(step.sum())]]).astype(np.int64) if len(T.first) else np.zeros(1, dtype=np.int64)
        T.ends = np.stack([T.j[T.first], T.j[T.last]], axis=1) if len(T.first) else np.zeros((0, 2), dtype=np.int64)
        T.unitig_support = np.bincount(T.U[placed] >> 1, minlength=len(self.paths)).astype(np.int64)[: max(len(self.paths), 0)]
        T.edge_support = np.zeros(self.edge_stats["n_edges"], dtype=np.int64)
        for p in np.nonzero(placed & before & (T.j == 0))[0]:
            frm, to = int(T.U[p - 1]), int(T.U[p])
            assert to in self.edges[frm], ("an edge step walks an edge of the graph", p, frm, to)
            T.edge_support[self.e_offsets[frm] + self.edges[frm].index(to)] += 1
        per_walk = np.diff(T.offsets)
        T.stats = dict(n_valid=n_valid, n_placed=int(placed.sum()), n_walks=len(T.first), n_steps=int(step.sum()),
                       max_steps=int(per_walk.max()) if len(per_walk) else 0)
        T.text = text
        return T

    def summary(self, T):
        s = T.stats
        return (s["n_valid"], s["n_placed"], s["n_walks"], s["n_steps"], s["max_steps"], int(T.edge_support.sum()))

    def check_facts(self, T):
        k, L = self.k, self.L
        assert len(T.first) == len(T.last) == len(T.offsets) - 1
        assert int(T.unitig_support.sum()) == T.stats["n_placed"] and int(T.edge_support.sum()) == T.stats["n_steps"] - T.stats["n_walks"]
        for w, (a, b) in enumerate(zip(T.first, T.last)):
            steps = [int(U) for U in T.steps[T.offsets[w]: T.offsets[w + 1]]]
            assert steps[0] == T.U[a]
            for p in range(a + 1, b + 1):
                if T.j[p] == 0:                                              # an edge step
                    assert T.j[p - 1] == L[T.U[p - 1] >> 1] - 1 and int(T.U[p]) in self.edges[int(T.U[p - 1])], (w, p)
                else:                                                        # an inside step
                    assert T.U[p] == T.U[p - 1] and T.j[p] == T.j[p - 1] + 1, (w, p)
            assert b - a + 1 == sum(L[U >> 1] for U in steps) - T.j[a] - (L[steps[-1] >> 1] - 1 - T.j[b]), ("the window count", w)
            glued = self.text_of(steps[0]) + "".join(self.text_of(U)[k - 1:] for U in steps[1:])
            cut = L[steps[-1] >> 1] - 1 - int(T.j[b])
            assert glued[int(T.j[a]): len(glued) - cut] == T.text[a - k + 1: b + 1], ("the text", w)


# ------------------------------------------------------------------ streams (computed once, shared, never changed)
def thread_stream(k):
    """What a threading has to get right, read through the graph of handmade_stream(k) (counted with abundance_min 1): fragments of k - 1 and
    of exactly k letters, a lower-case read, a read with N in the middle, separators other than a newline, no separator at the end, a read
    and its reverse complement, a read three and more times round the AC cycle, poly-A longer than k, the palindrome's read (even k), the AT
    hairpin, and a read that was not counted: one substitution, so k windows between its two walks are no rows.
    -> (stream, {name: (first byte, bytes)} of the reads the tests look at)"""
    reads = bytes(handmade_stream(k)).decode().split("\n")
    r300 = reads[-5]
    assert len(r300) == 300 and reads[-4] == revcomp_str(r300) and reads[-1] == ""
    sub = r300[:150] + {"A": "C", "C": "G", "G": "T", "T": "A"}[r300[150]] + r300[151:]
    parts = [("fwd", r300, "\n"), ("rev", revcomp_str(r300), ">"), ("short", r300[7: 7 + k - 1], " "), ("exact", r300[5: 5 + k], "\r\n"),
             ("lower", r300.lower(), "N"), ("n_inside", r300[:150] + "N" + r300[151:], "\t"), ("ac", "AC" * ((k + 1) // 2 + 4), "x"),
             ("poly_a", "A" * (k + 9), "\n\n"), ("at", "AT" * ((k + 21) // 2), "@"), ("sub", sub, "-")]
    if k % 2 == 0:
        parts.append(("palindrome", reads[4], "\n"))
    parts.append(("tail", r300[100:], ""))                                   # no separator at the end
    where, out = {}, ""
    for name, read, sep in parts:
        where[name] = (len(out), len(read))
        out += read + sep
    return np.frombuffer(out.encode(), dtype=np.uint8).copy(), where


def check_flipped(exp, T, where):
    """the reverse complement of a read walks the flipped steps in reverse order (a palindrome's unitig has one name, the even one)"""
    def flip(U):
        return U if exp.unitig_is_palindrome(U >> 1) else U ^ 1

    def walks_in(name):
        a, n = where[name]
        return [[int(U) for U in T.steps[T.offsets[w]: T.offsets[w + 1]]] for w in range(len(T.first)) if a <= T.first[w] < a + n]
    fwd, rev = walks_in("fwd"), walks_in("rev")
    assert len(fwd) == len(rev) >= 1
    assert [[flip(U) for U in reversed(w)] for w in reversed(fwd)] == rev


# (n_valid, n_placed, n_walks, n_steps, max_steps, sum of edge_support), computed by this restatement on the CPU
THREAD_PINNED = {
    ("hand", 1, 1): (1742, 1742, 11, 1742, 300, 1731), ("hand", 2, 1): (1754, 1754, 12, 1754, 299, 1742),
    ("hand", 15, 1): (1644, 1629, 12, 46, 22, 34), ("hand", 16, 1): (1656, 1640, 13, 48, 21, 35),
    ("hand", 31, 1): (1532, 1501, 12, 46, 22, 34), ("hand", 32, 1): (1544, 1512, 13, 48, 21, 35),
    ("hand", 33, 1): (1518, 1485, 12, 46, 22, 34), ("hand", 64, 1): (1320, 1256, 13, 50, 21, 37),
    ("hand", 65, 1): (1294, 1229, 12, 46, 22, 34), ("hand", 128, 1): (872, 744, 13, 48, 21, 35),
    ("golden", 15, 2): (430000, 376719, 7793, 23161, 12, 15368), ("golden", 31, 2): (350000, 263139, 6296, 11676, 10, 5380),
    ("golden", 63, 2): (190000, 103243, 3759, 4148, 4, 389), ("golden", 65, 2): (180000, 95783, 3604, 3894, 4, 290),
    # every k-mer of the golden reads, errors included: every window is placed, one walk per read
    ("golden", 15, 1): (430000, 430000, 5000, 204596, 68, 199596),
    ("circles", 31, 1): (28194, 28194, 3, 5, 2, 2),
}


def restate(oracle, stream, k, amin):
    values, ab = solid_rows(oracle, stream, k, amin)
    return ThreadRestatement(values, ab, k)


@pytest.mark.parametrize("k", sorted(k for kind, k, _ in THREAD_PINNED if kind == "hand"))
def test_handmade_stream(oracle, k):
    exp = restate(oracle, handmade_stream(k), k, 1)
    stream, where = thread_stream(k)
    T = exp.thread(stream)
    exp.check_facts(T)
    check_flipped(exp, T, where)
    print("thread", "hand", k, exp.summary(T))
    assert exp.summary(T) == THREAD_PINNED[("hand", k, 1)]
    if k >= 15:
        a, n = where["sub"]
        inside = [w for w in range(len(T.first)) if a <= T.first[w] < a + n]
        assert len(inside) == 2 and T.first[inside[1]] - T.last[inside[0]] == k + 1      # k windows that are no rows lie between the two walks
        a, n = where["ac"]
        w = [w for w in range(len(T.first)) if a <= T.first[w] < a + n]
        assert len(w) == 1 and T.offsets[w[0] + 1] - T.offsets[w[0]] >= 4               # round the cycle of two rows: an edge step every second window
    short = exp.thread(stream[where["short"][0]: where["short"][0] + k - 1])               # a stream shorter than k
    assert exp.summary(short) == (0, 0, 0, 0, 0, 0) and len(short.offsets) == 1


@pytest.mark.parametrize("k,amin", sorted((k, a) for kind, k, a in THREAD_PINNED if kind == "golden"))
def test_golden_reads(oracle, golden_dir, k, amin):
    stream = np.ascontiguousarray(oracle.load_bank(os.path.join(golden_dir, GOLDEN))[0])
    exp = restate(oracle, stream, k, amin)
    T = exp.thread(stream)
    exp.check_facts(T)
    print("thread", "golden", k, amin, exp.summary(T))
    assert exp.summary(T) == THREAD_PINNED[("golden", k, amin)]
    if amin == 1:
        assert T.stats["n_placed"] == T.stats["n_valid"]                     # every k-mer of the reads is a row


def test_long_chain_and_two_circles(oracle):
    stream = circles_stream(31)
    exp = restate(oracle, stream, 31, 1)
    T = exp.thread(stream)
    exp.check_facts(T)
    print("thread", "circles", 31, exp.summary(T))
    assert exp.summary(T) == THREAD_PINNED[("circles", 31, 1)]
