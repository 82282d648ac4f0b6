"""The edges of the compacted de Bruijn graph (include/dskgpu.h: "unitig links"), restated on STRINGS and checked on the CPU before
tests/test_gpu_unitig_edges.py trusts the restatement on the device: on the oracle's solid rows (global order) the four facts the header
derives from the definition hold, and (edges, oriented unitigs with 0 .. 4 edges, self edges) are the numbers fixed for these inputs."""
import os

import numpy as np
import pytest

pytest.importorskip("torch")          # (the GPU module imports it at the top)
from dsk_amd.engine import kmer_to_string      # noqa: E402
from tests.test_gpu_unitigs import GOLDEN, NONE, Restatement, circles_stream, encode, handmade_stream, revcomp_str      # noqa: E402
from tests.test_unitigs_restatement import solid_rows      # noqa: E402


class EdgeRestatement(Restatement):
    """Restatement + the edges between its oriented unitigs U = 2 u + t, by the definition: U -> V <=> first(V) is in succ(last(U))."""

    def __init__(self, values, ab, k):
        super().__init__(values, ab, k)
        S = [kmer_to_string(v, k) for v in values]
        row_of = {v: r for r, v in enumerate(values)}
        self.pal = [s == revcomp_str(s) for s in S]

        def text(o):
            return revcomp_str(S[o >> 1]) if o & 1 else S[o >> 1]

        def node(s):
            """the oriented node that reads s (a palindrome: its forward node), or NONE"""
            f, r = encode(s), encode(revcomp_str(s))
            row = row_of.get(min(f, r))
            return NONE if row is None else 2 * row + (0 if f <= r else 1)

        nu = len(self.paths)
        first, last = [], []
        for path, _ in self.paths:
            first += [path[0], path[-1] ^ 1]
            last += [path[-1], path[0] ^ 1]
        starts = {}                                                          # first(V) -> every V it is the first node of
        for V, o in enumerate(first):
            starts.setdefault(o, []).append(V)
        self.text_of = lambda U: revcomp_str(self.seq(U >> 1)) if U & 1 else self.seq(U >> 1)
        self.edges = []                                                      # edges[U] = the V in the order of the appended base A, C, T, G
        for U in range(2 * nu):
            out = []
            for b in "ACTG":
                p = node(text(last[U])[1:] + b)
                if p == NONE:
                    continue
                assert len(starts.get(p, ())) == 1, ("fact 1: a successor is the first node of exactly one oriented unitig", U, b)
                out.append(starts[p][0])
            self.edges.append(out)
        self.ends = np.array(last, dtype=np.int64)
        deg = [len(e) for e in self.edges]
        self.e_offsets = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        self.e_targets = np.array([V for e in self.edges for V in e], dtype=np.int64)
        self.hist = [deg.count(d) for d in range(5)]
        self.edge_stats = dict(n_edges=sum(deg), n_self=sum(1 for U, e in enumerate(self.edges) for V in e if V >> 1 == U >> 1),
                               n_dead_ends=self.hist[0], max_degree=max(deg) if deg else 0)

    def seq(self, u):
        return bytes(self.stream[self.offsets[u]: self.offsets[u + 1] - 1]).decode()

    def unitig_is_palindrome(self, u):
        path = self.paths[u][0]
        return len(path) == 1 and self.pal[path[0] >> 1]

    def summary(self):
        return (self.edge_stats["n_edges"], self.hist, self.edge_stats["n_self"])

    def check_facts(self):
        nu = len(self.paths)
        pairs = set()
        for U, e in enumerate(self.edges):
            assert len(set(e)) == len(e) <= 4, ("fact 2: the targets of one oriented unitig are distinct, at most 4", U, e)
            pairs.update((U, V) for V in e)
            for V in e:
                if self.unitig_is_palindrome(V >> 1):
                    assert V & 1 == 0, ("an edge into a palindrome names its forward reading", U, V)
        assert len(pairs) == self.edge_stats["n_edges"] <= 8 * nu
        for u, (path, cyc) in enumerate(self.paths):
            if cyc:
                assert self.edges[2 * u] == [2 * u] and self.edges[2 * u + 1] == [2 * u + 1], ("fact 3: a cycle has the link that closes it", u)
                assert not any(V >> 1 == u for U, V in pairs if U >> 1 != u), ("fact 3: and no other edge", u)
        for U, V in pairs:
            if not self.unitig_is_palindrome(U >> 1) and not self.unitig_is_palindrome(V >> 1):
                assert (V ^ 1, U ^ 1) in pairs, ("fact 4: U -> V <=> flip(V) -> flip(U)", U, V)
        k = self.k
        for U, V in pairs:                                                   # what an edge means on the sequences: a k - 1 overlap
            assert self.text_of(U)[len(self.text_of(U)) - (k - 1):] == self.text_of(V)[: k - 1], (U, V)


# (n_edges, [oriented unitigs with 0, 1, 2, 3, 4 edges], n_self): fixed on the CPU, whatever the row order
EDGES_PINNED = {
    ("hand", 1, 1): (16, [0, 0, 0, 0, 4], 8), ("hand", 2, 1): (80, [0, 0, 0, 0, 20], 4),
    ("hand", 15, 1): (8, [4, 8, 0, 0, 0], 8), ("hand", 31, 1): (8, [4, 8, 0, 0, 0], 8), ("hand", 33, 1): (8, [4, 8, 0, 0, 0], 8),
    ("hand", 65, 1): (8, [4, 8, 0, 0, 0], 8),
    ("hand", 16, 1): (16, [6, 12, 2, 0, 0], 6), ("hand", 32, 1): (16, [6, 12, 2, 0, 0], 6), ("hand", 128, 1): (16, [6, 12, 2, 0, 0], 6),
    ("hand", 64, 1): (17, [6, 15, 1, 0, 0], 6),
    ("golden", 15, 2): (1623, [235, 790, 406, 7, 0], 3), ("golden", 31, 2): (814, [279, 399, 203, 3, 0], 0),
    ("golden", 63, 2): (140, [145, 70, 35, 0, 0], 0), ("golden", 96, 2): (0, [1200, 0, 0, 0, 0], 0),
    ("circles", 31, 1): (4, [2, 4, 0, 0, 0], 4),
    # the branching-heavy case: every k-mer of the golden reads, errors included; the value this restatement gives
    ("golden", 15, 1): (27481, [1150, 9290, 7550, 989, 31], 9),
}


def check(oracle, kind, stream, k, amin):
    values, ab = solid_rows(oracle, stream, k, amin)
    exp = EdgeRestatement(values, ab, k)
    exp.check_facts()
    print("unitig edges", kind, k, amin, exp.summary())
    assert exp.summary() == EDGES_PINNED[(kind, k, amin)]
    assert sum(exp.hist) == 2 * exp.stats["n_unitigs"] and sum(d * c for d, c in enumerate(exp.hist)) == exp.edge_stats["n_edges"]
    return exp


@pytest.mark.parametrize("k", sorted(k for kind, k, _ in EDGES_PINNED if kind == "hand"))
def test_handmade_stream(oracle, k):
    check(oracle, "hand", handmade_stream(k), k, 1)


@pytest.mark.parametrize("k,amin", sorted((k, a) for kind, k, a in EDGES_PINNED if kind == "golden"))
def test_golden_reads(oracle, golden_dir, k, amin):
    stream = np.ascontiguousarray(oracle.load_bank(os.path.join(golden_dir, GOLDEN))[0])
    exp = check(oracle, "golden", stream, k, amin)
    if amin == 1:
        assert exp.hist[3] + exp.hist[4] > 100                               # ends of degree 3 and 4, which the solid rows hardly have


def test_long_chain_and_two_circles(oracle):
    exp = check(oracle, "circles", circles_stream(31), 31, 1)
    assert sorted(len(e) for e in exp.edges) == [0, 0, 1, 1, 1, 1]
