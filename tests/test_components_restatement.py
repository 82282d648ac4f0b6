"""The connected components of include/dskgpu.h ("connected components"), restated on the Python lists of the edge restatement and checked on
the CPU before tests/test_gpu_components.py trusts it on the device: components by a breadth-first search over the edges taken in both
directions, numbered by their smallest unitig; the table; small; and a drop() that restates the kept rows from scratch.  What follows from
the definition is asserted on every input the restatement sees: the symmetry fact, the column sums, first strictly ascending with
comp[first[c]] == c, a cycle is a component by itself, and -- after drop() -- the kept rows give exactly the old unitigs and the old table
of the components that were not small, and a second drop() removes nothing.  On the oracle's solid rows (global order) the numbers are
those fixed for these inputs."""
import os

import numpy as np
import pytest

pytest.importorskip("torch")          # (the GPU modules imported below import it at the top)
from tests.test_gpu_unitigs import GOLDEN, circles_stream, handmade_stream, revcomp_str      # noqa: E402
from tests.test_unitig_edges_restatement import EdgeRestatement      # noqa: E402
from tests.test_unitigs_restatement import solid_rows      # noqa: E402

STAT_NAMES = ("n_components", "n_single", "max_unitigs", "max_rows")
COLUMNS = ("unitigs", "rows", "ab_sum", "edges")


class ComponentRestatement(EdgeRestatement):
    """EdgeRestatement + the components of its unitigs, by the definition.  base: an EdgeRestatement of the same rows that exists already
    (the GPU tests share one per input), taken over instead of being made again."""

    def __init__(self, values, ab, k, base=None):
        if base is None:
            super().__init__(values, ab, k)
        else:
            assert base.n == len(values) and base.k == k
            self.__dict__.update(base.__dict__)
        self.values, self.ab = list(values), [int(a) for a in ab]
        nu = len(self.paths)
        joined = [set() for _ in range(nu)]
        for U, e in enumerate(self.edges):
            for V in e:
                if U >> 1 != V >> 1:                                         # every entry counts in both directions; self edges join nothing
                    joined[U >> 1].add(V >> 1)
                    joined[V >> 1].add(U >> 1)
        comp = [-1] * nu
        first = []
        for u in range(nu):                                                  # ascending: u is the smallest unitig of a component not seen yet
            if comp[u] >= 0:
                continue
            c = len(first)
            first.append(u)
            comp[u] = c
            todo = [u]
            while todo:
                nxt = []
                for x in todo:
                    for y in joined[x]:
                        if comp[y] < 0:
                            comp[y] = c
                            nxt.append(y)
                todo = nxt
        nc = len(first)
        self.L = [int(self.offsets[u + 1] - self.offsets[u]) - k for u in range(nu)]
        self.comp = np.array(comp, dtype=np.int64)
        self.first = np.array(first, dtype=np.int64)
        self.row_comp = self.comp[self.unitig] if self.n else np.zeros(0, np.int64)
        self.table = {name: np.zeros(nc, dtype=np.int64) for name in COLUMNS}
        for u in range(nu):
            c = comp[u]
            self.table["unitigs"][c] += 1
            self.table["rows"][c] += self.L[u]
            self.table["ab_sum"][c] += int(self.ab_sum[u])
            self.table["edges"][c] += len(self.edges[2 * u]) + len(self.edges[2 * u + 1])
        t = self.table
        self.comp_stats = dict(n_components=nc, n_single=int((t["unitigs"] == 1).sum()), max_unitigs=int(t["unitigs"].max()) if nc else 0,
                               max_rows=int(t["rows"].max()) if nc else 0)

    def component_summary(self):
        return tuple(self.comp_stats[n] for n in STAT_NAMES)

    def small(self, min_rows, max_abundance=0):
        """-> (uint8 per component, uint8 per row, the stats of dskgpu_graph_small_components)"""
        assert min_rows >= 1
        t = self.table
        sm = np.array([int(t["rows"][c]) < min_rows and (max_abundance == 0 or int(t["ab_sum"][c]) <= max_abundance * int(t["rows"][c]))
                       for c in range(len(self.first))], dtype=np.uint8)
        rows = sm[self.row_comp] if self.n else np.zeros(0, np.uint8)
        dropped = int(rows.sum())
        st = dict(n_small=int(sm.sum()), n_unitigs_dropped=int(t["unitigs"][sm != 0].sum()), n_rows_dropped=dropped, n_rows_left=self.n - dropped)
        assert dropped == int(t["rows"][sm != 0].sum())
        return sm, rows, st

    def canonical_texts(self, unitigs):
        return sorted(min(self.seq(u), revcomp_str(self.seq(u))) for u in unitigs)

    def check_component_facts(self):
        nu, nc = len(self.paths), len(self.first)
        pairs = {(U, V) for U, e in enumerate(self.edges) for V in e}
        for U, V in pairs:                                                   # the symmetry fact
            u, v = U >> 1, V >> 1
            assert any((Y, X) in pairs for Y in (2 * v, 2 * v + 1) for X in (2 * u, 2 * u + 1)), ("for every entry U -> V one from v back to u", U, V)
            assert self.comp[u] == self.comp[v]
        t = self.table
        assert int(t["unitigs"].sum()) == nu and int(t["rows"].sum()) == self.n
        assert int(t["ab_sum"].sum()) == sum(self.ab) and int(t["edges"].sum()) == self.edge_stats["n_edges"]
        assert (np.diff(self.first) > 0).all() and (self.comp[self.first] == np.arange(nc)).all()
        assert all(self.first[c] == np.nonzero(self.comp == c)[0].min() for c in range(nc)), "the label is the smallest unitig"
        for u, (_, cyc) in enumerate(self.paths):
            if cyc and self.edges[2 * u] == [2 * u] and self.edges[2 * u + 1] == [2 * u + 1] and not any(V >> 1 == u for U, V in pairs if U >> 1 != u):
                assert t["unitigs"][self.comp[u]] == 1, ("a cycle with no other edge is a component by itself", u)

    def drop(self, min_rows, max_abundance=0):
        """-> (the restatement of the rows that are on no small component, made from scratch; the stats of dskgpu_drop_components).  Checks
        that one application is final."""
        sm, row_drop, st = self.small(min_rows, max_abundance)
        if st["n_small"] == 0:                                                # (nothing to take out: the rows left are these rows)
            return self, st
        keep = row_drop == 0
        new = ComponentRestatement([v for v, f in zip(self.values, keep) if f], [a for a, f in zip(self.ab, keep) if f], self.k)
        new.check_facts()
        new.check_component_facts()
        kept_c = np.nonzero(sm == 0)[0]
        kept_u = [u for u in range(len(self.paths)) if sm[self.comp[u]] == 0]
        assert new.canonical_texts(range(len(new.paths))) == self.canonical_texts(kept_u), "the old unitigs of the components that were not small"
        rank = {u: i for i, u in enumerate(kept_u)}                            # the kept unitigs keep their order: renumbered, nothing else
        assert new.first.tolist() == [rank[int(self.first[c])] for c in kept_c]
        for name in COLUMNS:
            assert (new.table[name] == self.table[name][kept_c]).all(), name
        assert (new.comp == np.array([int(np.searchsorted(kept_c, self.comp[u])) for u in kept_u], dtype=np.int64)).all()
        assert new.edge_stats["n_edges"] == self.edge_stats["n_edges"] - int(self.table["edges"][sm != 0].sum())
        again = new.small(min_rows, max_abundance)[2]
        assert again["n_small"] == 0 and again["n_rows_dropped"] == 0, "a second application removes nothing"
        return new, st


def components_stream(k):
    """-> the reads.  A comb: one random backbone, read once, with a one-base fork every k + 3 bases (60 of them) -- 61 pieces of the backbone
    and 60 single-node branches in ONE component, the pieces a path of 61 unitigs whose numbers, given by k-mer values, are scattered along
    it; a second comb with 8 forks; a circle of k rows and one of 3 k; a lone k-mer; a lone chain of 10 rows, read three times."""
    rng = np.random.default_rng(9000 + k)
    def rnd(n): return "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    def other(c): return "ACGT"[("ACGT".index(c) + 1) % 4]
    def comb(forks):
        M = rnd((forks + 1) * (k + 3) + k)
        return [M] + [M[p - (k - 1): p] + other(M[p]) for p in range(k + 3, (forks + 1) * (k + 3), k + 3)]
    def circle(n):
        c = rnd(n)
        return ((c * k)[: n + k - 1])                                        # n windows, the last one's successor is the first
    chain = rnd(k + 9)
    reads = comb(60) + comb(8) + [circle(k), circle(3 * k), rnd(k), chain, chain, chain]
    return np.frombuffer(("\n".join(reads) + "\n").encode(), dtype=np.uint8).copy()


COMPONENTS_STREAM_K = [16, 31, 64, 65]

# (n_components, n_single, max_unitigs, max_rows) and the summary of drop(2 k) = (n_small, n_unitigs_dropped, n_rows_dropped): fixed on the
# CPU, whatever the row order
COMPONENTS_PINNED = {
    ("golden", 15, 2): ((26, 25, 694, 12912), (25, 25, 88)),
    ("golden", 31, 2): ((66, 65, 377, 12569), (65, 65, 527)),
    ("golden", 63, 2): ((55, 54, 71, 10297), (54, 54, 648)),
    ("golden", 96, 2): ((600, 600, 1, 19), (600, 600, 2525)),
    ("golden", 15, 1): ((1, 0, 9505, 66281), (0, 0, 0)),
    ("hand", 16, 1): ((7, 5, 3, 285), (6, 9, 28)),
    ("hand", 64, 1): ((7, 5, 4, 237), (6, 10, 26)),
    ("circles", 31, 1): ((3, 3, 1, 20000), (0, 0, 0)),
}
# the components stream at every k: six components, four of them one unitig (the circles, the k-mer, the chain); the comb has 121 unitigs and
# 61 (k + 3) + 1 + 60 rows, and drop(2 k) takes the small circle, the k-mer and the chain: k + 11 rows
COMPONENTS_STREAM_STATS = lambda k: (6, 4, 121, 61 * (k + 3) + 61)      # noqa: E731
COMPONENTS_STREAM_DROP = lambda k: (3, 3, k + 11)      # noqa: E731

_done = {}


def restated_stream(oracle, k):
    if k not in _done:
        values, ab = solid_rows(oracle, components_stream(k), k, 1)
        _done[k] = ComponentRestatement(values, ab, k)
    return _done[k]


def drop_summary(st):
    return (st["n_small"], st["n_unitigs_dropped"], st["n_rows_dropped"])


def check(oracle, kind, stream, k, amin):
    values, ab = solid_rows(oracle, stream, k, amin)
    exp = ComponentRestatement(values, ab, k)
    exp.check_component_facts()
    new, st = exp.drop(2 * k)
    print("components", kind, k, amin, exp.component_summary(), drop_summary(st))
    assert (exp.component_summary(), drop_summary(st)) == COMPONENTS_PINNED[(kind, k, amin)]
    assert new.n == st["n_rows_left"] == exp.n - st["n_rows_dropped"]
    return exp


@pytest.mark.parametrize("k,amin", sorted((k, a) for kind, k, a in COMPONENTS_PINNED if kind == "golden"))
def test_golden_reads(oracle, golden_dir, k, amin):
    stream = np.ascontiguousarray(oracle.load_bank(os.path.join(golden_dir, GOLDEN))[0])
    exp = check(oracle, "golden", stream, k, amin)
    if (k, amin) == (96, 2):
        assert exp.edge_stats["n_edges"] == 0 and exp.hist[0] == 1200      # 1200 dead ends and no edge: every unitig by itself
    if (k, amin) == (15, 1):
        assert exp.comp_stats["n_components"] == 1                          # one tangle


@pytest.mark.parametrize("k", [16, 64])
def test_handmade_stream(oracle, k):
    """even k: palindromes among the rows, whose edges the symmetry fact has to cover"""
    exp = check(oracle, "hand", handmade_stream(k), k, 1)
    assert exp.n_palindromes > 0


def test_long_chain_and_two_circles(oracle):
    exp = check(oracle, "circles", circles_stream(31), 31, 1)
    assert sorted(exp.table["rows"].tolist()) == [4096, 4097, 20000] and exp.table["edges"].tolist().count(2) == 2


@pytest.mark.parametrize("k", COMPONENTS_STREAM_K)
def test_components_stream(oracle, k):
    exp = restated_stream(oracle, k)
    exp.check_facts()
    exp.check_component_facts()
    print("components stream", k, exp.component_summary())
    assert exp.component_summary() == COMPONENTS_STREAM_STATS(k)
    big = int(np.argmax(exp.table["unitigs"]))
    assert exp.table["unitigs"][big] == 121 and sorted(exp.table["unitigs"].tolist()) == [1, 1, 1, 1, 17, 121]
    # the comb: its backbone pieces are a path of 61 unitigs (diameter >= 50), and their numbers are scattered along it
    members = [u for u in range(len(exp.paths)) if exp.comp[u] == big]
    nbr = {u: {V >> 1 for t in (0, 1) for V in exp.edges[2 * u + t]} - {u} for u in members}
    def far(src):
        dist, todo = {src: 0}, [src]
        while todo:
            nxt = []
            for x in todo:
                for y in nbr[x]:
                    if y not in dist:
                        dist[y] = dist[x] + 1
                        nxt.append(y)
            todo = nxt
        return max(dist.items(), key=lambda kv: kv[1])
    a, _ = far(members[0])
    _, diameter = far(a)
    assert diameter >= 50, diameter
    assert sum(1 for u in members if any(abs(u - w) > 10 for w in nbr[u])) > 60, "neighbours on the path are far apart in number"
    new, st = exp.drop(2 * k)
    assert drop_summary(st) == COMPONENTS_STREAM_DROP(k)
    assert new.component_summary() == (3, 1, 121, 61 * (k + 3) + 61)
    # the mean abundance of the chain is 3: with max_abundance = 2 it stays, with 3 it goes
    assert drop_summary(exp.small(2 * k, 2)[2]) == (2, 2, k + 1)
    assert drop_summary(exp.small(2 * k, 3)[2]) == (3, 3, k + 11)
    assert drop_summary(exp.small(1)[2]) == (0, 0, 0) and drop_summary(exp.small(2)[2]) == (1, 1, 1)
    assert exp.small(10 ** 6)[2]["n_rows_left"] == 0
