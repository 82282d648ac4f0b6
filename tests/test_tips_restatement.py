"""The tip rule of include/dskgpu.h ("tip clipping"), restated on the Python lists of the edge restatement and checked on the CPU before
tests/test_gpu_tips.py trusts it on the device: candidates, siblings, stronger, tip and outranked are applied literally, a round removes
the rows of all tips and the kept rows are restated from scratch.  On the oracle's solid rows (global order) the rounds give the numbers
fixed for these inputs (the CPU prototype of the rule gave the same ones), and what follows from the rule holds on every input: tip is a
subset of cand, outranked of tip, the clipped rows are whole unitigs, and a second clip of the rows left clips nothing."""
import os

import numpy as np
import pytest

pytest.importorskip("torch")          # (the GPU modules imported below import it at the top)
from tests.test_gpu_unitigs import GOLDEN, handmade_stream, revcomp_str      # noqa: E402
from tests.test_unitig_edges_restatement import EDGES_PINNED, EdgeRestatement      # noqa: E402
from tests.test_unitigs_restatement import solid_rows      # noqa: E402

CAND, TIP, OUTRANKED = 1, 2, 4


class TipRestatement(EdgeRestatement):
    """EdgeRestatement + one round of the tip rule, by the definition."""

    def __init__(self, values, ab, k, max_nodes, max_abundance=0):
        super().__init__(values, ab, k)
        assert 1 <= max_nodes <= 65535
        nu = len(self.paths)
        L = [int(self.offsets[u + 1] - self.offsets[u]) - k for u in range(nu)]
        S = [int(x) for x in self.ab_sum]
        E = self.edges
        deg = [len(e) for e in E]
        cand = [self.kind[u] == 0 and L[u] <= max_nodes and ((deg[2 * u] == 0) != (deg[2 * u + 1] == 0))
                and (max_abundance == 0 or S[u] <= max_abundance * L[u]) for u in range(nu)]

        def stronger(w, u):
            return S[w] * L[u] > S[u] * L[w] or (S[w] * L[u] == S[u] * L[w] and L[w] > L[u])

        self.siblings = {}
        bits = np.zeros(nu, dtype=np.uint8)
        for u in range(nu):
            if not cand[u]:
                continue
            A = 2 * u if deg[2 * u] else 2 * u + 1
            sib = sorted({X >> 1 for V in E[A] for X in E[V ^ 1]} - {u})
            self.siblings[u] = sib
            tip = any(not cand[w] or stronger(w, u) for w in sib)
            outranked = tip and not any(not cand[w] for w in sib)
            bits[u] = CAND | (TIP if tip else 0) | (OUTRANKED if outranked else 0)
        self.L, self.S = L, S
        self.bits = bits
        self.row_tip = ((bits[self.unitig] >> 1) & 1).astype(np.uint8) if self.n else np.zeros(0, np.uint8)
        clipped = int(self.row_tip.sum())
        self.tip_stats = dict(n_candidates=int((bits & CAND != 0).sum()), n_tips=int((bits & TIP != 0).sum()),
                              n_outranked=int((bits & OUTRANKED != 0).sum()), n_rows_clipped=clipped, n_rounds=1, n_rows_left=self.n - clipped)

    def round_summary(self):
        s = self.tip_stats
        return (self.n, self.stats["n_unitigs"], s["n_candidates"], s["n_tips"], s["n_outranked"], s["n_rows_clipped"])

    def check_tip_facts(self):
        b = self.bits
        assert not ((b & TIP != 0) & (b & CAND == 0)).any(), "tip is a subset of cand"
        assert not ((b & OUTRANKED != 0) & (b & TIP == 0)).any(), "outranked is a subset of tip"
        tips = set(np.nonzero(b & TIP)[0].tolist())
        assert self.tip_stats["n_rows_clipped"] == sum(self.L[u] for u in tips), "the clipped rows are whole unitigs"
        for u, (path, _) in enumerate(self.paths):
            assert all(self.row_tip[p >> 1] == (1 if u in tips else 0) for p in path)
        for u in tips:                                                       # the consequences the header names
            assert self.siblings[u], "a dead start that forks has no sibling and is never clipped"
            assert len(self.edges[2 * u]) + len(self.edges[2 * u + 1]) > 0, "an isolated unitig is never clipped"


class Clipped:
    """rounds: one round_summary per round that ran (the last one found no tip unless max_rounds stopped the loop); first / last: the
    restatements of the rows before the first and after the last round; values / ab: the rows left, in their order"""


def clip(values, ab, k, max_nodes, max_abundance=0, max_rounds=0):
    out = Clipped()
    out.rounds, out.first = [], None
    out.total = dict(n_candidates=0, n_tips=0, n_outranked=0, n_rows_clipped=0, n_rounds=0)
    values, ab = list(values), [int(a) for a in ab]
    while True:
        exp = TipRestatement(values, ab, k, max_nodes, max_abundance)
        exp.check_tip_facts()
        if out.first is None:
            out.first = exp
        out.last = exp
        if out.total["n_rounds"] == (max_rounds or 64):
            break
        out.rounds.append(exp.round_summary())
        for name in ("n_candidates", "n_tips", "n_outranked", "n_rows_clipped"):
            out.total[name] += exp.tip_stats[name]
        if exp.tip_stats["n_tips"] == 0:
            break
        out.total["n_rounds"] += 1
        keep = exp.row_tip == 0
        values = [v for v, f in zip(values, keep) if f]
        ab = [a for a, f in zip(ab, keep) if f]
    out.values, out.ab = values, ab
    out.total["n_rows_left"] = len(values)
    return out


def tips_stream(k):
    rng = np.random.default_rng(5000 + k)
    def rnd(n): return "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    def other(c): return "ACGT"[("ACGT".index(c) + 1) % 4]
    def other2(c): return "ACGT"[("ACGT".index(c) + 2) % 4]
    M = rnd(3 * k + 200); reads = [M, M]
    a = k + 60; X = other(M[a]) + rnd(9); stem = M[a - (k - 1): a] + X
    y = rnd(1); Y1 = y + rnd(3); Y2 = other(y) + rnd(6)
    reads += [stem + Y1, stem + Y2, stem + Y2]
    b = 2 * k + 120; Z = rnd(7) + other2(M[b - 1])
    reads += [revcomp_str(Z + M[b: b + k - 1])]
    return np.frombuffer(("\n".join(reads) + "\n").encode(), dtype=np.uint8).copy(), M


TIPS_STREAM_K = [15, 16, 31, 32, 33, 64, 65, 96, 97, 128]
# the tips stream at every k, max_nodes = max(k, 31), per round (unitigs, tips, outranked, rows clipped): the weak end of the fork goes first,
# outranked by the strong one, with the plain tip; then the branch, now one unitig; then nothing is left to clip but M
TIPS_STREAM_ROUNDS = [(7, 2, 1, 12), (3, 1, 0, 17), (1, 0, 0, 0)]
# golden reads, (k, abundance_min, max_nodes, max_abundance): per round (rows, unitigs, candidates, tips, outranked, rows clipped) -- the
# last round finds no tip --, fixed on the CPU, whatever the row order.  The unitigs of the last round are what is left.
TIPS_PINNED = {
    (31, 2, 31, 0): [(13096, 442, 147, 147, 0, 1758), (11338, 153, 0, 0, 0, 0)],
    (15, 2, 15, 0): [(13000, 719, 185, 184, 0, 1304), (11696, 356, 1, 0, 0, 0)],
    (63, 2, 63, 0): [(10945, 125, 35, 35, 0, 429), (10516, 55, 0, 0, 0, 0)],
    (15, 1, 15, 0): [(66281, 9505, 1086, 1084, 2, 8172), (58109, 7807, 2, 2, 0, 28), (58081, 7804, 0, 0, 0, 0)],
    (31, 1, 31, 1): [(99957, 7859, 2040, 2028, 10, 31164), (68793, 4386, 2, 0, 0, 0)],
}

_clipped = {}


def clipped_golden(oracle, golden_dir, k, amin, max_nodes, max_abundance):
    """clip() of the oracle's rows of the golden reads (global order), computed once and never changed"""
    key = (k, amin, max_nodes, max_abundance)
    if key not in _clipped:
        stream = np.ascontiguousarray(oracle.load_bank(os.path.join(golden_dir, GOLDEN))[0])
        values, ab = solid_rows(oracle, stream, k, amin)
        _clipped[key] = clip(values, ab, k, max_nodes, max_abundance)
    return _clipped[key]


def clipped_tips_stream(oracle, k):
    key = ("tips", k)
    if key not in _clipped:
        values, ab = solid_rows(oracle, tips_stream(k)[0], k, 1)
        _clipped[key] = clip(values, ab, k, max(k, 31))
    return _clipped[key]


def check_clip_facts(c, k, max_nodes, max_abundance=0):
    """what holds for every clip(): the sums, and a second clip of the rows left clips nothing"""
    assert c.total["n_rows_left"] == len(c.values) == c.last.n == c.first.n - c.total["n_rows_clipped"]
    assert c.total["n_rounds"] == sum(1 for r in c.rounds if r[3] > 0)
    assert c.last.tip_stats["n_tips"] == 0
    again = clip(c.values, c.ab, k, max_nodes, max_abundance)
    assert again.total["n_rounds"] == 0 and again.total["n_rows_clipped"] == 0 and again.values == c.values


@pytest.mark.parametrize("k", TIPS_STREAM_K)
def test_tips_stream(oracle, k):
    c = clipped_tips_stream(oracle, k)
    print("tips stream", k, c.rounds, c.total)
    assert [(r[1], r[3], r[4], r[5]) for r in c.rounds] == TIPS_STREAM_ROUNDS
    assert c.total["n_rounds"] == 2 and c.total["n_rows_clipped"] == 29
    M = tips_stream(k)[1]
    m_values, _ = solid_rows(oracle, np.frombuffer((M + "\n").encode(), dtype=np.uint8).copy(), k, 1)
    assert c.values == m_values                                             # exactly the rows of M alone
    assert c.last.seq(0) in (M, revcomp_str(M))
    check_clip_facts(c, k, max(k, 31))


@pytest.mark.parametrize("k,amin,max_nodes,max_abundance", sorted(TIPS_PINNED))
def test_golden_reads(oracle, golden_dir, k, amin, max_nodes, max_abundance):
    c = clipped_golden(oracle, golden_dir, k, amin, max_nodes, max_abundance)
    print("tips golden", (k, amin, max_nodes, max_abundance), c.rounds, c.total)
    assert c.rounds == TIPS_PINNED[(k, amin, max_nodes, max_abundance)]
    check_clip_facts(c, k, max_nodes, max_abundance)


@pytest.mark.parametrize("k", sorted(k for kind, k, _ in EDGES_PINNED if kind == "hand"))
def test_handmade_stream_has_no_tips(oracle, k):
    values, ab = solid_rows(oracle, handmade_stream(k), k, 1)
    c = clip(values, ab, k, max(k, 31))
    assert len(c.rounds) == 1 and c.rounds[0][3:] == (0, 0, 0) and c.values == values
    check_clip_facts(c, k, max(k, 31))


def test_max_rounds_stops_the_loop(oracle):
    values, ab = solid_rows(oracle, tips_stream(31)[0], 31, 1)
    c = clip(values, ab, 31, 31, max_rounds=1)
    assert c.total["n_rounds"] == 1 and c.total["n_rows_clipped"] == 12 and c.last.stats["n_unitigs"] == 3 and len(c.rounds) == 1
