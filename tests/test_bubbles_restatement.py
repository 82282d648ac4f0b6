"""The bubble rule of include/dskgpu.h ("bubble popping"), restated on the Python lists of the edge restatement and checked on the CPU
before tests/test_gpu_bubbles.py trusts it on the device: candidates, siblings, stronger, popped and in-a-bubble are applied literally, a
round removes the rows of all popped unitigs and the kept rows are restated from scratch; simplify() alternates with clip() of
tests/test_tips_restatement.py.  What follows from the rule is asserted on every input the restatement sees: siblinghood is symmetric,
every popped unitig has a sibling that stays, equally strong branches all stay, every branch with a stronger sibling goes in the same
round, and a unitig with more than one edge at an end is never popped.  On the oracle's solid rows (global order) the rounds give the
numbers fixed for these inputs."""
import numpy as np
import pytest

pytest.importorskip("torch")          # (the GPU modules imported below import it at the top)
from tests.test_gpu_unitigs import revcomp_str      # noqa: E402
from tests.test_tips_restatement import TIPS_PINNED, clip, clipped_golden      # noqa: E402
from tests.test_unitig_edges_restatement import EdgeRestatement      # noqa: E402
from tests.test_unitigs_restatement import solid_rows      # noqa: E402

CAND, POP, IN_BUBBLE = 1, 2, 4
TIP_NAMES = ("n_candidates", "n_tips", "n_outranked", "n_rows_clipped", "n_rounds")
BUBBLE_NAMES = ("n_candidates", "n_in_bubbles", "n_popped", "n_rows_popped", "n_rounds")


class BubbleRestatement(EdgeRestatement):
    """EdgeRestatement + one round of the bubble rule, by the definition."""

    def __init__(self, values, ab, k, max_nodes, max_diff):
        super().__init__(values, ab, k)
        assert 1 <= max_nodes <= 65535 and max_diff >= 0
        nu = len(self.paths)
        L = [int(self.offsets[u + 1] - self.offsets[u]) - k for u in range(nu)]
        S = [int(x) for x in self.ab_sum]
        E = self.edges
        deg = [len(e) for e in E]
        cand = [self.kind[u] == 0 and L[u] <= max_nodes and deg[2 * u] == 1 and deg[2 * u + 1] == 1
                and E[2 * u][0] >> 1 != u and E[2 * u + 1][0] >> 1 != u for u in range(nu)]
        out = [E[2 * u][0] if cand[u] else None for u in range(nu)]
        inn = [E[2 * u + 1][0] if cand[u] else None for u in range(nu)]

        def stronger(w, u):
            return S[w] * L[u] > S[u] * L[w] or (S[w] * L[u] == S[u] * L[w] and L[w] > L[u])

        self.siblings = {}
        for u in range(nu):
            if not cand[u]:
                continue
            sib = set()
            for X in E[inn[u] ^ 1]:
                w = X >> 1
                if w != u and cand[w] and E[X][0] == out[u] and E[X ^ 1][0] == inn[u] and abs(L[w] - L[u]) <= max_diff:
                    sib.add(w)
            self.siblings[u] = sorted(sib)
        bits = np.zeros(nu, dtype=np.uint8)
        for u, sib in self.siblings.items():
            pop = any(stronger(w, u) for w in sib)
            bits[u] = CAND | (POP if pop else 0) | (IN_BUBBLE if sib else 0)
        self.L, self.S, self.deg, self.stronger = L, S, deg, stronger
        self.bits = bits
        self.row_pop = ((bits[self.unitig] >> 1) & 1).astype(np.uint8) if self.n else np.zeros(0, np.uint8)
        popped = int(self.row_pop.sum())
        self.bubble_stats = dict(n_candidates=int((bits & CAND != 0).sum()), n_in_bubbles=int((bits & IN_BUBBLE != 0).sum()),
                                 n_popped=int((bits & POP != 0).sum()), n_rows_popped=popped, n_rounds=1, n_rows_left=self.n - popped)

    def round_summary(self):
        s = self.bubble_stats
        return (self.n, self.stats["n_unitigs"], s["n_candidates"], s["n_in_bubbles"], s["n_popped"], s["n_rows_popped"])

    def check_bubble_facts(self):
        b = self.bits
        assert not ((b & POP != 0) & (b & IN_BUBBLE == 0)).any() and not ((b & IN_BUBBLE != 0) & (b & CAND == 0)).any(), "pop < in a bubble < cand"
        popped = set(np.nonzero(b & POP)[0].tolist())
        assert self.bubble_stats["n_rows_popped"] == sum(self.L[u] for u in popped), "the popped rows are whole unitigs"
        for u, (path, _) in enumerate(self.paths):
            assert all(self.row_pop[p >> 1] == (1 if u in popped else 0) for p in path)
        for u, sib in self.siblings.items():
            for w in sib:
                assert u in self.siblings[w], ("siblinghood is symmetric", u, w)
                assert not (self.stronger(w, u) and self.stronger(u, w))
            if u in popped:
                assert any(w not in popped for w in sib), ("a popped unitig has a sibling that stays", u, sib)
                assert self.deg[2 * u] == 1 and self.deg[2 * u + 1] == 1, "more than one edge at an end: never popped"
            else:                                                            # equally strong branches all stay; of three the two weaker go at once
                assert not any(self.stronger(w, u) for w in sib), ("every branch with a stronger sibling goes in the same round", u)


class Popped:
    """rounds: one round_summary per round that ran (the last one popped nothing unless max_rounds stopped the loop); first / last: the
    restatements of the rows before the first and after the last round; values / ab: the rows left, in their order"""


def pop(values, ab, k, max_nodes, max_diff=4, max_rounds=0):
    out = Popped()
    out.rounds, out.first = [], None
    out.total = dict(n_candidates=0, n_in_bubbles=0, n_popped=0, n_rows_popped=0, n_rounds=0)
    values, ab = list(values), [int(a) for a in ab]
    while True:
        exp = BubbleRestatement(values, ab, k, max_nodes, max_diff)
        exp.check_bubble_facts()
        if out.first is None:
            out.first = exp
        out.last = exp
        if out.total["n_rounds"] == (max_rounds or 64):
            break
        out.rounds.append(exp.round_summary())
        for name in ("n_candidates", "n_in_bubbles", "n_popped", "n_rows_popped"):
            out.total[name] += exp.bubble_stats[name]
        if exp.bubble_stats["n_popped"] == 0:
            break
        out.total["n_rounds"] += 1
        keep = exp.row_pop == 0
        values = [v for v, f in zip(values, keep) if f]
        ab = [a for a, f in zip(ab, keep) if f]
    out.values, out.ab = values, ab
    out.total["n_rows_left"] = len(values)
    return out


class Simplified:
    """passes: per pass that ran (the rounds of its clip(), the rounds of its pop()); total: what dskgpu_simplify reports; last: the
    restatement of the rows left (an EdgeRestatement at least); values / ab: the rows left"""


def simplify(values, ab, k, tips=None, bubbles=None, max_passes=0):
    """tips: (max_nodes, max_abundance) or None = no tip half; bubbles: (max_nodes, max_diff) or None = no bubble half"""
    assert tips is not None or bubbles is not None
    out = Simplified()
    out.passes = []
    tsum, bsum = dict.fromkeys(TIP_NAMES, 0), dict.fromkeys(BUBBLE_NAMES, 0)
    n_passes = 0
    values, ab = list(values), [int(a) for a in ab]
    out.last = None
    for _ in range(max_passes or 16):
        c = p = None
        if tips is not None:
            c = clip(values, ab, k, tips[0], tips[1])
            values, ab, out.last = c.values, c.ab, c.last
            for name in TIP_NAMES:
                tsum[name] += c.total[name]
        if bubbles is not None:
            p = pop(values, ab, k, bubbles[0], bubbles[1])
            values, ab, out.last = p.values, p.ab, p.last
            for name in BUBBLE_NAMES:
                bsum[name] += p.total[name]
        out.passes.append((c.rounds if c else None, p.rounds if p else None))
        if (c.total["n_rows_clipped"] if c else 0) + (p.total["n_rows_popped"] if p else 0) == 0:
            break
        n_passes += 1
    tsum["n_rows_left"] = bsum["n_rows_left"] = len(values)
    out.total = dict(n_passes=n_passes, n_rows_left=len(values), tips=tsum, bubbles=bsum)
    out.values, out.ab = values, ab
    return out


def bubbles_stream(k):
    """-> (the reads, M, the branches that stay).  M is read twice.  Along it, 2 k + 5 bases apart: a two-way SNP bubble whose weak branch
    is read once, as a reverse complement; a three-way bubble (two weak branches); a bubble of two equally strong branches; an insertion of
    6 bases read once (the lengths differ by 6 > max_diff); a branch read once that differs from M in two bases 6 apart, with a SNP read once
    between them (a bubble nested in the strong branch of another); and a dead-end branch, read twice, that carries a SNP bubble."""
    rng = np.random.default_rng(7000 + k)
    def rnd(n): return "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    def other(c): return "ACGT"[("ACGT".index(c) + 1) % 4]
    def other2(c): return "ACGT"[("ACGT".index(c) + 2) % 4]
    def snp(s, i, f=other): return s[: i] + f(s[i]) + s[i + 1:]
    def around(s, lo, hi): return s[lo - (k - 1): hi + k]                   # the windows that hold a base of s[lo .. hi]
    step = 2 * k + 5
    a = 3 * k + 10; b = a + step; c = b + step; d = c + step; d1 = d + step; e = d1 + 3; d2 = d1 + 6; f = d2 + step
    M = rnd(f + 3 * k + 12); reads = [M, M]
    reads += [revcomp_str(around(snp(M, a), a, a))]
    reads += [around(snp(M, b), b, b), around(snp(M, b, other2), b, b)]
    equal = around(snp(M, c), c, c); reads += [equal, equal]
    longer = M[d - (k - 1): d] + other(M[d]) + rnd(4) + other(M[d - 1]) + M[d: d + k - 1]; reads += [longer]
    reads += [around(snp(snp(M, d1), d2), d1, d2), around(snp(M, e), e, e)]
    B = M[f - (k - 1): f] + other(M[f]) + rnd(k + 5)                          # the dead-end branch: k + 6 windows; its SNP at base k + 2
    reads += [B, B, around(snp(B, k + 2), k + 2, k + 2)]
    return np.frombuffer(("\n".join(reads) + "\n").encode(), dtype=np.uint8).copy(), M, [equal, longer]


BUBBLES_STREAM_K = [15, 16, 31, 32, 33, 64, 65, 96, 97, 128]


def stream_params(k):
    """(tips, bubbles) for the bubbles stream: chains of up to 2 k rows on both sides, max_diff = 4"""
    return (2 * k, 0), (2 * k, 4)


# the bubbles stream at every k, per round of one pop() of all its rows: (unitigs, candidates, in bubbles, popped, (a, b): a k + b rows popped).
# Round 1: the weak branches of the SNP, of the three-way bubble (two of them), of the nested bubble and of the dead-end branch's bubble;
# round 2: the outer branch, now that the strong one is one unitig; round 3: nothing more -- the equal pair and the longer branch stay
BUBBLES_STREAM_ROUNDS = [(25, 14, 11, 5, (5, 0)), (12, 6, 4, 1, (1, 6)), (9, 4, 2, 0, (0, 0))]
# ... and per pass of simplify(): (its tip rounds as (unitigs, candidates, tips, (a, b) rows clipped), its bubble rounds as above).  Pass 1
# finds no tip: the end of the dead-end branch has no sibling while the branch forks.  Pass 2 clips the branch, one unitig of k + 6 rows
# now; pass 3 removes nothing
BUBBLES_STREAM_PASSES = [
    ([(25, 1, 0, (0, 0))], BUBBLES_STREAM_ROUNDS),
    ([(9, 1, 1, (1, 6)), (7, 0, 0, (0, 0))], [(7, 4, 2, 0, (0, 0))]),
    ([(7, 0, 0, (0, 0))], [(7, 4, 2, 0, (0, 0))]),
]
BUBBLES_STREAM_TOTAL = dict(n_passes=2, tips=dict(n_candidates=2, n_tips=1, n_outranked=0, n_rounds=1),
                            bubbles=dict(n_candidates=32, n_in_bubbles=21, n_popped=6, n_rounds=2))
# golden reads, (k, abundance_min): the rounds of one pop() on the rows that clip(.., max_nodes = k) leaves, with max_nodes = 2 k and
# max_diff = 4; per round (rows, unitigs, candidates, in bubbles, popped, rows popped) -- the last round pops nothing --, fixed on the CPU,
# whatever the row order.  At (15, 1) the ties at abundance 1 stay.
BUBBLES_PINNED = {
    (31, 2): [(11338, 153, 57, 52, 26, 806), (10532, 75, 5, 0, 0, 0)],
    (15, 2): [(11696, 356, 199, 140, 70, 1050), (10646, 150, 61, 2, 0, 0)],
    (16, 2): [(11743, 341, 189, 134, 67, 1072), (10671, 144, 57, 2, 0, 0)],
    (63, 2): [(10516, 55, 0, 0, 0, 0)],
    (15, 1): [(58081, 7804, 2524, 259, 22, 330), (57751, 7780, 2501, 216, 0, 0)],
}


def bubble_rounds_of(rounds, k):
    """the rounds of a pop() of the bubbles stream as BUBBLES_STREAM_ROUNDS writes them"""
    return [(r[1], r[2], r[3], r[4], ((r[5] - r[5] % k) // k, r[5] % k)) for r in rounds]


def tip_rounds_of(rounds, k):
    return [(r[1], r[2], r[3], ((r[5] - r[5] % k) // k, r[5] % k)) for r in rounds]


_done = {}


def popped_golden(oracle, golden_dir, k, amin):
    """pop() of the rows that clip(.., max_nodes = k) leaves of the golden reads (global order), computed once and never changed"""
    if (k, amin) not in _done:
        c = clipped_golden(oracle, golden_dir, k, amin, k, 0)
        _done[(k, amin)] = pop(c.values, c.ab, k, 2 * k, 4)
    return _done[(k, amin)]


def simplified_bubbles_stream(oracle, k):
    if ("stream", k) not in _done:
        values, ab = solid_rows(oracle, bubbles_stream(k)[0], k, 1)
        tp, bp = stream_params(k)
        _done[("stream", k)] = (pop(values, ab, k, *bp), simplify(values, ab, k, tp, bp))
    return _done[("stream", k)]


def rows_of(oracle, reads, k):
    return solid_rows(oracle, np.frombuffer(("\n".join(reads) + "\n").encode(), dtype=np.uint8).copy(), k, 1)[0]


def check_pop_facts(p, k, max_nodes, max_diff=4):
    """what holds for every pop(): the sums, and a second pop of the rows left pops nothing"""
    assert p.total["n_rows_left"] == len(p.values) == p.last.n == p.first.n - p.total["n_rows_popped"]
    assert p.total["n_rounds"] == sum(1 for r in p.rounds if r[4] > 0)
    assert p.last.bubble_stats["n_popped"] == 0
    again = pop(p.values, p.ab, k, max_nodes, max_diff)
    assert again.total["n_rounds"] == 0 and again.total["n_rows_popped"] == 0 and again.values == p.values


@pytest.mark.parametrize("k", BUBBLES_STREAM_K)
def test_bubbles_stream(oracle, k):
    p, s = simplified_bubbles_stream(oracle, k)
    print("bubbles stream", k, p.rounds, p.total, s.passes, s.total)
    assert bubble_rounds_of(p.rounds, k) == BUBBLES_STREAM_ROUNDS
    assert p.total["n_rounds"] == 2 and p.total["n_popped"] == 6 and p.total["n_rows_popped"] == 6 * k + 6
    check_pop_facts(p, k, 2 * k)
    assert [(tip_rounds_of(c, k), bubble_rounds_of(b, k)) for c, b in s.passes] == BUBBLES_STREAM_PASSES
    assert s.total["n_passes"] == 2 and s.total["n_rows_left"] == len(s.values)
    for half in ("tips", "bubbles"):
        assert {n: s.total[half][n] for n in BUBBLES_STREAM_TOTAL[half]} == BUBBLES_STREAM_TOTAL[half]
    assert s.total["tips"]["n_rows_clipped"] == k + 6 and s.total["bubbles"]["n_rows_popped"] == 6 * k + 6
    # what is left: the rows of M and of the branches the rule says stay -- the equal pair's and the one that is 6 rows longer
    _, M, stay = bubbles_stream(k)
    assert sorted(s.values) == sorted(rows_of(oracle, [M] + stay, k))
    assert len(s.values) == len(M) - k + 1 + k + (k + 5)
    assert s.last.stats["n_unitigs"] == 7


@pytest.mark.parametrize("k,amin", sorted(BUBBLES_PINNED))
def test_golden_reads(oracle, golden_dir, k, amin):
    if (k, amin, k, 0) in TIPS_PINNED:
        assert clipped_golden(oracle, golden_dir, k, amin, k, 0).rounds == TIPS_PINNED[(k, amin, k, 0)]
    p = popped_golden(oracle, golden_dir, k, amin)
    print("bubbles golden", (k, amin), p.rounds, p.total)
    assert p.rounds == BUBBLES_PINNED[(k, amin)]
    check_pop_facts(p, k, 2 * k)
    c = clip(p.values, p.ab, k, k)                                          # a final clip finds no tip
    assert c.total["n_rounds"] == 0 and c.total["n_tips"] == 0 and c.values == p.values


@pytest.mark.parametrize("k,amin", [(12, 2), (21, 2), (32, 2), (64, 2)])
def test_the_facts_hold_where_there_are_palindromes(oracle, golden_dir, k, amin):
    """no numbers pinned: check_bubble_facts runs on every round (even k: palindromes among the rows)"""
    p = popped_golden(oracle, golden_dir, k, amin)
    check_pop_facts(p, k, 2 * k)


def test_max_rounds_and_max_passes_stop_the_loops(oracle):
    k = 31
    values, ab = solid_rows(oracle, bubbles_stream(k)[0], k, 1)
    tp, bp = stream_params(k)
    p = pop(values, ab, k, *bp, max_rounds=1)
    assert p.total["n_rounds"] == 1 and p.total["n_popped"] == 5 and p.last.stats["n_unitigs"] == 12 and len(p.rounds) == 1
    s = simplify(values, ab, k, tp, bp, max_passes=1)
    assert s.total["n_passes"] == 1 and len(s.passes) == 1 and s.last.stats["n_unitigs"] == 9
    rest = simplify(s.values, s.ab, k, tp, bp)
    assert rest.total["n_passes"] == 1 and rest.total["tips"]["n_rows_clipped"] == k + 6 and rest.last.stats["n_unitigs"] == 7


def test_one_half_alone(oracle):
    k = 31
    values, ab = solid_rows(oracle, bubbles_stream(k)[0], k, 1)
    tp, bp = stream_params(k)
    s = simplify(values, ab, k, None, bp)
    assert s.total["n_passes"] == 1 and s.total["bubbles"]["n_popped"] == 6 and s.total["tips"]["n_candidates"] == 0
    s = simplify(values, ab, k, tp, None)
    assert s.total["n_passes"] == 0 and s.values == values
