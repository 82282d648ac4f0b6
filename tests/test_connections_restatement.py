"""The erroneous-connection rule of include/dskgpu.h ("erroneous connections"), restated on the Python lists of the edge restatement and
checked on the CPU before tests/test_gpu_connections.py trusts it on the device: candidate, flank, weak, removed and one-sided are applied
literally, a round removes the rows of all removed unitigs and the kept rows are restated from scratch; simplify_all() runs clip() of
tests/test_tips_restatement.py, pop() of tests/test_bubbles_restatement.py and remove() in turn.  What follows from min_ratio >= 2 is
asserted on every input the restatement sees: every removed unitig has, at both ends, a flank unitig that stays in that round and
satisfies the inequality; removed is a subset of the candidates; the removed rows are whole unitigs.  On the oracle's solid rows (global
order) the rounds give the numbers fixed for these inputs.  On the connections stream the rule alone removes the five connections and
keeps every row of M1 and M2; with the tip rule in front (simplify_all with the stream's parameters) M2 loses its head of 2 k rows to the
tips and c1 stays as part of M2's path -- test_connections_stream asserts both."""
import numpy as np
import pytest

pytest.importorskip("torch")          # (the GPU modules imported below import it at the top)
from tests.test_bubbles_restatement import (BUBBLE_NAMES, BUBBLES_STREAM_K, TIP_NAMES, pop, popped_golden, rows_of, simplify,      # noqa: E402
                                            stream_params)
from tests.test_gpu_unitigs import revcomp_str      # noqa: E402
from tests.test_tips_restatement import clip      # noqa: E402
from tests.test_unitig_edges_restatement import EdgeRestatement      # noqa: E402
from tests.test_unitigs_restatement import solid_rows      # noqa: E402

CAND, REM, WEAK0, WEAK1 = 1, 2, 4, 8
CONNECTION_NAMES = ("n_candidates", "n_one_sided", "n_removed", "n_rows_removed", "n_rounds")


class ConnectionRestatement(EdgeRestatement):
    """EdgeRestatement + one round of the erroneous-connection rule, by the definition."""

    def __init__(self, values, ab, k, max_nodes, min_ratio=4, max_abundance=0):
        super().__init__(values, ab, k)
        assert 1 <= max_nodes <= 65535 and 2 <= min_ratio <= 255
        nu = len(self.paths)
        L = [int(self.offsets[u + 1] - self.offsets[u]) - k for u in range(nu)]
        S = [int(x) for x in self.ab_sum]
        E = self.edges
        deg = [len(e) for e in E]
        cand = [self.kind[u] == 0 and L[u] <= max_nodes and deg[2 * u] >= 1 and deg[2 * u + 1] >= 1
                and all(V >> 1 != u for V in E[2 * u] + E[2 * u + 1])
                and (max_abundance == 0 or S[u] <= max_abundance * L[u]) for u in range(nu)]

        def heavier(w, u):
            return S[w] * L[u] > min_ratio * S[u] * L[w]

        self.flank = {}                                                      # flank[A] of both ends of every candidate
        bits = np.zeros(nu, dtype=np.uint8)
        for u in range(nu):
            if not cand[u]:
                continue
            weak = []
            for A in (2 * u, 2 * u + 1):
                fl = {V >> 1 for V in E[A]} | {X >> 1 for V in E[A] for X in E[V ^ 1]}
                self.flank[A] = sorted(fl - {u})
                weak.append(any(heavier(w, u) for w in self.flank[A]))
            bits[u] = CAND | (REM if weak[0] and weak[1] else 0) | (WEAK0 if weak[0] else 0) | (WEAK1 if weak[1] else 0)
        self.L, self.S, self.deg, self.heavier, self.min_ratio = L, S, deg, heavier, min_ratio
        self.bits = bits
        self.row_rem = ((bits[self.unitig] >> 1) & 1).astype(np.uint8) if self.n else np.zeros(0, np.uint8)
        removed = int(self.row_rem.sum())
        one_sided = (bits & CAND != 0) & ((bits & WEAK0 != 0) != (bits & WEAK1 != 0))
        self.connection_stats = dict(n_candidates=int((bits & CAND != 0).sum()), n_one_sided=int(one_sided.sum()), n_removed=int((bits & REM != 0).sum()),
                                     n_rows_removed=removed, n_rounds=1, n_rows_left=self.n - removed)

    def round_summary(self):
        s = self.connection_stats
        return (self.n, self.stats["n_unitigs"], s["n_candidates"], s["n_one_sided"], s["n_removed"], s["n_rows_removed"])

    def check_connection_facts(self):
        b = self.bits
        assert not ((b & (REM | WEAK0 | WEAK1) != 0) & (b & CAND == 0)).any(), "removed and weak are subsets of cand"
        assert ((b & REM != 0) == ((b & WEAK0 != 0) & (b & WEAK1 != 0))).all(), "removed <=> weak at both ends"
        removed = set(np.nonzero(b & REM)[0].tolist())
        assert self.connection_stats["n_rows_removed"] == sum(self.L[u] for u in removed), "the removed rows are whole unitigs"
        for u, (path, _) in enumerate(self.paths):
            assert all(self.row_rem[p >> 1] == (1 if u in removed else 0) for p in path)
        for u in removed:
            assert self.deg[2 * u] >= 1 and self.deg[2 * u + 1] >= 1, "a dead end is never removed"
            for A in (2 * u, 2 * u + 1):
                assert len(self.flank[A]) <= 20
                assert any(w not in removed and self.heavier(w, u) for w in self.flank[A]), ("a removed unitig has a flank unitig that stays", u, A)
                for w in self.flank[A]:                                      # min_ratio >= 2: never each the reason for the other
                    assert not (self.heavier(w, u) and self.heavier(u, w))


class Removed:
    """rounds: one round_summary per round that ran (the last one removed nothing unless max_rounds stopped the loop); first / last: the
    restatements of the rows before the first and after the last round; values / ab: the rows left, in their order"""


def remove(values, ab, k, max_nodes, min_ratio=4, max_abundance=0, max_rounds=0):
    out = Removed()
    out.rounds, out.first = [], None
    out.total = dict(n_candidates=0, n_one_sided=0, n_removed=0, n_rows_removed=0, n_rounds=0)
    values, ab = list(values), [int(a) for a in ab]
    while True:
        exp = ConnectionRestatement(values, ab, k, max_nodes, min_ratio, max_abundance)
        exp.check_connection_facts()
        if out.first is None:
            out.first = exp
        out.last = exp
        if out.total["n_rounds"] == (max_rounds or 64):
            break
        out.rounds.append(exp.round_summary())
        for name in ("n_candidates", "n_one_sided", "n_removed", "n_rows_removed"):
            out.total[name] += exp.connection_stats[name]
        if exp.connection_stats["n_removed"] == 0:
            break
        out.total["n_rounds"] += 1
        keep = exp.row_rem == 0
        values = [v for v, f in zip(values, keep) if f]
        ab = [a for a, f in zip(ab, keep) if f]
    out.values, out.ab = values, ab
    out.total["n_rows_left"] = len(values)
    return out


class SimplifiedAll:
    """passes: per pass that ran (the rounds of its clip(), of its pop(), of its remove(); None for a part that is skipped); total: what
    dskgpu_simplify_all reports; last: the restatement of the rows left (an EdgeRestatement at least); values / ab: the rows left"""


def simplify_all(values, ab, k, tips=None, bubbles=None, connections=None, max_passes=0):
    """tips: (max_nodes, max_abundance), bubbles: (max_nodes, max_diff), connections: (max_nodes, min_ratio, max_abundance); None = no such part"""
    assert tips is not None or bubbles is not None or connections is not None
    out = SimplifiedAll()
    out.passes = []
    tsum, bsum, csum = dict.fromkeys(TIP_NAMES, 0), dict.fromkeys(BUBBLE_NAMES, 0), dict.fromkeys(CONNECTION_NAMES, 0)
    n_passes = 0
    values, ab = list(values), [int(a) for a in ab]
    out.last = None
    for _ in range(max_passes or 16):
        n_before = len(values)
        c = p = r = None
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
        if connections is not None:
            r = remove(values, ab, k, connections[0], connections[1], connections[2])
            values, ab, out.last = r.values, r.ab, r.last
            for name in CONNECTION_NAMES:
                csum[name] += r.total[name]
        out.passes.append((c.rounds if c else None, p.rounds if p else None, r.rounds if r else None))
        if len(values) == n_before:
            break
        n_passes += 1
    tsum["n_rows_left"] = bsum["n_rows_left"] = csum["n_rows_left"] = len(values)
    out.total = dict(n_passes=n_passes, n_rows_left=len(values), tips=tsum, bubbles=bsum, connections=csum)
    out.values, out.ab = values, ab
    return out


CONNECTIONS = ("c1", "c5", "c6", "c10", "c11")                            # the pieces of the connections stream that the rule removes


def connections_stream(k):
    """-> (the reads, the pieces by name).  Three random strands: M1 read 12 times (its tail 30 times), M2 20 times, M3 once.  Between them,
    k + 4 bases apart, short pieces that hold only the windows crossing a junction: c1 (read once, removed), c2 (3 times: 12 > 4 * 3 is
    false, one-sided, stays), c3 (once, into M3 that is read once: one-sided, stays), c4 (2 k + 1 rows: no candidate), c6 (2 k rows:
    removed), c5 (given as a reverse complement: removed), c10 (4 times: not weak on M1 before c11, 6 bases on, is gone and the stretch
    between them has merged into M1's tail: round 2) and c11 (once: removed in round 1).  The bases at each junction are chosen so that
    no junction window equals a k-mer of the strands."""
    rng = np.random.default_rng(9000 + k)
    def rnd(n): return ["ACGT"[i] for i in rng.integers(0, 4, n)]
    def other(c): return "ACGT"[("ACGT".index(c) + 1) % 4]
    a = [2 * k + i * (k + 4) for i in range(7)]; b = a
    p10, p11 = a[6], a[6] + 6
    M1 = rnd(p11 + 3 * k); M2 = rnd(b[6] + 3 * k); M3 = rnd(5 * k)
    for p, q in ((a[0], b[0]), (a[1], b[1]), (p10, b[5]), (p11, b[6])):      # M1 -> M2, no middle
        M2[q] = other(M1[p]); M2[q - 1] = other(M1[p - 1])
    M3[2 * k] = other(M1[a[2]]); M3[2 * k - 1] = other(M1[a[2] - 1])        # M1 -> M3
    M2[b[4]] = other(M1[a[5]]); M2[b[4] - 1] = other(M1[a[5] - 1])          # M2 -> M1
    M1, M2, M3 = "".join(M1), "".join(M2), "".join(M3)

    def join(A, p, B, q, n_mid=0):      # only the windows that cross the junction: k - 1 + n_mid rows
        mid = rnd(n_mid)
        if n_mid:
            mid[0] = other(A[p]); mid[-1] = other(B[q - 1])
        return A[p - (k - 1): p] + "".join(mid) + B[q: q + k - 1]
    c1 = join(M1, a[0], M2, b[0])
    c2 = join(M1, a[1], M2, b[1])
    c3 = join(M1, a[2], M3, 2 * k)
    c4 = join(M2, b[2], M1, a[3], k + 2)
    c6 = join(M2, b[3], M1, a[4], k + 1)
    c5 = revcomp_str(join(M2, b[4], M1, a[5]))
    c10 = join(M1, p10, M2, b[5])
    c11 = join(M1, p11, M2, b[6])
    extra = M1[p11 - k + 1:]
    reads = [M1] * 12 + [M2] * 20 + [M3, c1] + [c2] * 3 + [c3, c4, c6, c5] + [c10] * 4 + [c11] + [extra] * 18
    parts = dict(M1=M1, M2=M2, M3=M3, c1=c1, c2=c2, c3=c3, c4=c4, c5=c5, c6=c6, c10=c10, c11=c11)
    return np.frombuffer(("\n".join(reads) + "\n").encode(), dtype=np.uint8).copy(), parts


def stream_params_all(k):
    """(tips, bubbles, connections) for the connections stream: those of the bubbles stream, and connections of up to 2 k rows, min_ratio 4"""
    return stream_params(k) + ((2 * k, 4, 0),)


# the connections stream at every k, per round of one remove() of all its rows: (unitigs, candidates, one-sided, removed, rows removed)
def CONNECTIONS_STREAM_ROUNDS(k): return [(27, 18, 3, 4, 5 * k - 3), (15, 5, 2, 1, k - 1), (12, 4, 2, 0, 0)]


# ... and with other parameters, without the rows: (unitigs, candidates, one-sided, removed)
CONNECTIONS_STREAM_OTHER = {
    "min_ratio = 2": [(27, 18, 2, 6), (9, 1, 1, 0)],
    "min_ratio = 5": [(27, 18, 2, 4), (15, 5, 3, 0)],
    "max_nodes = 2 k - 1": [(27, 17, 3, 3), (18, 8, 2, 1), (15, 6, 2, 0)],
}
# golden reads, (k, abundance_min): the rounds of one remove() on the rows that popped_golden() leaves, with max_nodes = 2 k and min_ratio = 4;
# per round (rows, unitigs, candidates, one-sided, removed, rows removed) -- the last round removes nothing --, fixed on the CPU, whatever
# the row order
CONNECTIONS_PINNED = {
    (31, 2): [(10532, 75, 8, 0, 3, 93), (10439, 66, 0, 0, 0, 0)],
    (15, 2): [(10646, 150, 105, 0, 42, 630), (10016, 27, 0, 0, 0, 0)],
    (16, 2): [(10671, 144, 97, 0, 39, 624), (10047, 30, 0, 0, 0, 0)],
    (21, 2): [(10459, 79, 34, 0, 13, 273), (10186, 40, 0, 0, 0, 0)],
    (63, 2): [(10516, 55, 0, 0, 0, 0)],
    (15, 1): [(57751, 7780, 7699, 263, 2777, 43542), (14209, 694, 527, 263, 0, 0)],
}

_done = {}


def stream_rows(oracle, k):
    if ("rows", k) not in _done:
        stream, parts = connections_stream(k)
        _done[("rows", k)] = solid_rows(oracle, stream, k, 1) + (parts,)
    return _done[("rows", k)]


def removed_golden(oracle, golden_dir, k, amin):
    """remove() of the rows that popped_golden() leaves of the golden reads (global order), computed once and never changed"""
    if (k, amin) not in _done:
        p = popped_golden(oracle, golden_dir, k, amin)
        _done[(k, amin)] = remove(p.values, p.ab, k, 2 * k, 4)
    return _done[(k, amin)]


def check_remove_facts(r, k, max_nodes, min_ratio=4, max_abundance=0):
    """what holds for every remove(): the sums, and a second remove of the rows left removes nothing"""
    assert r.total["n_rows_left"] == len(r.values) == r.last.n == r.first.n - r.total["n_rows_removed"]
    assert r.total["n_rounds"] == sum(1 for x in r.rounds if x[4] > 0)
    assert r.last.connection_stats["n_removed"] == 0
    again = remove(r.values, r.ab, k, max_nodes, min_ratio, max_abundance)
    assert again.total["n_rounds"] == 0 and again.total["n_rows_removed"] == 0 and again.values == r.values


@pytest.mark.parametrize("k", BUBBLES_STREAM_K)
def test_connections_stream(oracle, k):
    values, ab, parts = stream_rows(oracle, k)
    r = remove(values, ab, k, 2 * k, 4)
    print("connections stream", k, r.rounds, r.total)
    assert [x[1:] for x in r.rounds] == CONNECTIONS_STREAM_ROUNDS(k)
    assert r.total["n_rounds"] == 2 and r.total["n_removed"] == 5 and r.total["n_rows_removed"] == 6 * k - 4
    assert r.last.stats["n_unitigs"] == 12
    check_remove_facts(r, k, 2 * k)
    gone = sorted(v for name in CONNECTIONS for v in rows_of(oracle, [parts[name]], k))
    assert len(gone) == 6 * k - 4 and sorted(set(values) - set(r.values)) == gone
    # simplify alone: 4 k rows and none of the connections
    tp, bp, cp = stream_params_all(k)
    s = simplify(values, ab, k, tp, bp)
    assert len(values) - len(s.values) == 4 * k and not set(gone) - set(s.values)
    # the new rule alone, as passes: no row of the five connections is left, every row of M1 and M2 is
    only = simplify_all(values, ab, k, None, None, cp)
    assert only.values == r.values and only.total["n_passes"] == 1 and only.total["connections"] == r.total | dict(n_candidates=r.total["n_candidates"] + 4, n_one_sided=r.total["n_one_sided"] + 2)
    assert not set(gone) & set(only.values) and not set(rows_of(oracle, [parts["M1"], parts["M2"]], k)) - set(only.values)
    # all three rules.  The tip rule runs first and clips the two heads of 2 k rows that a connection runs into: M3's before c3 and M2's
    # before c1 -- c1 is no tip candidate, which makes it a sibling that counts as solid.  With M2's head gone c1 is the only way into the
    # rest of M2 and compacts into one unitig with it, so c1 stays; c5, c6, c10 and c11 go as before and every row of M1 is left
    sa = simplify_all(values, ab, k, tp, bp, cp)
    print("simplify_all", k, sa.passes, sa.total)
    left = set(sa.values)
    assert not set(v for name in ("c5", "c6", "c10", "c11") for v in rows_of(oracle, [parts[name]], k)) & left
    assert not set(rows_of(oracle, [parts["M1"], parts["c1"]], k)) - left
    assert sorted(set(rows_of(oracle, [parts["M2"]], k)) - left) == sorted(rows_of(oracle, [parts["M2"][: 3 * k - 1]], k))
    assert sa.total["n_rows_left"] == len(sa.values) == sa.last.n == len(values) - 4 * k - (5 * k - 3)
    assert sa.total["n_passes"] == 1 and len(sa.passes) == 2
    assert {n: sa.total["tips"][n] for n in ("n_tips", "n_rows_clipped", "n_rounds")} == dict(n_tips=2, n_rows_clipped=4 * k, n_rounds=1)
    assert sa.total["bubbles"]["n_popped"] == 0
    assert {n: sa.total["connections"][n] for n in ("n_removed", "n_rows_removed", "n_rounds")} == dict(n_removed=4, n_rows_removed=5 * k - 3, n_rounds=2)


@pytest.mark.parametrize("k", [15, 32, 65])
def test_other_parameters_on_the_stream(oracle, k):
    values, ab, _ = stream_rows(oracle, k)
    one = remove(values, ab, k, 2 * k, 4, max_rounds=1)
    assert one.total["n_rounds"] == 1 and one.total["n_removed"] == 4 and len(one.rounds) == 1 and one.last.stats["n_unitigs"] == 15
    for name, args in (("min_ratio = 2", (2 * k, 2)), ("min_ratio = 5", (2 * k, 5)), ("max_nodes = 2 k - 1", (2 * k - 1, 4))):
        r = remove(values, ab, k, *args)
        print("connections stream", k, name, r.rounds)
        assert [x[1:5] for x in r.rounds] == CONNECTIONS_STREAM_OTHER[name], name
        check_remove_facts(r, k, *args)
    # a limit on the mean abundance: 1 keeps the pieces read once, and c10 (read 4 times) is no candidate in any round
    r = remove(values, ab, k, 2 * k, 4, max_abundance=1)
    assert r.total["n_removed"] == 4 and r.total["n_rounds"] == 1 and r.last.stats["n_unitigs"] == 15


@pytest.mark.parametrize("k,amin", sorted(CONNECTIONS_PINNED))
def test_golden_reads(oracle, golden_dir, k, amin):
    r = removed_golden(oracle, golden_dir, k, amin)
    print("connections golden", (k, amin), r.rounds, r.total)
    assert r.rounds == CONNECTIONS_PINNED[(k, amin)]
    check_remove_facts(r, k, 2 * k)


@pytest.mark.parametrize("k,amin", [(12, 2), (32, 2), (64, 2)])
def test_the_facts_hold_where_there_are_palindromes(oracle, golden_dir, k, amin):
    """no numbers pinned: check_connection_facts runs on every round (even k: palindromes among the rows)"""
    r = removed_golden(oracle, golden_dir, k, amin)
    check_remove_facts(r, k, 2 * k)


@pytest.mark.parametrize("k", [15, 31])
def test_without_connections_simplify_all_is_simplify(oracle, k):
    values, ab, _ = stream_rows(oracle, k)
    tp, bp, cp = stream_params_all(k)
    s, sa = simplify(values, ab, k, tp, bp), simplify_all(values, ab, k, tp, bp, None)
    assert sa.values == s.values and sa.ab == s.ab and [x[:2] for x in sa.passes] == s.passes
    assert {n: sa.total[n] for n in ("n_passes", "n_rows_left", "tips", "bubbles")} == s.total
    assert sa.total["connections"] == dict(dict.fromkeys(CONNECTION_NAMES, 0), n_rows_left=len(s.values))
    for one in (dict(tips=tp), dict(bubbles=bp)):
        s, sa = simplify(values, ab, k, one.get("tips"), one.get("bubbles")), simplify_all(values, ab, k, connections=None, **one)
        assert sa.values == s.values and sa.total["n_passes"] == s.total["n_passes"]
    only = simplify_all(values, ab, k, None, None, cp)                      # the new rule alone: remove(), then a pass that removes nothing
    assert only.total["n_passes"] == 1 and only.total["connections"]["n_removed"] == 5 and only.last.stats["n_unitigs"] == 12
    one = simplify_all(values, ab, k, tp, bp, cp, max_passes=1)
    assert one.total["n_passes"] == 1 and len(one.passes) == 1
