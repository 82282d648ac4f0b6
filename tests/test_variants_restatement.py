"""Variant reporting (include/dskgpu.h: "variant reporting"), restated on STRINGS on top of the bubble restatement and checked on the CPU
before tests/test_gpu_variants.py trusts it on the device.  VariantRestatement applies the definitions literally through self.siblings,
self.edges and self.text_of: the pairs a < b, their readings, lcp / lcs / n_mismatch / kind of the two texts, the records, the stats, the
line offsets and the variant stream.  check_variant_facts asserts what follows from the definitions on every input it sees; with an oracle
it also counts the stream back.  The numbers pinned below were found on the CPU with this restatement on the oracle's solid rows (global
order); they were never read off the device."""
import os
from collections import Counter

import numpy as np
import pytest

pytest.importorskip("torch")          # (the GPU modules imported below import it at the top)
from tests.test_bubbles_restatement import BUBBLES_STREAM_K, BubbleRestatement, bubbles_stream, pop      # noqa: E402
from tests.test_gpu_unitigs import GOLDEN      # noqa: E402
from tests.test_tips_restatement import clipped_golden      # noqa: E402
from tests.test_unitigs_restatement import solid_rows      # noqa: E402

SNP, MULTI, INDEL, COMPLEX = 1, 2, 3, 4


def common_prefix(s, t):
    n = 0
    while n < min(len(s), len(t)) and s[n] == t[n]:
        n += 1
    return n


class VariantRestatement(BubbleRestatement):
    """BubbleRestatement + the variants of its siblings, by the definition."""

    def __init__(self, values, ab, k, max_nodes, max_diff):
        super().__init__(values, ab, k, max_nodes, max_diff)
        self.values = list(values)
        E, L = self.edges, self.L
        recs, lines = [], []
        self.per_unitig = Counter()
        for a in sorted(self.siblings):
            for b in self.siblings[a]:                                       # (sorted: ascending (a, b))
                assert a in self.siblings[b], ("siblinghood is symmetric", a, b)
                if b < a:
                    continue
                frm, to = E[2 * a + 1][0] ^ 1, E[2 * a][0]
                assert [X for X in E[frm] if X >> 1 == a] == [2 * a], ("from reaches a in its forward reading only", a)
                Bs = [X for X in E[frm] if X >> 1 == b]
                assert len(Bs) == 1, ("from reaches b in one reading", a, b)
                A, B = 2 * a, Bs[0]
                ta, tb = self.text_of(A), self.text_of(B)
                na, nb = len(ta), len(tb)
                assert na == k + L[a] - 1 and nb == k + L[b] - 1
                m = min(na, nb)
                lcp = common_prefix(ta, tb)
                lcs = min(common_prefix(ta[::-1], tb[::-1]), m - lcp)
                if L[a] == L[b]:
                    nm = sum(1 for x, y in zip(ta, tb) if x != y)
                    assert nm >= 1, "equal texts would be the same rows"
                    kind = SNP if nm == 1 else MULTI
                else:
                    nm, kind = 0, (INDEL if lcp + lcs == m else COMPLEX)
                recs.append((A, B, frm, to, lcp, lcs, nm, kind))
                lines += [ta, tb]
                self.per_unitig[a] += 1
                self.per_unitig[b] += 1
        self.records = np.array(recs, dtype=np.int64).reshape(len(recs), 8)
        self.lines = lines
        self.v_offsets = np.concatenate([[0], np.cumsum([len(t) + 1 for t in lines])]).astype(np.int64)
        self.v_stream = np.frombuffer("".join(t + "\n" for t in lines).encode(), dtype=np.uint8).copy()
        kinds = [r[7] for r in recs]
        self.variant_stats = dict(n_variants=len(recs), n_snps=kinds.count(SNP), n_multi=kinds.count(MULTI), n_indels=kinds.count(INDEL),
                                  n_complex=kinds.count(COMPLEX), n_unitigs=len(self.per_unitig), stream_bytes=len(self.v_stream),
                                  max_letters=max((len(t) for t in lines), default=0))

    def kinds(self):
        return sorted(int(x) for x in self.records[:, 7])

    def check_variant_facts(self, oracle=None):
        k, L, s = self.k, self.L, self.variant_stats
        pairs = [(int(r[0]) >> 1, int(r[1]) >> 1) for r in self.records]
        assert pairs == sorted(set(pairs)) and all(a < b for a, b in pairs), "each pair once, a < b, ascending"
        assert s["n_unitigs"] == self.bubble_stats["n_in_bubbles"]
        assert s["stream_bytes"] == sum(L[a] + L[b] for a, b in pairs) + 2 * len(pairs) * k == int(self.v_offsets[-1])
        no_palindrome = not any(self.pal)
        for (a, b), r in zip(pairs, self.records):
            lcp, lcs, nm, kind = (int(x) for x in r[4:])
            na, nb = k + L[a] - 1, k + L[b] - 1
            assert lcp + lcs <= min(na, nb)
            if L[a] == L[b]:
                assert nm >= 1 and (kind == SNP) == (lcp + lcs == na - 1)
            else:
                assert nm == 0 and kind in (INDEL, COMPLEX)
            if no_palindrome:
                assert lcp >= k - 1, ("both branches leave `from` over k - 1 letters", a, b)
        if oracle is not None and len(pairs):
            back = oracle.count(self.v_stream.copy(), k)
            got = sorted((int(v), int(c)) for v, c in zip(back.values(), back.ab))
            want = sorted((self.values[p >> 1], n) for u, n in self.per_unitig.items() for p in self.paths[u][0])
            assert got == want, "the stream counts back to the rows of the flagged unitigs, each as often as its unitig has variants"


def restate(values, ab, k, max_nodes, max_diff=4, oracle=None):
    exp = VariantRestatement(values, ab, k, max_nodes, max_diff)
    exp.check_bubble_facts()
    exp.check_variant_facts(oracle)
    return exp


def variants_stream(k):
    """-> (the reads, M).  M is read three times.  Along it, 2 k + 9 bases apart: two substitutions 3 apart read once (MULTI), a deletion of 3
    read twice (INDEL), a substitution followed by two inserted bases (COMPLEX), and one more base in a run of 5 (INDEL whose lcs the cap
    cuts to k - 1 - 5)."""
    rng = np.random.default_rng(9000 + k)
    def rnd(n): return "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    def other(c): return "ACGT"[("ACGT".index(c) + 1) % 4]
    def other2(c): return "ACGT"[("ACGT".index(c) + 2) % 4]
    step = 2 * k + 9
    p1 = 3 * k + 10; p2 = p1 + step; p3 = p2 + step; p4 = p3 + step
    M = list(rnd(p4 + 3 * k + 12)); run = other(M[p4 - 1])
    for i in range(5): M[p4 + i] = run                      # a run of 5
    if M[p4 + 5] == run: M[p4 + 5] = other(run)
    M = "".join(M); reads = [M, M, M]
    def win(mid, lo, hi): return M[lo - (k - 1): lo] + mid + M[hi: hi + k - 1]      # M[lo:hi] replaced
    reads += [win(other(M[p1]) + M[p1 + 1: p1 + 3] + other(M[p1 + 3]), p1, p1 + 4)]   # two SNPs 3 apart: MULTI
    reads += [win("", p2, p2 + 3)] * 2                                                # a deletion of 3: INDEL
    y = other(M[p3]); y = y if y != M[p3 + 1] else other2(M[p3])
    reads += [M[p3 - (k - 1): p3] + other(M[p3]) + rnd(1) + y + M[p3 + 1: p3 + k]]    # substitution + 2 inserted: COMPLEX
    reads += [win(run * 6, p4, p4 + 5)]                                               # one more in the run: INDEL, lcs capped
    return np.frombuffer(("\n".join(reads) + "\n").encode(), dtype=np.uint8).copy(), M


# golden reads, (k, abundance_min): variants with max_nodes = 2 k and max_diff = 4 of (the rows clip(.., max_nodes = k) leaves, all rows);
# every one a SNP
VARIANTS_PINNED = {(31, 2): (26, 12), (15, 2): (73, 49), (16, 2): (70, 49), (63, 2): (0, 0), (15, 1): (134, 114)}


def check_bubbles_stream(exp4, exp6, k):
    """the bubbles stream at max_diff 4 and 6: seven SNPs; with 6 the branch that is 6 rows longer is an INDEL too"""
    assert exp4.kinds() == [SNP] * 7 and exp4.variant_stats["n_unitigs"] == 11
    assert exp6.kinds() == [SNP] * 7 + [INDEL] and exp6.variant_stats["n_unitigs"] == 13
    indel = exp6.records[exp6.records[:, 7] == INDEL][0]
    assert (int(indel[4]), int(indel[5])) == (k - 1, k - 1)


def check_popped_bubbles_stream(exp, k):
    """after one round of pops the outer branch of the nested bubble is one MULTI: two bases 6 apart"""
    multi = exp.records[exp.records[:, 7] == MULTI]
    assert len(multi) == 1 and int(multi[0][6]) == 2
    a, b = exp.lines[2 * int(np.nonzero(exp.records[:, 7] == MULTI)[0][0]):][:2]
    assert [i for i, (x, y) in enumerate(zip(a, b)) if x != y] == [k - 1, k + 5]
    assert (int(multi[0][4]), int(multi[0][5])) == (k - 1, k - 1)


def check_variants_stream(exp, k):
    """13 unitigs, 4 variants of kinds {2, 3, 3, 4}; the MULTI's two bases 3 apart, one INDEL's lcs cut by the cap, texts of up to 2 k + 2 letters"""
    assert exp.stats["n_unitigs"] == 13 and exp.kinds() == [MULTI, INDEL, INDEL, COMPLEX]
    s = exp.variant_stats
    assert (s["n_variants"], s["n_snps"], s["n_multi"], s["n_indels"], s["n_complex"]) == (4, 0, 1, 2, 1)
    multi = exp.records[exp.records[:, 7] == MULTI][0]
    assert (int(multi[4]), int(multi[5]), int(multi[6])) == (k - 1, k - 1, 2)
    by_diff = {abs(len(exp.lines[2 * i]) - len(exp.lines[2 * i + 1])): int(r[5]) for i, r in enumerate(exp.records) if r[7] == INDEL}
    assert sorted(by_diff) == [1, 3] and by_diff[1] == k - 1 - 5 and by_diff[3] <= k - 1      # the run of 5: the cap; the deletion of 3
    assert all(int(r[6]) == 0 for r in exp.records if r[7] != MULTI)
    assert s["max_letters"] == 2 * k + 2                                         # (the longest branch has k + 3 nodes)


_done = {}


def restated_stream(oracle, which, k, max_diff=4):
    key = (which, k, max_diff)
    if key not in _done:
        stream = (bubbles_stream if which == "bubbles" else variants_stream)(k)[0]
        values, ab = solid_rows(oracle, stream, k, 1)
        _done[key] = restate(values, ab, k, 2 * k, max_diff, oracle)
    return _done[key]


@pytest.mark.parametrize("k", BUBBLES_STREAM_K)
def test_bubbles_stream(oracle, k):
    exp4, exp6 = restated_stream(oracle, "bubbles", k, 4), restated_stream(oracle, "bubbles", k, 6)
    print("variants of the bubbles stream", k, exp4.variant_stats, exp6.variant_stats)
    check_bubbles_stream(exp4, exp6, k)


@pytest.mark.parametrize("k", BUBBLES_STREAM_K)
def test_bubbles_stream_after_one_round_of_pops(oracle, k):
    values, ab = solid_rows(oracle, bubbles_stream(k)[0], k, 1)
    p = pop(values, ab, k, 2 * k, 4, max_rounds=1)
    exp = restate(p.values, p.ab, k, 2 * k, 4, oracle)
    print("variants after one pop", k, exp.variant_stats)
    check_popped_bubbles_stream(exp, k)


@pytest.mark.parametrize("k", BUBBLES_STREAM_K)
def test_variants_stream(oracle, k):
    exp = restated_stream(oracle, "variants", k)
    print("variants stream", k, exp.variant_stats, exp.records.tolist())
    check_variants_stream(exp, k)


@pytest.mark.parametrize("k,amin", sorted(VARIANTS_PINNED))
def test_golden_reads(oracle, golden_dir, k, amin):
    c = clipped_golden(oracle, golden_dir, k, amin, k, 0)
    clipped = restate(c.values, c.ab, k, 2 * k, 4, oracle)
    values, ab = solid_rows(oracle, np.ascontiguousarray(oracle.load_bank(os.path.join(golden_dir, GOLDEN))[0]), k, amin)
    whole = restate(values, ab, k, 2 * k, 4, oracle)
    print("variants golden", (k, amin), clipped.variant_stats, whole.variant_stats)
    assert (clipped.variant_stats["n_variants"], whole.variant_stats["n_variants"]) == VARIANTS_PINNED[(k, amin)]
    assert clipped.variant_stats["n_snps"] == clipped.variant_stats["n_variants"] and whole.variant_stats["n_snps"] == whole.variant_stats["n_variants"]


def test_the_definitions_on_two_handmade_pairs():
    """lcp / lcs / kind on strings, without a graph: the cap for an indel inside a run, and a substitution next to an indel"""
    for ta, tb, want in (("ACGTTTTTGCA", "ACGTTTTTTGCA", (8, 3, INDEL)), ("ACGTACGT", "ACGAACGT", (3, 4, SNP)), ("ACGTACGTAC", "ACGAGGACGTAC", (3, 6, COMPLEX))):
        m = min(len(ta), len(tb))
        lcp = common_prefix(ta, tb)
        lcs = min(common_prefix(ta[::-1], tb[::-1]), m - lcp)
        kind = (SNP if sum(x != y for x, y in zip(ta, tb)) == 1 else MULTI) if len(ta) == len(tb) else (INDEL if lcp + lcs == m else COMPLEX)
        assert (lcp, lcs, kind) == want, (ta, tb)
