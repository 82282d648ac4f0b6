"""Every restatement of the graph layer on the dense inputs of tests/dense_streams.py (k = 3 .. 14), on the CPU, before
tests/test_gpu_dense.py trusts them on the device.  restate_all() takes the rows of one input through the component, tip, bubble,
connection, simplify_all, variant, thread and correction restatements, so every check_*_facts of those modules runs on every input; the
COVERAGE conditions below assert that the inputs hold the structures they were made for, so that no device test can pass vacuously; and
DENSE_PINNED fixes what the restatements give.  The pinned numbers were computed here, on the oracle's solid rows (global order); they were
never read off a device."""
from collections import Counter

import numpy as np
import pytest

pytest.importorskip("torch")          # (the GPU modules imported below import it at the top)
from tests.dense_streams import DENSE_CASES, ROW_CAP, dense_parts, dense_stream, revcomp, space      # noqa: E402
from tests.test_bubbles_restatement import check_pop_facts, pop      # noqa: E402
from tests.test_components_restatement import ComponentRestatement, drop_summary      # noqa: E402
from tests.test_connections_restatement import ConnectionRestatement, check_remove_facts, remove, simplify_all      # noqa: E402
from tests.test_correct_restatement import CorrectRestatement      # noqa: E402
from tests.test_gpu_graph import adj_of, degree_table      # noqa: E402
from tests.test_thread_restatement import ThreadRestatement      # noqa: E402
from tests.test_tips_restatement import check_clip_facts, clip      # noqa: E402
from tests.test_unitigs_restatement import solid_rows      # noqa: E402
from tests.test_variants_restatement import COMPLEX, INDEL, MULTI, SNP, restate as restate_variants      # noqa: E402

TRUST_MIN = 2


def params(k):
    """(tips, bubbles, connections): the defaults of the device calls -- tips of up to k rows, bubbles of up to 2 k rows whose lengths differ by
    at most 4, connections of up to 2 k rows with min_ratio 4"""
    return (k, 0), (2 * k, 4), (2 * k, 4, 0)


class DenseRestated:
    """what restate_all() gives; every member is a restatement of the modules named above, or what one returns"""


def restate_all(values, ab, k, stream, oracle=None):
    tp, bp, cp = params(k)
    D = DenseRestated()
    D.k, D.values, D.ab = k, list(values), [int(a) for a in ab]
    D.comp = ComponentRestatement(values, ab, k)                             # unitigs, edges and components of all rows
    D.comp.check_facts()
    D.comp.check_component_facts()
    solid = set(D.values)
    D.adj = np.array([adj_of(v, k, solid) for v in D.values], dtype=np.uint8)
    D.degrees = degree_table(D.adj)
    D.dropped, D.drop_stats = D.comp.drop(2 * k)
    D.clip = clip(values, ab, k, *tp)
    check_clip_facts(D.clip, k, *tp)
    D.pop = pop(values, ab, k, *bp)
    check_pop_facts(D.pop, k, *bp)
    D.remove = remove(values, ab, k, *cp)
    check_remove_facts(D.remove, k, *cp)
    D.conn2 = ConnectionRestatement(values, ab, k, cp[0], 2)
    D.conn2.check_connection_facts()
    D.all = simplify_all(values, ab, k, tp, bp, cp)
    D.variants = restate_variants(values, ab, k, *bp, oracle=oracle)
    D.pop1 = pop(values, ab, k, *bp, max_rounds=1)
    D.variants1 = restate_variants(D.pop1.values, D.pop1.ab, k, *bp, oracle=oracle)
    D.thread = ThreadRestatement(values, ab, k)
    D.walks = D.thread.thread(stream)
    D.thread.check_facts(D.walks)
    D.thread_all = ThreadRestatement(D.all.values, D.all.ab, k)
    D.walks_all = D.thread_all.thread(stream)
    D.thread_all.check_facts(D.walks_all)
    D.correct = CorrectRestatement(values, ab, k, TRUST_MIN)
    D.corrected = D.correct.correct(stream)
    D.correct.check_facts(stream, D.corrected)
    return D


def kinds_of(v):
    s = v.variant_stats
    return (s["n_snps"], s["n_multi"], s["n_indels"], s["n_complex"])


def summary(D):
    """what DENSE_PINNED fixes per input.  Counts only: the row order changes the numbering, never these."""
    e = D.comp
    return dict(
        rows=e.n, unitigs=e.stats["n_unitigs"], cycles=e.stats["n_cycles"], palindromes=e.n_palindromes, edges=e.summary(),
        components=(e.component_summary(), drop_summary(D.drop_stats)),
        tips=[r[2:] for r in D.clip.rounds], bubbles=[r[2:] for r in D.pop.rounds], connections=[r[2:] for r in D.remove.rounds],
        all=(D.all.total["n_passes"], D.all.total["tips"]["n_rows_clipped"], D.all.total["bubbles"]["n_rows_popped"],
             D.all.total["connections"]["n_rows_removed"], D.all.total["n_rows_left"]),
        variants=(kinds_of(D.variants), kinds_of(D.variants1)),
        thread=(D.thread.summary(D.walks), D.thread_all.summary(D.walks_all)),
        correct=D.corrected.summary())


def coverage(D):
    """how many of each structure the input holds: what the conditions below ask for and what the pull request's summary quotes"""
    e, E = D.comp, D.comp.edges
    entries = [(U, V) for U, out in enumerate(E) for V in out]
    between = Counter()
    for U, V in set(min((U, V), (V ^ 1, U ^ 1)) for U, V in entries):       # an entry and its mirror image count once
        if U >> 1 != V >> 1:
            between[(min(U >> 1, V >> 1), max(U >> 1, V >> 1))] += 1
    deg = [len(out) for out in E]
    first = D.remove.first
    last = D.pop.last
    t, b, c = D.clip.total, D.pop.total, D.remove.total
    small = D.comp.small(2 * D.k)[2]
    return dict(
        palindromes=e.n_palindromes, self_edges=e.edge_stats["n_self"], hairpins=sum(1 for U, V in entries if V == U ^ 1),
        double_joins=sum(1 for n in between.values() if n > 1), max_degree=e.edge_stats["max_degree"], ends_of_4=deg.count(4),
        unitigs_of_8=sum(1 for u in range(len(deg) // 2) if deg[2 * u] + deg[2 * u + 1] == 8),
        connection_candidates=c["n_candidates"], connections_removed=c["n_removed"], connection_rounds=c["n_rounds"],
        max_flank=max((len(f) for f in first.flank.values()), default=0), flanks_over_4=sum(1 for f in first.flank.values() if len(f) > 4),
        tips=t["n_tips"], outranked=t["n_outranked"], popped=b["n_popped"],
        equal_pairs=sum(1 for u, sib in last.siblings.items() for w in sib if u < w and not last.stronger(u, w) and not last.stronger(w, u)),
        variants=kinds_of(D.variants), components=e.comp_stats["n_components"], small_components=small["n_small"], cycles=e.stats["n_cycles"],
        corrected=D.corrected.stats["n_corrected"], ambiguous=D.corrected.stats["n_ambiguous"], unfixable=D.corrected.stats["n_unfixable"])


_done = {}


def restated_dense(oracle, k, seed):
    """restate_all() of the oracle's rows of dense_stream(k, seed) (global order), computed once and never changed"""
    if (k, seed) not in _done:
        stream = dense_stream(k, seed)
        values, ab = solid_rows(oracle, stream, k, 1)
        _done[(k, seed)] = restate_all(values, ab, k, stream, oracle)
    return _done[(k, seed)]


# what summary() gives per input, fixed on the CPU, whatever the row order.  edges: (entries, [oriented unitigs with 0 .. 4 entries], self
# entries); components: ((components, of one unitig, most unitigs, most rows), drop(2 k) as (small, unitigs dropped, rows dropped)); tips /
# bubbles / connections: per round of clip() / pop() / remove() the (candidates, flagged, outranked | popped | removed, rows taken out) -- for
# the bubbles (candidates, in bubbles, popped, rows), for the connections (candidates, one-sided, removed, rows); all: simplify_all as (passes,
# rows clipped, popped, removed, left); variants: (SNP, MULTI, INDEL, COMPLEX) of all rows and after one round of pops; thread: (valid, placed,
# walks, steps, most steps, edge support) through all rows and through what simplify_all leaves; correct: the stats in the order of STATS
DENSE_PINNED = {
    (3, 1): {'rows': 19, 'unitigs': 19, 'cycles': 0, 'palindromes': 0, 'edges': (91, [9, 6, 0, 7, 16], 11), 'components': ((3, 2, 17, 17), (2, 2, 2)), 'tips': [(7, 6, 0, 6), (1, 0, 0, 0)], 'bubbles': [(0, 0, 0, 0)], 'connections': [(4, 0, 0, 0)], 'all': (1, 6, 0, 0, 13), 'variants': ((0, 0, 0, 0), (0, 0, 0, 0)), 'thread': ((457, 457, 28, 457, 96, 429), (457, 448, 28, 448, 95, 420)), 'correct': (457, 450, 7, 0, 1, 4, 2, 0, 5, 0)},
    (4, 1): {'rows': 109, 'unitigs': 109, 'cycles': 0, 'palindromes': 11, 'edges': (753, [7, 0, 7, 77, 127], 4), 'components': ((3, 2, 107, 107), (2, 2, 2)), 'tips': [(3, 3, 0, 3), (0, 0, 0, 0)], 'bubbles': [(0, 0, 0, 0)], 'connections': [(102, 10, 11, 11), (91, 10, 0, 0)], 'all': (1, 3, 0, 11, 95), 'variants': ((0, 0, 0, 0), (0, 0, 0, 0)), 'thread': ((1801, 1801, 62, 1801, 408, 1739), (1801, 1762, 95, 1762, 131, 1667)), 'correct': (1801, 1792, 9, 0, 0, 4, 5, 0, 4, 0)},
    (5, 1): {'rows': 264, 'unitigs': 239, 'cycles': 0, 'palindromes': 0, 'edges': (1290, [7, 43, 135, 195, 98], 40), 'components': ((4, 3, 236, 247), (3, 3, 17)), 'tips': [(1, 1, 0, 1), (0, 0, 0, 0)], 'bubbles': [(1, 0, 0, 0)], 'connections': [(199, 23, 23, 23), (174, 23, 0, 0)], 'all': (1, 1, 0, 23, 240), 'variants': ((0, 0, 0, 0), (0, 0, 0, 0)), 'thread': ((1351, 1351, 52, 1278, 246, 1226), (1351, 1321, 71, 1236, 219, 1165)), 'correct': (1351, 1290, 31, 0, 1, 5, 25, 2, 4, 0)},
    (6, 1): {'rows': 951, 'unitigs': 825, 'cycles': 0, 'palindromes': 22, 'edges': (4040, [7, 137, 758, 605, 143], 2), 'components': ((4, 3, 822, 940), (3, 3, 11)), 'tips': [(1, 1, 0, 1), (0, 0, 0, 0)], 'bubbles': [(9, 0, 0, 0)], 'connections': [(820, 50, 35, 39), (782, 50, 0, 0)], 'all': (1, 1, 0, 39, 911), 'variants': ((0, 0, 0, 0), (0, 0, 0, 0)), 'thread': ((3966, 3966, 63, 3567, 935, 3504), (3966, 3926, 86, 3520, 932, 3434)), 'correct': (3966, 3851, 54, 1, 1, 8, 44, 5, 3, 2)},
    (6, 2): {'rows': 939, 'unitigs': 822, 'cycles': 0, 'palindromes': 27, 'edges': (3969, [7, 177, 746, 556, 158], 2), 'components': ((4, 3, 819, 910), (3, 3, 29)), 'tips': [(1, 1, 0, 1), (0, 0, 0, 0)], 'bubbles': [(12, 0, 0, 0)], 'connections': [(817, 46, 40, 43), (770, 46, 0, 0)], 'all': (1, 1, 0, 43, 895), 'variants': ((0, 0, 0, 0), (0, 0, 0, 0)), 'thread': ((3986, 3986, 63, 3667, 962, 3604), (3986, 3936, 100, 3578, 355, 3478)), 'correct': (3986, 3866, 53, 1, 2, 6, 44, 3, 6, 0)},
    (7, 1): {'rows': 1504, 'unitigs': 768, 'cycles': 1, 'palindromes': 0, 'edges': (2999, [12, 274, 1039, 197, 14], 47), 'components': ((7, 6, 762, 1480), (6, 6, 24)), 'tips': [(6, 6, 0, 8), (0, 0, 0, 0)], 'bubbles': [(39, 0, 0, 0)], 'connections': [(715, 40, 11, 23), (700, 40, 0, 0)], 'all': (1, 8, 0, 23, 1473), 'variants': ((0, 0, 0, 0), (0, 0, 0, 0)), 'thread': ((5147, 5147, 59, 2861, 764, 2802), (5147, 5112, 68, 2825, 759, 2757)), 'correct': (5147, 4948, 50, 4, 1, 7, 38, 4, 3, 5)},
    (8, 1): {'rows': 1677, 'unitigs': 377, 'cycles': 1, 'palindromes': 13, 'edges': (1288, [19, 228, 463, 42, 2], 4), 'components': ((6, 5, 372, 1651), (5, 5, 26)), 'tips': [(12, 11, 1, 29), (0, 0, 0, 0)], 'bubbles': [(38, 6, 2, 16), (35, 2, 0, 0)], 'connections': [(350, 20, 8, 48), (335, 20, 0, 0)], 'all': (1, 29, 16, 32, 1600), 'variants': ((2, 0, 1, 0), (1, 0, 0, 0)), 'thread': ((5333, 5333, 62, 1309, 319, 1247), (5333, 5250, 70, 1231, 304, 1161)), 'correct': (5333, 5052, 46, 12, 1, 10, 23, 8, 2, 13)},
    (9, 1): {'rows': 1525, 'unitigs': 170, 'cycles': 1, 'palindromes': 0, 'edges': (490, [18, 160, 156, 6, 0], 14), 'components': ((7, 6, 164, 1511), (6, 6, 14)), 'tips': [(11, 10, 1, 39), (1, 1, 0, 9), (0, 0, 0, 0)], 'bubbles': [(47, 15, 7, 56), (34, 2, 0, 0)], 'connections': [(129, 18, 11, 57), (101, 18, 0, 0)], 'all': (1, 48, 63, 35, 1379), 'variants': ((7, 0, 2, 0), (1, 0, 0, 0)), 'thread': ((4849, 4849, 61, 598, 109, 537), (4849, 4670, 73, 438, 74, 365)), 'correct': (4849, 4552, 45, 9, 0, 10, 26, 7, 1, 11)},
    (9, 2): {'rows': 1540, 'unitigs': 164, 'cycles': 1, 'palindromes': 0, 'edges': (476, [17, 152, 153, 6, 0], 16), 'components': ((7, 6, 158, 1513), (6, 6, 27)), 'tips': [(9, 8, 1, 24), (1, 1, 0, 9), (0, 0, 0, 0)], 'bubbles': [(38, 20, 9, 81), (21, 2, 0, 0)], 'connections': [(120, 15, 13, 86), (85, 16, 0, 0)], 'all': (1, 33, 81, 68, 1358), 'variants': ((3, 0, 7, 0), (1, 0, 0, 0)), 'thread': ((4854, 4854, 61, 573, 113, 512), (4854, 4658, 75, 389, 73, 314)), 'correct': (4854, 4536, 40, 13, 0, 9, 18, 9, 1, 12)},
    (10, 1): {'rows': 1625, 'unitigs': 144, 'cycles': 2, 'palindromes': 5, 'edges': (381, [20, 159, 105, 4, 0], 6), 'components': ((9, 6, 133, 1531), (7, 10, 64)), 'tips': [(12, 9, 1, 35), (2, 0, 0, 0)], 'bubbles': [(51, 26, 12, 121), (28, 2, 0, 0)], 'connections': [(107, 15, 7, 69), (88, 13, 2, 21), (83, 13, 0, 0)], 'all': (1, 35, 121, 32, 1437), 'variants': ((6, 0, 7, 0), (1, 0, 0, 0)), 'thread': ((5031, 5031, 62, 493, 91, 431), (5031, 4843, 77, 345, 58, 268)), 'correct': (5031, 4640, 42, 9, 0, 9, 24, 9, 1, 8)},
    (12, 1): {'rows': 1690, 'unitigs': 113, 'cycles': 2, 'palindromes': 3, 'edges': (278, [20, 139, 62, 5, 0], 6), 'components': ((9, 6, 102, 1608), (7, 10, 46)), 'tips': [(12, 9, 1, 52), (2, 0, 0, 0)], 'bubbles': [(52, 41, 20, 231), (14, 2, 0, 0)], 'connections': [(80, 16, 7, 78), (58, 13, 3, 36), (51, 12, 1, 14), (48, 12, 0, 0)], 'all': (2, 52, 258, 48, 1332), 'variants': ((9, 1, 11, 1), (1, 0, 0, 0)), 'thread': ((5281, 5281, 62, 397, 61, 335), (5281, 4909, 89, 154, 21, 65)), 'correct': (5281, 4835, 41, 12, 0, 9, 20, 9, 1, 11)},
    (14, 1): {'rows': 1799, 'unitigs': 116, 'cycles': 2, 'palindromes': 3, 'edges': (285, [20, 141, 69, 2, 0], 6), 'components': ((9, 6, 104, 1678), (7, 11, 79)), 'tips': [(12, 9, 1, 65), (2, 0, 0, 0)], 'bubbles': [(49, 27, 13, 179), (24, 2, 0, 0)], 'connections': [(86, 12, 11, 150), (50, 11, 1, 13), (47, 11, 0, 0)], 'all': (1, 65, 233, 68, 1433), 'variants': ((8, 1, 6, 0), (1, 0, 0, 0)), 'thread': ((5579, 5579, 62, 413, 64, 351), (5579, 5199, 85, 185, 21, 100)), 'correct': (5579, 5029, 43, 11, 1, 10, 21, 8, 1, 13)},
}


# ------------------------------------------------------------------ the generator
@pytest.mark.parametrize("k,seed", DENSE_CASES)
def test_the_stream_is_what_its_description_says(oracle, k, seed):
    P = dense_parts(k, seed)
    assert dense_stream(k, seed) is P.stream and P.stream.dtype == np.uint8 and P.stream[-1] == ord("\n")
    assert bytes(P.stream).decode().split("\n")[:-1] == P.reads
    assert P.reads[:3] == [P.G, P.G, revcomp(P.G)] and len(P.pieces) >= 2 and len(P.degenerate) == (4 if k % 2 == 0 else 3)
    values, ab = solid_rows(oracle, P.stream, k, 1)
    assert len(values) <= ROW_CAP * 11 // 10
    share = len(values) / space(k)
    print("dense stream", (k, seed), "rows", len(values), "of", space(k), "share %.3f" % share, "reads", len(P.reads))
    if k <= 4:
        assert share > 0.5                                                   # a tiny space: the input holds most of it
    elif k <= 7:
        assert 0.05 <= share <= 0.70
    # (from k = 8 on the row cap, not the space, bounds the input: 2 000 rows are 6 % of the space at k = 8 and 1.5 % at k = 9)


# ------------------------------------------------------------------ per input: the facts, the coverage, the pinned numbers
@pytest.mark.parametrize("k,seed", DENSE_CASES)
def test_every_restatement_on_a_dense_input(oracle, k, seed):
    D = restated_dense(oracle, k, seed)                                     # every check_*_facts ran in there
    got, cov = summary(D), coverage(D)
    print("dense summary", (k, seed), got)
    print("dense coverage", (k, seed), cov)
    # edges
    if k % 2 == 0:
        assert cov["palindromes"] > 0
    if k <= 8:                                                               # (2 000 rows are too few of 4^9 / 2 for an end with 4 targets)
        assert cov["max_degree"] == 4
    if k <= 6:
        assert cov["unitigs_of_8"] > 0 and cov["double_joins"] > 0 and cov["flanks_over_4"] > 0
    # the connection rule
    if k >= 4:
        assert cov["connections_removed"] > 0
    # tips, bubbles
    if k >= 8:
        assert cov["tips"] > 0
    if k >= 9:
        assert cov["popped"] > 0
        assert cov["variants"][0] > 0 and cov["variants"][2] > 0               # SNP and INDEL
        assert cov["cycles"] > 0
        assert cov["corrected"] > 0 and cov["ambiguous"] > 0
    if k <= 6:
        assert cov["ambiguous"] + cov["unfixable"] > 0
    # components
    assert cov["components"] > 2 and cov["small_components"] > 0
    # every valid window of the counted stream is placed; after simplify_all some are not
    s = D.walks.stats
    assert s["n_placed"] == s["n_valid"] > 0 and D.walks_all.stats["n_placed"] <= s["n_placed"]
    assert got == DENSE_PINNED[(k, seed)]


def test_all_inputs_together_hold_every_structure(oracle):
    cov = {case: coverage(restated_dense(oracle, *case)) for case in DENSE_CASES}
    total = {name: sum(c[name] for c in cov.values()) for name in next(iter(cov.values())) if name != "variants"}
    kinds = [sum(c["variants"][i] for c in cov.values()) for i in range(4)]
    print("dense coverage, all inputs", total, dict(zip(("snp", "multi", "indel", "complex"), kinds)))
    assert total["self_edges"] > 0 and total["hairpins"] > 0 and total["double_joins"] > 0
    assert max(c["max_degree"] for c in cov.values()) == 4 and total["unitigs_of_8"] > 0
    assert sum(1 for c in cov.values() if c["connection_rounds"] > 1) >= 3
    assert max(c["max_flank"] for c in cov.values()) > 4
    assert total["outranked"] > 0
    assert kinds[SNP - 1] > 0 and kinds[INDEL - 1] > 0 and kinds[MULTI - 1] + kinds[COMPLEX - 1] > 0
    assert total["equal_pairs"] > 0                                          # equally strong branches, and both stay
