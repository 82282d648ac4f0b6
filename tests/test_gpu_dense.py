"""Every graph kernel on the dense inputs of tests/dense_streams.py: k = 3 .. 14, where a modest input fills a large share of the canonical
k-mers and palindromic rows, self-loops, hairpin edges, several edges between two unitigs, ends with 4 targets, full flanks and ambiguous
corrections occur by the hundred (include/dskgpu.h, from "the rows' de Bruijn neighbours" to "erroneous connections").

All comparisons are exact.  The expectation is restate_all() of tests/test_dense_restatement.py (which the CPU suite checks first), made of
the rows as the context returns them and cached per (k, seed, row order); the helpers that compare are those of the test_gpu_* module of
each feature.  Three tests per input and row order, one context each, so that the products are also checked after each other: the tables
and one round of every rule; the loops; the reads, the drop and a new count.  All of it is counted with abundance_min = 1.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from tests import test_gpu_bubbles as bubbles_mod      # noqa: E402
from tests import test_gpu_components as components_mod      # noqa: E402
from tests import test_gpu_connections as connections_mod      # noqa: E402
from tests import test_gpu_correct as correct_mod      # noqa: E402
from tests import test_gpu_graph as graph_mod      # noqa: E402
from tests import test_gpu_query as query_mod      # noqa: E402
from tests import test_gpu_thread as thread_mod      # noqa: E402
from tests import test_gpu_tips as tips_mod      # noqa: E402
from tests import test_gpu_unitig_edges as edges_mod      # noqa: E402
from tests import test_gpu_unitigs as unitigs_mod      # noqa: E402
from tests import test_gpu_variants as variants_mod      # noqa: E402
from tests.dense_streams import DENSE_CASES, dense_stream      # noqa: E402
from tests.test_dense_restatement import DENSE_PINNED, TRUST_MIN, params, restate_all, summary      # noqa: E402
from tests.test_gpu_unitigs import count, row_values      # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


_done, _lookups = {}, {}


def restated(kc, k, seed, order):
    """restate_all() of the rows of kc, cached per (k, seed, row order) and never changed"""
    key = (k, seed, order)
    if key not in _done:
        kk, ab = kc.rows()
        _done[key] = restate_all(row_values(kk), ab, k, dense_stream(k, seed))
        assert summary(_done[key]) == DENSE_PINNED[(k, seed)]                # the row order changes the numbering, never the counts
    return _done[key]


def lookups(D, k, seed):
    """-> (values, their abundance as dskgpu_query_kmers answers, their adjacency byte by the string restatement), the same for both row
    orders.  k <= 8: all 4^k values, canonical or not; beyond: the rows, their reverse complements and the 8 neighbours of every row."""
    if (k, seed) not in _lookups:
        from dsk_amd.engine import kmer_to_string
        ab_of = dict(zip(D.values, D.ab))
        solid = set(ab_of)
        if k <= 8:
            values = list(range(4 ** k))
        else:
            values = []
            for v in sorted(solid):
                s = kmer_to_string(v, k)
                values += [v, graph_mod.encode(graph_mod.revcomp_str(s))]
                values += [graph_mod.encode(s[1:] + c) for c in "ACTG"] + [graph_mod.encode(c + s[:-1]) for c in "ACTG"]
        want_ab = np.array([ab_of.get(v, 0) for v in values], dtype=np.uint32)      # a value that is not canonical is simply not found
        want_adj = np.array([graph_mod.adj_of(v, k, solid) for v in values], dtype=np.uint8)
        _lookups[(k, seed)] = (np.array(values, dtype=np.uint64).reshape(-1, 1), want_ab, want_adj)
    return _lookups[(k, seed)]


def check_lookups(kc, D, k, seed, dev):
    graph_mod.check_rows_against_restatement(kc, k, dict(zip(D.values, (int(a) for a in D.adj))), D.comp.n)
    values, want_ab, want_adj = lookups(D, k, seed)
    got = query_mod.query_kmers(kc, values, dev)
    bad = np.nonzero(got != want_ab)[0]
    assert len(bad) == 0, ("query_kmers", len(bad), values[bad[:5], 0], got[bad[:5]], want_ab[bad[:5]])
    assert int((got != 0).sum()) >= D.comp.n
    got = graph_mod.neighbors(kc, values, dev, 3)
    bad = np.nonzero(got != want_adj)[0]
    assert len(bad) == 0, ("graph_neighbors", len(bad), values[bad[:5], 0], got[bad[:5]], want_adj[bad[:5]])


def check_graph_of(kc, exp):
    unitigs_mod.check_against_restatement(kc, exp)
    edges_mod.check_against_restatement(kc, exp)


def check_rounds(kc, D, k):
    """one round of each rule as flags; none of them changes the context"""
    tp, bp, cp = params(k)
    tips_mod.check_round(kc, D.clip.first, *tp)
    bubbles_mod.check_round(kc, D.pop.first, *bp)
    connections_mod.check_round(kc, D.remove.first, *cp)
    connections_mod.check_round(kc, D.conn2, cp[0], 2)


def check_tables(kc, D, k, seed, dev):
    check_lookups(kc, D, k, seed, dev)
    check_graph_of(kc, D.comp)
    components_mod.check_against_restatement(kc, D.comp)
    components_mod.check_small(kc, D.comp, 2 * k)
    components_mod.check_small(kc, D.comp, 2 * k, 1)
    check_rounds(kc, D, k)
    variants_mod.check_variants(kc, D.variants, *params(k)[1])


def products(kc, k):
    """what the context answers, as one flat list of dicts and arrays"""
    tp, bp, cp = params(k)
    out = list(unitigs_mod.device_answer(kc)) + list(edges_mod.device_edges(kc))
    st, ucomp, rcomp, table = components_mod.device_components(kc)
    out += [st, ucomp, rcomp] + table
    out += [kc.graph_adjacency_tensor()[0].cpu().numpy()]
    for rows, bits, st in (kc.graph_tips_tensor(*tp), kc.graph_bubbles_tensor(*bp), kc.graph_connections_tensor(*cp)):
        out += [rows.cpu().numpy(), bits.cpu().numpy(), st]
    out += [kc.variants(*bp)] + list(variants_mod.device_variants(kc))
    return out


def check_same(before, after):
    assert len(before) == len(after)
    for i, (a, b) in enumerate(zip(before, after)):
        assert (a == b) if isinstance(a, dict) else (a.shape == b.shape and (a == b).all()), i


def check_rows_are(kc, exp_values, exp_ab):
    kk, ab = kc.rows()
    assert row_values(kk) == exp_values and [int(a) for a in ab] == exp_ab and kc.result_device()[2] == len(exp_values)


CASES = [pytest.param(k, seed, id="k%d-seed%d" % (k, seed)) for k, seed in DENSE_CASES]


# ------------------------------------------------------------------ 1. the tables and one round of every rule
@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k,seed", CASES)
def test_tables_and_one_round_of_every_rule(dev, k, seed, partition_order):
    """adjacency and exhaustive lookups, unitigs, edges, components and their small flags, the flags of one round of tips, bubbles and
    connections (min_ratio 4 and 2), the variants -- and all of it once more, unchanged by the calls in between"""
    with count(dense_stream(k, seed), dev, k, abundance_min=1, partition_order=partition_order) as kc:
        D = restated(kc, k, seed, partition_order)
        kk, ab = kc.rows()
        s0 = kc.stats()
        check_tables(kc, D, k, seed, dev)
        first = products(kc, k)
        check_tables(kc, D, k, seed, dev)
        check_same(first, products(kc, k))
        k2, a2 = kc.rows()
        assert (k2 == kk).all() and (a2 == ab).all() and kc.stats() == s0


# ------------------------------------------------------------------ 2. the loops
@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k,seed", CASES)
def test_the_loops(dev, k, seed, partition_order):
    """clip_tips, pop_bubbles (one round, then the variants of what is left; and all rounds), remove_connections and simplify_all: totals,
    rounds, the rows left in their order, the graph of the rows left, and the reads threaded through the simplified graph"""
    tp, bp, cp = params(k)
    with count(dense_stream(k, seed), dev, k, abundance_min=1, partition_order=partition_order) as kc:
        D = restated(kc, k, seed, partition_order)
        kk, _ = kc.rows()
        for name, call, exp in (("clip", lambda: kc.clip_tips(*tp), D.clip), ("pop", lambda: kc.pop_bubbles(*bp), D.pop),
                                ("remove", lambda: kc.remove_connections(*cp), D.remove)):
            total = call()
            print(name, "stats", total, "expected", exp.total)
            assert total == exp.total, name
            check_rows_are(kc, exp.values, exp.ab)
            check_graph_of(kc, exp.last)
            kc.count()                                                      # the full graph again
            assert (kc.rows()[0] == kk).all()
        total = kc.pop_bubbles(*bp, max_rounds=1)
        assert total == D.pop1.total
        check_rows_are(kc, D.pop1.values, D.pop1.ab)
        variants_mod.check_variants(kc, D.variants1, *bp)
        kc.count()
        total = kc.simplify_all(tips=dict(max_nodes=tp[0], max_abundance=tp[1]), bubbles=dict(max_nodes=bp[0], max_diff=bp[1]),
                                connections=dict(max_nodes=cp[0], min_ratio=cp[1], max_abundance=cp[2]))
        print("simplify_all stats", total, "expected", D.all.total)
        assert total == D.all.total
        check_rows_are(kc, D.all.values, D.all.ab)
        check_graph_of(kc, D.all.last)
        thread_mod.check_against_restatement(kc, D.walks_all, kc._reads_keepalive)
        assert kc.simplify_all()["n_passes"] == 0                           # the defaults are these parameters: nothing is left to do


# ------------------------------------------------------------------ 3. the reads, the drop, a new count
@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k,seed", CASES)
def test_reads_drop_and_a_new_count(dev, k, seed, partition_order):
    """the counted stream threaded through its own graph (every valid window is placed, every hairpin and self-loop step taken) and
    corrected with trust_min = 2; drop_components(2 k) and the components of what is left; a new count gives every first answer back"""
    stream = dense_stream(k, seed)
    with count(stream, dev, k, abundance_min=1, partition_order=partition_order) as kc:
        D = restated(kc, k, seed, partition_order)
        kk, ab = kc.rows()
        first = products(kc, k)
        st = thread_mod.check_against_restatement(kc, D.walks, kc._reads_keepalive)
        assert st["n_placed"] == st["n_valid"]
        correct_mod.same(correct_mod.run(kc, dev, stream, TRUST_MIN), D.corrected)
        total = kc.drop_components(2 * k)
        print("drop stats", total, "expected", D.drop_stats)
        assert total == D.drop_stats and total["n_small"] > 0
        check_rows_are(kc, D.dropped.values, D.dropped.ab)
        check_graph_of(kc, D.dropped)
        components_mod.check_against_restatement(kc, D.dropped)
        kc.count()
        k2, a2 = kc.rows()
        assert (k2 == kk).all() and (a2 == ab).all()
        check_same(first, products(kc, k))
        components_mod.check_against_restatement(kc, D.comp)
        thread_mod.check_against_restatement(kc, D.walks, kc._reads_keepalive)
