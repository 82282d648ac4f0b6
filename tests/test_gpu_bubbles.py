"""The simple bubbles of the compacted de Bruijn graph, found and popped on the device, and tips and bubbles in turn (include/dskgpu.h:
dskgpu_graph_bubbles / dskgpu_pop_bubbles / dskgpu_simplify; csrc/bubbles.h).

All comparisons are exact.  Tests 1 to 3 compare the device with the restatement of tests/test_bubbles_restatement.py, made of the rows as
the context returns them: the bits of every unitig, the flag of every row, the stats of a round, and the rows a pop and a simplify leave.
Test 4 needs no oracle and no restatement: identities on a medium-sized count.  All of it fails before the feature: KmerCounter has no
graph_bubbles().
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from tests import test_gpu_unitig_edges as edges_mod      # noqa: E402
from tests import test_gpu_unitigs as unitigs_mod      # noqa: E402
from tests.test_bubbles_restatement import (BUBBLES_PINNED, BUBBLES_STREAM_K, BUBBLES_STREAM_PASSES, BUBBLES_STREAM_ROUNDS,      # noqa: E402
                                            BubbleRestatement, bubble_rounds_of, bubbles_stream, pop, simplify, stream_params, tip_rounds_of)
from tests.test_gpu_unitigs import code_of, count, row_values, sorted_rows, stream_of      # noqa: E402

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
ZERO = dict(n_candidates=0, n_in_bubbles=0, n_popped=0, n_rows_popped=0, n_rounds=0, n_rows_left=0)
ZERO_TIPS = dict(n_candidates=0, n_tips=0, n_outranked=0, n_rows_clipped=0, n_rounds=0, n_rows_left=0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


_streams, _done = {}, {}


def bubbles_stream_of(k):
    if k not in _streams:
        _streams[k] = bubbles_stream(k)
    return _streams[k]


def restated(key, make):
    """a restatement of the rows of a context, cached per (what, input, k, abundance_min, row order, parameters) and never changed"""
    if key not in _done:
        _done[key] = make()
    return _done[key]


def check_round(kc, exp, max_nodes, max_diff=4):
    """one round on the device against the restatement of the same rows: bits, row flags, stats"""
    row_pop, bits, st = kc.graph_bubbles_tensor(max_nodes, max_diff)
    assert row_pop.dtype == torch.uint8 and bits.dtype == torch.uint8
    print("bubble stats", st, "expected", exp.bubble_stats)
    bits, rows = bits.cpu().numpy(), row_pop.cpu().numpy()
    assert len(bits) == len(exp.bits) and (bits == exp.bits).all(), np.nonzero(bits != exp.bits)[0][:8]
    assert len(rows) == exp.n and (rows == exp.row_pop).all()
    assert st == exp.bubble_stats
    return st


def check_graph_of(kc, exp):
    unitigs_mod.check_against_restatement(kc, exp)
    edges_mod.check_against_restatement(kc, exp)


# ------------------------------------------------------------------ 1. one round against the restatement
@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k,amin", [(31, 2), (63, 2), (16, 2)])
def test_golden_reads_match_the_restatement(oracle, golden_dir, dev, k, amin, partition_order):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, k, abundance_min=amin, partition_order=partition_order) as kc:
        kc.clip_tips()
        kk, ab = kc.rows()
        p = restated(("pop", "golden", k, amin, partition_order), lambda: pop(row_values(kk), ab, k, 2 * k, 4))
        assert p.rounds == BUBBLES_PINNED[(k, amin)]                        # the row order changes the numbering, never the counts
        s0 = kc.stats(); u0 = unitigs_mod.device_answer(kc); e0 = edges_mod.device_edges(kc)
        check_round(kc, p.first, 2 * k)
        # the round changed nothing: rows, stats, unitigs and edges
        k2, a2 = kc.rows()
        assert (k2 == kk).all() and (a2 == ab).all() and kc.stats() == s0
        for before, after in zip(u0 + e0, unitigs_mod.device_answer(kc) + edges_mod.device_edges(kc)):
            assert (before == after) if isinstance(before, dict) else (before == after).all()


@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k", BUBBLES_STREAM_K)
def test_bubbles_stream(dev, k, partition_order):
    """a SNP bubble given as a reverse complement, a three-way bubble, an equal pair, a pair too different in length, a nested bubble and a
    dead-end branch that carries one: every key width and its boundaries"""
    stream, M, _ = bubbles_stream_of(k)
    tp, bp = stream_params(k)
    with count(stream, dev, k, abundance_min=1, partition_order=partition_order) as kc:
        kk, ab = kc.rows()
        p, s = restated(("stream", k, partition_order), lambda: (pop(row_values(kk), ab, k, *bp), simplify(row_values(kk), ab, k, tp, bp)))
        assert bubble_rounds_of(p.rounds, k) == BUBBLES_STREAM_ROUNDS
        assert [(tip_rounds_of(c, k), bubble_rounds_of(b, k)) for c, b in s.passes] == BUBBLES_STREAM_PASSES
        st = check_round(kc, p.first, *bp)
        assert (st["n_in_bubbles"], st["n_popped"], st["n_rows_popped"]) == (11, 5, 5 * k)
        total = kc.pop_bubbles(*bp)
        print("pop stats", total, "expected", p.total)
        assert total == p.total and total["n_rounds"] == 2
        assert row_values(kc.rows()[0]) == p.values and kc.result_device()[2] == len(p.values)
        assert kc.unitigs()["n_unitigs"] == 9
        kc.count()                                                          # the full graph again
        assert (kc.rows()[0] == kk).all()
        total = kc.simplify(tips=dict(max_nodes=tp[0], max_abundance=tp[1]), bubbles=dict(max_nodes=bp[0], max_diff=bp[1]))
        print("simplify stats", total, "expected", s.total)
        assert total == s.total and total["n_passes"] == 2
        k3, a3 = kc.rows()
        assert row_values(k3) == s.values and [int(a) for a in a3] == s.ab
        assert kc.result_device()[2] == len(M) - k + 1 + k + (k + 5) and kc.unitigs()["n_unitigs"] == 7
        text = kc.unitigs_stream_tensor().cpu().numpy()
        assert len(text) == len(s.last.stream) and (text == s.last.stream).all()


# ------------------------------------------------------------------ 2. simplify against the restatement's
@pytest.mark.parametrize("k,amin,partition_order", [(15, 1, False), (31, 2, False), (31, 2, True)])
def test_simplify_on_the_golden_reads(oracle, golden_dir, dev, k, amin, partition_order, tmp_path):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, k, abundance_min=amin, partition_order=partition_order) as kc:
        kk, ab = kc.rows()
        s = restated(("simplify", "golden", k, amin, partition_order), lambda: simplify(row_values(kk), ab, k, (k, 0), (2 * k, 4)))
        assert s.passes[0][1] == BUBBLES_PINNED[(k, amin)] and len(s.passes) == 2 and s.total["n_passes"] == 1
        s0, h0 = kc.stats(), kc.histogram()
        total = kc.simplify()                                               # tips: max_nodes = k; bubbles: max_nodes = 2 k, max_diff = 4
        print("simplify stats", total, "expected", s.total)
        assert total == s.total
        assert total["n_rows_left"] == total["tips"]["n_rows_left"] == total["bubbles"]["n_rows_left"] == kc.result_device()[2] == len(s.values)
        k2, a2 = kc.rows()
        assert row_values(k2) == s.values and [int(a) for a in a2] == s.ab
        assert kc.stats() == s0 and (kc.histogram() == h0).all()            # the count's record
        check_graph_of(kc, s.last)                                          # what the context holds now: the graph of the rows left
        gfa = kc.write_gfa(str(tmp_path / "clean.gfa"))
        lines = open(str(tmp_path / "clean.gfa")).read().split("\n")
        assert gfa == dict(n_segments=s.last.stats["n_unitigs"], n_links=s.last.edge_stats["n_edges"])
        assert sum(1 for ln in lines if ln.startswith("S\t")) == s.last.stats["n_unitigs"]
        assert sum(1 for ln in lines if ln.startswith("L\t")) == s.last.edge_stats["n_edges"]
        st = kc.graph_bubbles(2 * k)
        assert st["n_popped"] == 0 and st["n_rows_left"] == len(s.values)
        assert kc.graph_tips(k)["n_tips"] == 0


def test_the_row_order_never_changes_the_kmers_left(oracle, golden_dir, dev):
    """the numbering differs between the row orders, the set of k-mers a simplify leaves does not: both counted here, compared sorted"""
    stream = stream_of("golden", oracle, golden_dir)
    left = []
    for partition_order in (False, True):
        with count(stream, dev, 31, abundance_min=2, partition_order=partition_order) as kc:
            total = kc.simplify()
            assert (total["n_passes"], total["tips"]["n_rows_clipped"], total["bubbles"]["n_popped"], total["bubbles"]["n_rows_popped"]) == (1, 1758, 26, 806)
            assert kc.unitigs()["n_unitigs"] == 75
            kk, ab = kc.rows()
            order = np.argsort(kk[:, 0], kind="stable")
            left.append((kk[order, 0], ab[order], kc.num_partitions()))
    assert left[0][2] != left[1][2]                                         # (the two layouts differ)
    assert (left[0][0] == left[1][0]).all() and (left[0][1] == left[1][1]).all()


def test_max_rounds_and_max_passes_stop_where_the_restatement_stops(dev):
    k = 31
    stream, _, _ = bubbles_stream_of(k)
    tp, bp = stream_params(k)
    with count(stream, dev, k, abundance_min=1) as kc:
        kk, ab = kc.rows()
        p1 = pop(row_values(kk), ab, k, *bp, max_rounds=1)
        total = kc.pop_bubbles(*bp, max_rounds=1)
        assert total == p1.total and total["n_rounds"] == 1 and total["n_popped"] == 5
        assert row_values(kc.rows()[0]) == p1.values
        check_graph_of(kc, p1.last)                                         # twelve unitigs: the edges of the final rows are there
        assert kc.unitigs()["n_unitigs"] == 12
        total = kc.pop_bubbles(*bp)                                         # and the rest
        assert (total["n_rounds"], total["n_popped"], total["n_rows_popped"], kc.unitigs()["n_unitigs"]) == (1, 1, k + 6, 9)
        kc.count()
        s1 = simplify(row_values(kk), ab, k, tp, bp, max_passes=1)
        args = dict(tips=dict(max_nodes=tp[0]), bubbles=dict(max_nodes=bp[0], max_diff=bp[1]))
        total = kc.simplify(max_passes=1, **args)
        assert total == s1.total and total["n_passes"] == 1 and total["tips"]["n_tips"] == 0
        assert row_values(kc.rows()[0]) == s1.values and kc.unitigs()["n_unitigs"] == 9
        total = kc.simplify(**args)                                         # and the rest: the dead-end branch is a tip now
        assert (total["n_passes"], total["tips"]["n_rows_clipped"], total["bubbles"]["n_popped"], kc.unitigs()["n_unitigs"]) == (1, k + 6, 0, 7)


def test_one_half_alone(dev):
    k = 33
    stream, _, _ = bubbles_stream_of(k)
    tp, bp = stream_params(k)
    with count(stream, dev, k, abundance_min=1) as kc:
        n = kc.result_device()[2]
        total = kc.simplify(tips=dict(max_nodes=tp[0]), bubbles=False)
        assert total["n_passes"] == 0 and total["bubbles"] == dict(ZERO, n_rows_left=n) and total["tips"]["n_candidates"] == 1 and kc.result_device()[2] == n
        total = kc.simplify(tips=False, bubbles=dict(max_nodes=bp[0]))
        assert total["n_passes"] == 1 and total["tips"] == dict(ZERO_TIPS, n_rows_left=n - 6 * k - 6)
        assert (total["bubbles"]["n_popped"], total["bubbles"]["n_rounds"], total["n_rows_left"]) == (6, 2, n - 6 * k - 6)


# ------------------------------------------------------------------ 3. identities, no oracle, medium size
@pytest.fixture(scope="module")
def reads100k(dev):
    from dsk_amd import synth
    return synth.make_reads(synth.make_genome(300_000, dev), 100_000, 150)


def test_identities_on_the_reads(reads100k, dev):
    from dsk_amd import KmerCounter
    k = 31
    with KmerCounter(kmer_size=k, abundance_min=2) as kc:
        kc.set_reads_device(reads100k.data_ptr(), reads100k.numel())
        kc.count()
        n = kc.result_device()[2]
        assert n > 100_000
        row_pop, bits, st = kc.graph_bubbles_tensor(2 * k, 4)
        bits, row_pop = bits.cpu().numpy(), row_pop.cpu().numpy()
        off = kc.unitigs_table_tensor()[0].cpu().numpy()
        kinds = kc.unitigs_table_tensor()[2].cpu().numpy()
        unitig = kc.unitigs_rows_tensor()[0].cpu().numpy()
        e_off, e_tgt = (t.cpu().numpy().astype(np.int64) for t in kc.unitig_edges_tensor()[:2])
        deg = np.diff(e_off)
        nodes = np.diff(off) - k
        nu = len(nodes)
        cand, popped, in_bubble = bits & 1 != 0, bits & 2 != 0, bits & 4 != 0
        one = (deg[0::2] == 1) & (deg[1::2] == 1)
        first = e_tgt[np.minimum(e_off[:-1], max(len(e_tgt) - 1, 0))] if len(e_tgt) else np.zeros(2 * nu, np.int64)      # E(U)[0] where deg(U) > 0
        me = np.arange(nu)
        no_self = (first[0::2] >> 1 != me) & (first[1::2] >> 1 != me)
        assert (cand == ((kinds == 0) & (nodes <= 2 * k) & one & no_self)).all()
        assert not (popped & ~in_bubble).any() and not (in_bubble & ~cand).any()
        assert (row_pop == popped[unitig]).all()
        assert st == dict(n_candidates=int(cand.sum()), n_in_bubbles=int(in_bubble.sum()), n_popped=int(popped.sum()), n_rows_popped=int(nodes[popped].sum()),
                          n_rounds=1, n_rows_left=n - int(nodes[popped].sum()))
        assert st["n_popped"] > 0                                           # (the reads carry errors)
        total = kc.simplify()
        print("simplify stats", total)
        left = kc.result_device()[2]
        assert total["n_rows_left"] == left and left + total["tips"]["n_rows_clipped"] + total["bubbles"]["n_rows_popped"] == n
        assert total["n_passes"] >= 1 and total["bubbles"]["n_popped"] > 0 and total["tips"]["n_tips"] > 0
        assert kc.graph_bubbles(2 * k)["n_popped"] == 0 and kc.graph_tips(k)["n_tips"] == 0
        # the stream of the cleaned graph counts back to exactly the rows left
        kk, _ = kc.rows()
        text = kc.unitigs_stream_tensor()
        assert text.numel() == left + k * kc.unitigs()["n_unitigs"]
        with KmerCounter(kmer_size=k, abundance_min=1) as again:
            again.set_reads_device(text.data_ptr(), text.numel())
            again.count()
            k2, a2 = again.rows()
            assert again.stats()["n_kmers"] == left and (a2 == 1).all()
            assert len(k2) == left and (sorted_rows(k2) == sorted_rows(kk)).all()


# ------------------------------------------------------------------ 4. lifecycle and errors
def test_parameter_errors_and_null_pointers(dev):
    from dsk_amd import KmerCounter
    from dsk_amd.engine import _BubbleParams, _BubbleStats, _SimplifyStats, _TipParams
    k = 33
    stream, _, _ = bubbles_stream_of(k)
    buf = torch.zeros(1024, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with KmerCounter(kmer_size=k) as kc:
        for call in (lambda: kc.graph_bubbles(2 * k, 4, buf.data_ptr(), 0), kc.pop_bubbles, kc.simplify):
            assert code_of(call) == E_STATE                                  # no result
    with count(stream, dev, k, abundance_min=1) as kc:
        kk, ab = kc.rows()
        exp = BubbleRestatement(row_values(kk), ab, k, 2 * k, 4)
        n, nu = exp.n, exp.stats["n_unitigs"]
        for mn in (0, 65536):
            assert code_of(lambda: kc.graph_bubbles(mn)) == E_ARG
            assert code_of(lambda: kc.pop_bubbles(mn)) == E_ARG
            assert code_of(lambda: kc.simplify(bubbles=dict(max_nodes=mn))) == E_ARG
            assert code_of(lambda: kc.simplify(tips=dict(max_nodes=mn))) == E_ARG
        assert code_of(lambda: kc.pop_bubbles(2 * k, max_rounds=65)) == E_ARG
        assert code_of(lambda: kc.simplify(bubbles=dict(max_rounds=65))) == E_ARG
        assert code_of(lambda: kc.simplify(tips=dict(max_rounds=65))) == E_ARG
        assert code_of(lambda: kc.simplify(max_passes=17)) == E_ARG
        tip, par, st, sst = _TipParams(max_nodes=2 * k), _BubbleParams(max_nodes=2 * k, max_diff=4), _BubbleStats(), _SimplifyStats()
        assert kc._lib.dskgpu_graph_bubbles(kc._h, None, buf.data_ptr(), None, C.byref(st)) == E_ARG
        assert kc._lib.dskgpu_pop_bubbles(kc._h, None, C.byref(st)) == E_ARG
        assert kc._lib.dskgpu_simplify(kc._h, None, None, 0, C.byref(sst)) == E_ARG
        assert kc._lib.dskgpu_graph_bubbles(kc._h, C.byref(par), None, None, None) == E_ARG
        assert kc.result_device()[2] == n                                    # nothing was removed on the way
        assert kc.graph_bubbles(2 * k) == exp.bubble_stats                   # stats alone
        assert kc.graph_bubbles(2 * k, 0xFFFFFFFF)["n_popped"] == 6          # any max_diff: the longer branch is a sibling now
        # each output alone, inside its array
        r = torch.full((n + 64,), 249, dtype=torch.uint8, device=dev)
        u = torch.full((nu + 64,), 249, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        assert kc._lib.dskgpu_graph_bubbles(kc._h, C.byref(par), r.data_ptr(), None, None) == 0
        assert (u == 249).all() and (r[n:] == 249).all() and (r[:n].cpu().numpy() == exp.row_pop).all()
        assert kc._lib.dskgpu_graph_bubbles(kc._h, C.byref(par), None, u.data_ptr(), None) == 0
        assert (u[nu:] == 249).all() and (u[:nu].cpu().numpy() == exp.bits).all()
        assert kc._lib.dskgpu_pop_bubbles(kc._h, C.byref(par), None) == 0   # stats may be NULL
        assert kc.unitigs()["n_unitigs"] == 9
        assert kc._lib.dskgpu_simplify(kc._h, C.byref(tip), C.byref(par), 0, None) == 0
        assert kc.unitigs()["n_unitigs"] == 7


def test_max_diff_zero_means_equal_lengths_only(dev):
    k = 31
    stream, _, _ = bubbles_stream_of(k)
    with count(stream, dev, k, abundance_min=1) as kc:
        kk, ab = kc.rows()
        check_round(kc, BubbleRestatement(row_values(kk), ab, k, 2 * k, 0), 2 * k, 0)      # every bubble of the stream but the longer branch has equal lengths
        exp = BubbleRestatement(row_values(kk), ab, k, 2 * k, 6)
        st = check_round(kc, exp, 2 * k, 6)                                 # ... and with 6 the longer branch, read once, goes too
        assert (st["n_in_bubbles"], st["n_popped"]) == (13, 6)
        exp = BubbleRestatement(row_values(kk), ab, k, k, 4)                 # max_nodes = k: the branch of k + 5 rows is no candidate
        st = check_round(kc, exp, k, 4)
        assert st["n_popped"] == 5


def test_a_result_without_rows(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31, abundance_min=10 ** 6) as kc:
        assert kc.stats()["n_solid"] == 0
        r = torch.full((8,), 249, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        assert kc.graph_bubbles(62, 4, r.data_ptr(), r.data_ptr()) == ZERO
        assert (r == 249).all()
        row_pop, bits, st = kc.graph_bubbles_tensor(62)
        assert row_pop.numel() == 0 and bits.numel() == 0 and st == ZERO
        assert kc.pop_bubbles() == ZERO
        assert kc.simplify() == dict(n_passes=0, n_rows_left=0, tips=ZERO_TIPS, bubbles=ZERO)
        assert kc.unitig_edges() == dict(n_edges=0, n_self=0, n_dead_ends=0, max_degree=0)


def test_a_new_count_after_a_pop(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31, abundance_min=2) as kc:
        kk, ab = kc.rows()
        un = kc.unitigs()
        total = kc.simplify()
        assert total["bubbles"]["n_rows_popped"] == 806 and kc.unitigs()["n_unitigs"] == 75
        kc.count()
        k2, a2 = kc.rows()
        assert (k2 == kk).all() and (a2 == ab).all() and kc.unitigs() == un


def test_a_rank_of_a_group_is_a_state_error(oracle, golden_dir, dev):
    from dsk_amd import KmerGroup
    s = stream_of("golden", oracle, golden_dir)
    recs = bytes(s).split(b"\n")
    with KmerGroup([0, 0], kmer_size=31, abundance_min=2) as g:
        for r in range(2):
            g.rank(r).push_reads(b"\n".join(recs[r::2]) + b"\n")
        g.count()
        kc = g.rank(0)
        n = kc.stats()["n_solid"]
        assert n > 0
        for call in (lambda: kc.graph_bubbles(62), kc.pop_bubbles, kc.simplify, lambda: kc.simplify(tips=False)):
            assert code_of(call) == E_STATE
            assert "world_size" in kc._lib.dskgpu_last_error(kc._h).decode()
        assert kc.result_device()[2] == n


def test_stage_times_name_the_bubbles(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31, abundance_min=2, timing=True) as kc:
        before = dict(kc.stage_times())
        assert not any(n in before for n in ("bubbles", "tips", "filter rows", "unitig edges"))
        kc.graph_bubbles(62)
        one = dict(kc.stage_times())
        assert one["bubbles"] > 0 and one["unitig edges"] > 0 and "filter rows" not in one and "tips" not in one
        kc.pop_bubbles()
        two = dict(kc.stage_times())
        assert two["bubbles"] > one["bubbles"] and two["filter rows"] > 0 and two["unitig edges"] > one["unitig edges"] and "tips" not in two
        kc.simplify()
        after = dict(kc.stage_times())
        assert after["tips"] > 0 and after["bubbles"] > two["bubbles"] and after["filter rows"] > two["filter rows"]
        assert all(after[n] == v for n, v in before.items())
