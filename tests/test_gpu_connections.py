"""The erroneous connections of the compacted de Bruijn graph, found and removed on the device, and all three rules in turn
(include/dskgpu.h: dskgpu_graph_connections / dskgpu_remove_connections / dskgpu_simplify_all; csrc/connections.h).

All comparisons are exact.  Tests 1 and 2 compare the device with the restatement of tests/test_connections_restatement.py, made of the
rows as the context returns them: the bits of every unitig, the flag of every row, the stats of a round, and the rows a removal and a
simplify_all leave.  Test 3 needs no oracle and no restatement: the rule applied to the tables the device returns.  All of it fails before
the feature: KmerCounter has no graph_connections().
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from tests import test_gpu_graph as graph_mod      # noqa: E402
from tests import test_gpu_unitig_edges as edges_mod      # noqa: E402
from tests import test_gpu_unitigs as unitigs_mod      # noqa: E402
from tests.test_bubbles_restatement import BUBBLES_STREAM_K      # noqa: E402
from tests.test_connections_restatement import (CONNECTIONS_PINNED, CONNECTIONS_STREAM_ROUNDS, ConnectionRestatement, connections_stream,      # noqa: E402
                                                remove, simplify_all, stream_params_all)
from tests.test_gpu_unitigs import code_of, count, row_values, stream_of      # noqa: E402

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
ZERO = dict(n_candidates=0, n_one_sided=0, n_removed=0, n_rows_removed=0, n_rounds=0, n_rows_left=0)
ZERO_TIPS = dict(n_candidates=0, n_tips=0, n_outranked=0, n_rows_clipped=0, n_rounds=0, n_rows_left=0)
ZERO_BUBBLES = dict(n_candidates=0, n_in_bubbles=0, n_popped=0, n_rows_popped=0, n_rounds=0, n_rows_left=0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


_streams, _done = {}, {}


def connections_stream_of(k):
    if k not in _streams:
        _streams[k] = connections_stream(k)[0]
    return _streams[k]


def restated(key, make):
    """a restatement of the rows of a context, cached per (what, input, k, abundance_min, row order, parameters) and never changed"""
    if key not in _done:
        _done[key] = make()
    return _done[key]


def check_round(kc, exp, max_nodes, min_ratio=4, max_abundance=0):
    """one round on the device against the restatement of the same rows: bits, row flags, stats"""
    row_rem, bits, st = kc.graph_connections_tensor(max_nodes, min_ratio, max_abundance)
    assert row_rem.dtype == torch.uint8 and bits.dtype == torch.uint8
    print("connection stats", st, "expected", exp.connection_stats)
    bits, rows = bits.cpu().numpy(), row_rem.cpu().numpy()
    assert len(bits) == len(exp.bits) and (bits == exp.bits).all(), np.nonzero(bits != exp.bits)[0][:8]
    assert len(rows) == exp.n and (rows == exp.row_rem).all()
    assert st == exp.connection_stats
    return st


def check_graph_of(kc, exp):
    unitigs_mod.check_against_restatement(kc, exp)
    edges_mod.check_against_restatement(kc, exp)


def check_nothing_changed(kc, kk, ab, before):
    s0, u0, e0 = before
    k2, a2 = kc.rows()
    assert (k2 == kk).all() and (a2 == ab).all() and kc.stats() == s0
    for was, now in zip(u0 + e0, unitigs_mod.device_answer(kc) + edges_mod.device_edges(kc)):
        assert (was == now) if isinstance(was, dict) else (was == now).all()


# ------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k", BUBBLES_STREAM_K)
def test_connections_stream(dev, k, partition_order):
    """connections read once between strands read 12 and 20 times, one at the strict edge of the ratio, one into a strand read once, one a row
    too long, one given as a reverse complement and one that is weak only in round 2: every key width and its boundaries"""
    stream = connections_stream_of(k)
    tp, bp, cp = stream_params_all(k)
    with count(stream, dev, k, abundance_min=1, partition_order=partition_order) as kc:
        kk, ab = kc.rows()
        r, s = restated(("stream", k, partition_order), lambda: (remove(row_values(kk), ab, k, *cp), simplify_all(row_values(kk), ab, k, tp, bp, cp)))
        assert [x[1:] for x in r.rounds] == CONNECTIONS_STREAM_ROUNDS(k)
        before = (kc.stats(), unitigs_mod.device_answer(kc), edges_mod.device_edges(kc))
        st = check_round(kc, r.first, *cp)
        assert (st["n_candidates"], st["n_one_sided"], st["n_removed"], st["n_rows_removed"]) == (18, 3, 4, 5 * k - 3)
        check_nothing_changed(kc, kk, ab, before)
        total = kc.remove_connections(cp[0], cp[1])
        print("remove stats", total, "expected", r.total)
        assert total == r.total and (total["n_rounds"], total["n_removed"], total["n_rows_removed"]) == (2, 5, 6 * k - 4)
        assert row_values(kc.rows()[0]) == r.values and kc.result_device()[2] == len(r.values)
        assert kc.unitigs()["n_unitigs"] == 12
        text = kc.unitigs_stream_tensor().cpu().numpy()
        assert len(text) == len(r.last.stream) and (text == r.last.stream).all()
        kc.count()                                                          # the full graph again
        assert (kc.rows()[0] == kk).all()
        total = kc.simplify_all(tips=dict(max_nodes=tp[0], max_abundance=tp[1]), bubbles=dict(max_nodes=bp[0], max_diff=bp[1]),
                                connections=dict(max_nodes=cp[0], min_ratio=cp[1], max_abundance=cp[2]))
        print("simplify_all stats", total, "expected", s.total)
        assert total == s.total
        assert (total["n_rows_left"] == total["tips"]["n_rows_left"] == total["bubbles"]["n_rows_left"] == total["connections"]["n_rows_left"]
                == kc.result_device()[2] == len(s.values))
        k3, a3 = kc.rows()
        assert row_values(k3) == s.values and [int(a) for a in a3] == s.ab
        check_graph_of(kc, s.last)                                          # what the context holds now: the graph of the rows left


def test_max_rounds_stops_where_the_restatement_stops(dev):
    k = 31
    stream = connections_stream_of(k)
    with count(stream, dev, k, abundance_min=1) as kc:
        kk, ab = kc.rows()
        r1 = remove(row_values(kk), ab, k, 2 * k, 4, max_rounds=1)
        total = kc.remove_connections(max_rounds=1)                         # max_nodes: 2 k, min_ratio: 4
        assert total == r1.total and (total["n_rounds"], total["n_removed"]) == (1, 4)
        assert row_values(kc.rows()[0]) == r1.values
        check_graph_of(kc, r1.last)                                         # fifteen unitigs: the edges of the final rows are there
        assert kc.unitigs()["n_unitigs"] == 15
        total = kc.remove_connections()                                     # and the rest
        assert (total["n_rounds"], total["n_removed"], total["n_rows_removed"], kc.unitigs()["n_unitigs"]) == (1, 1, k - 1, 12)
        assert kc.remove_connections() == dict(ZERO, n_candidates=4, n_one_sided=2, n_rows_left=total["n_rows_left"])


@pytest.mark.parametrize("what,args", [("min_ratio = 2", (2, 0)), ("min_ratio = 5", (5, 0)), ("max_nodes = 2 k - 1", (4, 0)), ("max_abundance = 1", (4, 1))])
def test_other_parameters(dev, what, args):
    k = 33
    stream = connections_stream_of(k)
    max_nodes = 2 * k - 1 if what.startswith("max_nodes") else 2 * k
    with count(stream, dev, k, abundance_min=1) as kc:
        kk, ab = kc.rows()
        r = remove(row_values(kk), ab, k, max_nodes, *args)
        check_round(kc, r.first, max_nodes, *args)
        assert kc.remove_connections(max_nodes, *args) == r.total
        assert row_values(kc.rows()[0]) == r.values


def test_without_connections_simplify_all_is_simplify(dev):
    k = 33
    stream = connections_stream_of(k)
    tp, bp, _ = stream_params_all(k)
    args = dict(tips=dict(max_nodes=tp[0]), bubbles=dict(max_nodes=bp[0], max_diff=bp[1]))
    with count(stream, dev, k, abundance_min=1) as kc, count(stream, dev, k, abundance_min=1) as other:
        n = kc.result_device()[2]
        a, b = kc.simplify_all(connections=False, **args), other.simplify(**args)
        assert {name: a[name] for name in b} == b and a["connections"] == dict(ZERO, n_rows_left=b["n_rows_left"])
        assert b["n_rows_left"] == n - 4 * k                                # (the two heads of 2 k rows, clipped as tips)
        (k1, a1), (k2, a2) = kc.rows(), other.rows()
        assert (k1 == k2).all() and (a1 == a2).all()
        for x, y in zip(unitigs_mod.device_answer(kc) + edges_mod.device_edges(kc), unitigs_mod.device_answer(other) + edges_mod.device_edges(other)):
            assert (x == y) if isinstance(x, dict) else (x == y).all()
        kc.count()
        total = kc.simplify_all(tips=False, bubbles=False, connections=dict(max_nodes=2 * k))      # one part alone
        assert total["tips"] == dict(ZERO_TIPS, n_rows_left=n - 6 * k + 4) and total["bubbles"] == dict(ZERO_BUBBLES, n_rows_left=n - 6 * k + 4)
        assert (total["n_passes"], total["connections"]["n_removed"], total["connections"]["n_rounds"], kc.unitigs()["n_unitigs"]) == (1, 5, 2, 12)


# ------------------------------------------------------------------ 2. golden reads
@pytest.mark.parametrize("k,amin,partition_order", [(31, 2, False), (31, 2, True), (15, 2, False), (63, 2, False)])
def test_golden_reads_match_the_restatement(oracle, golden_dir, dev, k, amin, partition_order, tmp_path):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, k, abundance_min=amin, partition_order=partition_order) as kc:
        s0, h0 = kc.stats(), kc.histogram()
        kc.clip_tips()
        kc.pop_bubbles()
        kk, ab = kc.rows()
        r = restated(("remove", "golden", k, amin, partition_order), lambda: remove(row_values(kk), ab, k, 2 * k, 4))
        assert r.rounds == CONNECTIONS_PINNED[(k, amin)]                    # the row order changes the numbering, never the counts
        before = (kc.stats(), unitigs_mod.device_answer(kc), edges_mod.device_edges(kc))
        check_round(kc, r.first, 2 * k)
        check_nothing_changed(kc, kk, ab, before)
        total = kc.remove_connections()
        print("remove stats", total, "expected", r.total)
        assert total == r.total and total["n_rows_left"] == kc.result_device()[2] == len(r.values)
        k2, a2 = kc.rows()
        assert row_values(k2) == r.values and [int(a) for a in a2] == r.ab
        assert kc.stats() == s0 and (kc.histogram() == h0).all()            # the count's record
        check_graph_of(kc, r.last)
        gfa = kc.write_gfa(str(tmp_path / "clean.gfa"))
        lines = open(str(tmp_path / "clean.gfa")).read().split("\n")
        assert gfa == dict(n_segments=r.last.stats["n_unitigs"], n_links=r.last.edge_stats["n_edges"])
        assert sum(1 for ln in lines if ln.startswith("S\t")) == r.last.stats["n_unitigs"] == CONNECTIONS_PINNED[(k, amin)][-1][1]
        assert sum(1 for ln in lines if ln.startswith("L\t")) == r.last.edge_stats["n_edges"]
        assert kc.graph_connections(2 * k)["n_removed"] == 0


# ------------------------------------------------------------------ 3. the rule on the device's own tables, no oracle
def test_the_rule_holds_on_the_tables_of_synthetic_reads(dev):
    from dsk_amd import KmerCounter
    k, min_ratio = 31, 4
    stream = graph_mod.stream_of("tiny2000", None, None, dev)
    with count(stream, dev, k, abundance_min=1) as kc:
        n = kc.result_device()[2]
        row_rem, bits, st = kc.graph_connections_tensor(2 * k, min_ratio)
        bits, row_rem = bits.cpu().numpy(), row_rem.cpu().numpy()
        off, ab_sum, kinds = (t.cpu().numpy() for t in kc.unitigs_table_tensor())
        unitig = kc.unitigs_rows_tensor()[0].cpu().numpy()
        e_off, e_tgt = (t.cpu().numpy().astype(np.int64) for t in kc.unitig_edges_tensor()[:2])
        L, S = [int(x) - k for x in np.diff(off)], [int(x) for x in ab_sum]
        nu = len(L)
        assert nu > 1000
        E = [e_tgt[e_off[U]: e_off[U + 1]].tolist() for U in range(2 * nu)]
        want = np.zeros(nu, dtype=np.uint8)
        for u in range(nu):
            if not (kinds[u] == 0 and L[u] <= 2 * k and E[2 * u] and E[2 * u + 1] and all(V >> 1 != u for V in E[2 * u] + E[2 * u + 1])):
                continue
            weak = [any(S[w] * L[u] > min_ratio * S[u] * L[w] for w in ({V >> 1 for V in E[A]} | {X >> 1 for V in E[A] for X in E[V ^ 1]}) - {u})
                    for A in (2 * u, 2 * u + 1)]
            want[u] = 1 | (2 if weak[0] and weak[1] else 0) | (4 if weak[0] else 0) | (8 if weak[1] else 0)
        assert (bits == want).all(), np.nonzero(bits != want)[0][:8]
        cand, removed, one_sided = bits & 1 != 0, bits & 2 != 0, (bits & 4 != 0) != (bits & 8 != 0)
        assert not (removed & ~cand).any() and not (one_sided & ~cand).any() and not (removed & one_sided).any()
        assert (row_rem == removed[unitig]).all()
        rows_removed = int(np.asarray(L)[removed].sum())
        assert st == dict(n_candidates=int(cand.sum()), n_one_sided=int(one_sided.sum()), n_removed=int(removed.sum()), n_rows_removed=rows_removed,
                          n_rounds=1, n_rows_left=n - rows_removed)
        assert st["n_removed"] > 0 and st["n_one_sided"] > 0                # (the reads carry errors)
        total = kc.remove_connections(2 * k, min_ratio)
        print("remove stats", total)
        assert total["n_rounds"] >= 1 and total["n_rows_left"] == kc.result_device()[2] == n - total["n_rows_removed"]
        again = kc.remove_connections(2 * k, min_ratio)
        assert (again["n_rounds"], again["n_removed"], again["n_rows_removed"], again["n_rows_left"]) == (0, 0, 0, total["n_rows_left"])
        total = kc.simplify_all()
        print("simplify_all stats", total)
        left = kc.result_device()[2]
        assert total["n_rows_left"] == left
        assert left + total["tips"]["n_rows_clipped"] + total["bubbles"]["n_rows_popped"] + total["connections"]["n_rows_removed"] == again["n_rows_left"]
        assert kc.graph_connections(2 * k)["n_removed"] == 0 and kc.graph_bubbles(2 * k)["n_popped"] == 0 and kc.graph_tips(k)["n_tips"] == 0
        # the stream of the cleaned graph counts back to exactly the rows left
        kk, _ = kc.rows()
        text = kc.unitigs_stream_tensor()
        assert text.numel() == left + k * kc.unitigs()["n_unitigs"]
        with KmerCounter(kmer_size=k, abundance_min=1) as back:
            back.set_reads_device(text.data_ptr(), text.numel())
            back.count()
            k2, a2 = back.rows()
            assert len(k2) == left and (a2 == 1).all() and (unitigs_mod.sorted_rows(k2) == unitigs_mod.sorted_rows(kk)).all()


# ------------------------------------------------------------------ 4. lifecycle and errors
def test_parameter_errors_and_null_pointers(dev):
    from dsk_amd import KmerCounter
    from dsk_amd.engine import _BubbleParams, _ConnectionParams, _ConnectionStats, _SimplifyAllStats, _TipParams
    k = 33
    stream = connections_stream_of(k)
    buf = torch.zeros(1024, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with KmerCounter(kmer_size=k) as kc:
        for call in (lambda: kc.graph_connections(2 * k, 4, 0, buf.data_ptr(), 0), kc.remove_connections, kc.simplify_all):
            assert code_of(call) == E_STATE                                  # no result
    with count(stream, dev, k, abundance_min=1) as kc:
        kk, ab = kc.rows()
        exp = ConnectionRestatement(row_values(kk), ab, k, 2 * k, 4)
        n, nu = exp.n, exp.stats["n_unitigs"]
        for mn in (0, 65536):
            assert code_of(lambda: kc.graph_connections(mn)) == E_ARG
            assert code_of(lambda: kc.remove_connections(mn)) == E_ARG
            assert code_of(lambda: kc.simplify_all(connections=dict(max_nodes=mn))) == E_ARG
            assert code_of(lambda: kc.simplify_all(tips=dict(max_nodes=mn))) == E_ARG
            assert code_of(lambda: kc.simplify_all(bubbles=dict(max_nodes=mn))) == E_ARG
        for ratio in (0, 1, 256):
            assert code_of(lambda: kc.graph_connections(2 * k, ratio)) == E_ARG
            assert code_of(lambda: kc.remove_connections(2 * k, ratio)) == E_ARG
            assert code_of(lambda: kc.simplify_all(connections=dict(min_ratio=ratio))) == E_ARG
        assert code_of(lambda: kc.remove_connections(2 * k, max_rounds=65)) == E_ARG
        for part in ("tips", "bubbles", "connections"):
            assert code_of(lambda: kc.simplify_all(**{part: dict(max_rounds=65)})) == E_ARG
        assert code_of(lambda: kc.simplify_all(max_passes=17)) == E_ARG
        tip, bub, par = _TipParams(max_nodes=2 * k), _BubbleParams(max_nodes=2 * k, max_diff=4), _ConnectionParams(max_nodes=2 * k, min_ratio=4)
        st, sst = _ConnectionStats(), _SimplifyAllStats()
        assert kc._lib.dskgpu_graph_connections(kc._h, None, buf.data_ptr(), None, C.byref(st)) == E_ARG
        assert kc._lib.dskgpu_remove_connections(kc._h, None, C.byref(st)) == E_ARG
        assert kc._lib.dskgpu_simplify_all(kc._h, None, None, None, 0, C.byref(sst)) == E_ARG
        assert kc._lib.dskgpu_graph_connections(kc._h, C.byref(par), None, None, None) == E_ARG
        assert kc.result_device()[2] == n                                    # nothing was removed on the way
        assert kc.graph_connections(2 * k) == exp.connection_stats           # stats alone
        # each output alone, inside its array
        r = torch.full((n + 64,), 249, dtype=torch.uint8, device=dev)
        u = torch.full((nu + 64,), 249, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        assert kc._lib.dskgpu_graph_connections(kc._h, C.byref(par), r.data_ptr(), None, None) == 0
        assert (u == 249).all() and (r[n:] == 249).all() and (r[:n].cpu().numpy() == exp.row_rem).all()
        assert kc._lib.dskgpu_graph_connections(kc._h, C.byref(par), None, u.data_ptr(), None) == 0
        assert (u[nu:] == 249).all() and (u[:nu].cpu().numpy() == exp.bits).all()
        assert kc._lib.dskgpu_remove_connections(kc._h, C.byref(par), None) == 0      # stats may be NULL
        assert kc.unitigs()["n_unitigs"] == 12
        assert kc._lib.dskgpu_simplify_all(kc._h, C.byref(tip), C.byref(bub), C.byref(par), 0, None) == 0
        assert kc.graph_tips(2 * k)["n_tips"] == 0


def test_a_result_without_rows(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31, abundance_min=10 ** 6) as kc:
        assert kc.stats()["n_solid"] == 0
        r = torch.full((8,), 249, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        assert kc.graph_connections(62, 4, 0, r.data_ptr(), r.data_ptr()) == ZERO
        assert (r == 249).all()
        row_rem, bits, st = kc.graph_connections_tensor(62)
        assert row_rem.numel() == 0 and bits.numel() == 0 and st == ZERO
        assert kc.remove_connections() == ZERO
        assert kc.simplify_all() == dict(n_passes=0, n_rows_left=0, tips=ZERO_TIPS, bubbles=ZERO_BUBBLES, connections=ZERO)
        assert kc.unitig_edges() == dict(n_edges=0, n_self=0, n_dead_ends=0, max_degree=0)


def test_a_new_count_after_a_removal(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31, abundance_min=2) as kc:
        kk, ab = kc.rows()
        un = kc.unitigs()
        total = kc.simplify_all()
        assert (total["n_passes"], total["connections"]["n_removed"], total["connections"]["n_rows_removed"], kc.unitigs()["n_unitigs"]) == (1, 3, 93, 66)
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
        for call in (lambda: kc.graph_connections(62), kc.remove_connections, kc.simplify_all, lambda: kc.simplify_all(tips=False, bubbles=False)):
            assert code_of(call) == E_STATE
            assert "world_size" in kc._lib.dskgpu_last_error(kc._h).decode()
        assert kc.result_device()[2] == n


def test_stage_times_name_the_connections(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 15, abundance_min=2, timing=True) as kc:
        before = dict(kc.stage_times())
        assert not any(n in before for n in ("connections", "bubbles", "tips", "filter rows", "unitig edges"))
        kc.graph_connections(30)
        one = dict(kc.stage_times())
        assert one["connections"] > 0 and one["unitig edges"] > 0 and not any(n in one for n in ("filter rows", "tips", "bubbles"))
        kc.remove_connections()
        two = dict(kc.stage_times())
        assert two["connections"] > one["connections"] and two["filter rows"] > 0 and two["unitig edges"] > one["unitig edges"] and "tips" not in two
        kc.simplify_all()
        after = dict(kc.stage_times())
        assert after["tips"] > 0 and after["bubbles"] > 0 and after["connections"] > two["connections"]
        assert all(after[n] == v for n, v in before.items())
