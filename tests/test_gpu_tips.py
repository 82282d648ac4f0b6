"""The tips of the compacted de Bruijn graph, found and clipped on the device (include/dskgpu.h: dskgpu_graph_tips / dskgpu_clip_tips;
csrc/tips.h on the helpers of csrc/rules.h; the rows go through csrc/rowfilter.h).

All comparisons are exact.  Tests 1 to 3 compare the device with the restatement of tests/test_tips_restatement.py, made of the rows as the
context returns them: the bits of every unitig, the flag of every row, the stats of a round, and the rows a clip leaves.  Test 4 needs no
oracle and no restatement: identities on a medium-sized count.  All of it fails before the feature: KmerCounter has no graph_tips().
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from tests import test_gpu_unitig_edges as edges_mod      # noqa: E402
from tests import test_gpu_unitigs as unitigs_mod      # noqa: E402
from tests.test_gpu_unitigs import code_of, count, revcomp_str, row_values, sorted_rows, stream_of      # noqa: E402
from tests.test_tips_restatement import (TIPS_PINNED, TIPS_STREAM_K, TIPS_STREAM_ROUNDS, TipRestatement, clip,      # noqa: E402
                                         tips_stream)
from tests.test_unitig_edges_restatement import EdgeRestatement      # noqa: E402

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
ZERO = dict(n_candidates=0, n_tips=0, n_outranked=0, n_rows_clipped=0, n_rounds=0, n_rows_left=0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


_streams, _clipped = {}, {}


def tips_stream_of(k):
    if k not in _streams:
        _streams[k] = tips_stream(k)
    return _streams[k]


def clipped(kc, name, k, amin, order, max_nodes, max_abundance=0):
    """clip() of the rows of kc, cached per (input, k, abundance_min, row order, parameters) and never changed"""
    key = (name, k, amin, order, max_nodes, max_abundance)
    if key not in _clipped:
        kk, ab = kc.rows()
        _clipped[key] = clip(row_values(kk), ab, k, max_nodes, max_abundance)
    return _clipped[key]


def check_round(kc, exp, max_nodes, max_abundance=0):
    """one round on the device against the restatement of the same rows: bits, row flags, stats"""
    row_tip, unitig_tip, st = kc.graph_tips_tensor(max_nodes, max_abundance)
    assert row_tip.dtype == torch.uint8 and unitig_tip.dtype == torch.uint8
    print("tip stats", st, "expected", exp.tip_stats)
    bits, rows = unitig_tip.cpu().numpy(), row_tip.cpu().numpy()
    assert len(bits) == len(exp.bits) and (bits == exp.bits).all(), np.nonzero(bits != exp.bits)[0][:8]
    assert len(rows) == exp.n and (rows == exp.row_tip).all()
    assert st == exp.tip_stats
    return st


def check_graph_of(kc, exp):
    unitigs_mod.check_against_restatement(kc, exp)
    edges_mod.check_against_restatement(kc, exp)


# ------------------------------------------------------------------ 1. one round against the restatement
@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k,amin", [(31, 2), (63, 2), (15, 1)])
def test_golden_reads_match_the_restatement(oracle, golden_dir, dev, k, amin, partition_order):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, k, abundance_min=amin, partition_order=partition_order) as kc:
        c = clipped(kc, "golden", k, amin, partition_order, k)
        assert c.rounds == TIPS_PINNED[(k, amin, k, 0)]                     # the row order changes the numbering, never the counts
        kk, ab = kc.rows(); s0 = kc.stats(); u0 = unitigs_mod.device_answer(kc); e0 = edges_mod.device_edges(kc)
        check_round(kc, c.first, k)
        # the round changed nothing: rows, stats, unitigs and edges
        k2, a2 = kc.rows()
        assert (k2 == kk).all() and (a2 == ab).all() and kc.stats() == s0
        for before, after in zip(u0 + e0, unitigs_mod.device_answer(kc) + edges_mod.device_edges(kc)):
            assert (before == after) if isinstance(before, dict) else (before == after).all()


@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k", TIPS_STREAM_K)
def test_tips_stream(dev, k, partition_order):
    """a branch that forks into a weak and a strong end (the weak one is outranked; the branch goes in the second round) and a plain tip
    given as a reverse complement: every key width and its boundaries"""
    stream, M = tips_stream_of(k)
    mn = max(k, 31)
    with count(stream, dev, k, abundance_min=1, partition_order=partition_order) as kc:
        c = clipped(kc, "tips", k, 1, partition_order, mn)
        assert [(r[1], r[3], r[4], r[5]) for r in c.rounds] == TIPS_STREAM_ROUNDS
        st = check_round(kc, c.first, mn)
        assert (st["n_tips"], st["n_outranked"], st["n_rows_clipped"]) == (2, 1, 12)
        total = kc.clip_tips(mn)
        print("clip stats", total, "expected", c.total)
        assert total == c.total and total["n_rounds"] == 2
        un = kc.unitigs()
        assert un["n_unitigs"] == 1 and kc.result_device()[2] == len(M) - k + 1
        text = bytes(kc.unitigs_stream_tensor().cpu().numpy()).decode()
        assert text in (M + "\n", revcomp_str(M) + "\n")
        assert row_values(kc.rows()[0]) == c.values


# ------------------------------------------------------------------ 2. clip_tips against the restatement's clip
@pytest.mark.parametrize("partition_order", [False, True])
def test_clip_tips_on_every_kmer_of_the_golden_reads(oracle, golden_dir, dev, partition_order, tmp_path):
    k = 15
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, k, abundance_min=1, partition_order=partition_order) as kc:
        c = clipped(kc, "golden", k, 1, partition_order, k)
        s0, h0 = kc.stats(), kc.histogram()
        total = kc.clip_tips()                                              # max_nodes None = k
        print("clip stats", total, "expected", c.total)
        assert total == c.total and total["n_rounds"] == 2
        assert total["n_candidates"] == sum(r[2] for r in c.rounds) and total["n_tips"] == sum(r[3] for r in c.rounds)
        assert total["n_outranked"] == sum(r[4] for r in c.rounds) and total["n_rows_clipped"] == sum(r[5] for r in c.rounds)
        assert total["n_rows_left"] == kc.result_device()[2] == len(c.values)
        kk, ab = kc.rows()
        assert row_values(kk) == c.values and [int(a) for a in ab] == c.ab
        assert kc.stats() == s0 and (kc.histogram() == h0).all()            # the count's record
        check_graph_of(kc, c.last)                                          # what the context holds now: the graph of the rows left
        gfa = kc.write_gfa(str(tmp_path / "clean.gfa"))
        lines = open(str(tmp_path / "clean.gfa")).read().split("\n")
        assert gfa == dict(n_segments=c.last.stats["n_unitigs"], n_links=c.last.edge_stats["n_edges"])
        assert sum(1 for ln in lines if ln.startswith("S\t")) == c.last.stats["n_unitigs"]
        assert sum(1 for ln in lines if ln.startswith("L\t")) == c.last.edge_stats["n_edges"]
        st = kc.graph_tips(k)
        assert st["n_tips"] == 0 and st["n_rows_left"] == len(c.values)


def test_the_row_order_never_changes_the_kmers_left(oracle, golden_dir, dev):
    """the numbering differs between the row orders, the set of k-mers a clip leaves does not: both counted here, compared sorted"""
    stream = stream_of("golden", oracle, golden_dir)
    left = []
    for partition_order in (False, True):
        with count(stream, dev, 31, abundance_min=2, partition_order=partition_order) as kc:
            total = kc.clip_tips()
            assert (total["n_rounds"], total["n_rows_clipped"]) == (1, 1758)
            kk, ab = kc.rows()
            order = np.argsort(kk[:, 0], kind="stable")
            left.append((kk[order, 0], ab[order], kc.num_partitions()))
    assert left[0][2] != left[1][2]                                         # (the two layouts differ: 4 ranges against the partitions of the reference)
    assert (left[0][0] == left[1][0]).all() and (left[0][1] == left[1][1]).all()


def test_max_rounds_stops_after_one_round(dev):
    k = 31
    stream, _ = tips_stream_of(k)
    with count(stream, dev, k, abundance_min=1) as kc:
        kk, ab = kc.rows()
        c1 = clip(row_values(kk), ab, k, 31, max_rounds=1)
        total = kc.clip_tips(31, max_rounds=1)
        assert total == c1.total and total["n_rounds"] == 1 and total["n_rows_clipped"] == 12
        assert row_values(kc.rows()[0]) == c1.values
        check_graph_of(kc, c1.last)                                         # three unitigs: the edges of the final rows are there
        assert kc.unitigs()["n_unitigs"] == 3
        total = kc.clip_tips(31)                                            # and the rest
        assert (total["n_rounds"], total["n_rows_clipped"], kc.unitigs()["n_unitigs"]) == (1, 17, 1)


def test_max_abundance_one_on_every_kmer_of_the_golden_reads(oracle, golden_dir, dev):
    k = 31
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, k, abundance_min=1) as kc:
        c = clipped(kc, "golden", k, 1, False, k, 1)
        assert c.rounds == TIPS_PINNED[(k, 1, k, 1)]
        check_round(kc, c.first, k, 1)
        total = kc.clip_tips(k, max_abundance=1)
        assert total == c.total
        assert row_values(kc.rows()[0]) == c.values
        check_round(kc, c.last, k, 1)


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
        # every tip has one dead end and at most max_nodes rows, from the tables before
        row_tip, bits, st = kc.graph_tips_tensor(k)
        bits, row_tip = bits.cpu().numpy(), row_tip.cpu().numpy()
        off = kc.unitigs_table_tensor()[0].cpu().numpy()
        kinds = kc.unitigs_table_tensor()[2].cpu().numpy()
        unitig = kc.unitigs_rows_tensor()[0].cpu().numpy()
        deg = np.diff(kc.unitig_edges_tensor()[0].cpu().numpy())
        nodes = np.diff(off) - k
        cand, tip, outranked = bits & 1 != 0, bits & 2 != 0, bits & 4 != 0
        dead = (deg[0::2] == 0).astype(int) + (deg[1::2] == 0).astype(int)
        assert (cand == ((kinds == 0) & (nodes <= k) & (dead == 1))).all()
        assert not (tip & ~cand).any() and not (outranked & ~tip).any()
        assert (row_tip == tip[unitig]).all()
        assert st == dict(n_candidates=int(cand.sum()), n_tips=int(tip.sum()), n_outranked=int(outranked.sum()), n_rows_clipped=int(nodes[tip].sum()),
                          n_rounds=1, n_rows_left=n - int(nodes[tip].sum()))
        assert st["n_tips"] > 0                                             # (the reads carry errors)
        total = kc.clip_tips()
        print("clip stats", total)
        left = kc.result_device()[2]
        assert total["n_rows_left"] == left and left + total["n_rows_clipped"] == n and total["n_rounds"] >= 1 and total["n_tips"] >= st["n_tips"]
        assert kc.graph_tips(k)["n_tips"] == 0
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
    from dsk_amd.engine import _TipParams, _TipStats
    import ctypes as C
    k = 33
    stream, _ = tips_stream_of(k)
    buf = torch.zeros(1024, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with KmerCounter(kmer_size=k) as kc:
        for call in (lambda: kc.graph_tips(k, 0, buf.data_ptr(), 0), kc.clip_tips):
            assert code_of(call) == E_STATE                                  # no result
    with count(stream, dev, k, abundance_min=1) as kc:
        kk, ab = kc.rows()
        exp = TipRestatement(row_values(kk), ab, k, k)
        n, nu = exp.n, exp.stats["n_unitigs"]
        for mn in (0, 65536):
            assert code_of(lambda: kc.graph_tips(mn)) == E_ARG
            assert code_of(lambda: kc.clip_tips(mn)) == E_ARG
        assert code_of(lambda: kc.clip_tips(k, max_rounds=65)) == E_ARG
        par, st = _TipParams(max_nodes=k), _TipStats()
        assert kc._lib.dskgpu_graph_tips(kc._h, None, buf.data_ptr(), None, C.byref(st)) == E_ARG
        assert kc._lib.dskgpu_clip_tips(kc._h, None, C.byref(st)) == E_ARG
        assert kc._lib.dskgpu_graph_tips(kc._h, C.byref(par), None, None, None) == E_ARG
        assert kc.result_device()[2] == n                                    # nothing was clipped on the way
        assert kc.graph_tips(k) == exp.tip_stats                             # stats alone
        # each output alone, inside its array
        r = torch.full((n + 64,), 249, dtype=torch.uint8, device=dev)
        u = torch.full((nu + 64,), 249, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        assert kc._lib.dskgpu_graph_tips(kc._h, C.byref(par), r.data_ptr(), None, None) == 0
        assert (u == 249).all() and (r[n:] == 249).all() and (r[:n].cpu().numpy() == exp.row_tip).all()
        assert kc._lib.dskgpu_graph_tips(kc._h, C.byref(par), None, u.data_ptr(), None) == 0
        assert (u[nu:] == 249).all() and (u[:nu].cpu().numpy() == exp.bits).all()
        assert kc._lib.dskgpu_clip_tips(kc._h, C.byref(par), None) == 0     # stats may be NULL
        assert kc.unitigs()["n_unitigs"] == 1


def test_a_result_without_rows(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31, abundance_min=10 ** 6) as kc:
        assert kc.stats()["n_solid"] == 0
        r = torch.full((8,), 249, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        assert kc.graph_tips(31, 0, r.data_ptr(), r.data_ptr()) == ZERO
        assert (r == 249).all()
        row_tip, unitig_tip, st = kc.graph_tips_tensor(31)
        assert row_tip.numel() == 0 and unitig_tip.numel() == 0 and st == ZERO
        assert kc.clip_tips() == ZERO
        assert kc.unitig_edges() == dict(n_edges=0, n_self=0, n_dead_ends=0, max_degree=0)


def test_a_new_count_after_a_clip(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31, abundance_min=2) as kc:
        kk, ab = kc.rows()
        un = kc.unitigs()
        assert kc.clip_tips()["n_rows_clipped"] == 1758 and kc.unitigs()["n_unitigs"] == 153
        kc.count()
        k2, a2 = kc.rows()
        assert (k2 == kk).all() and (a2 == ab).all() and kc.unitigs() == un


def test_stage_times_name_the_tips_and_the_filter(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31, timing=True) as kc:
        before = dict(kc.stage_times())
        assert not any(n in before for n in ("tips", "filter rows", "unitig edges"))
        kc.graph_tips(31)
        one = dict(kc.stage_times())
        assert one["tips"] > 0 and one["unitig edges"] > 0 and "filter rows" not in one
        kc.clip_tips()
        after = dict(kc.stage_times())
        assert after["tips"] > one["tips"] and after["filter rows"] > 0 and after["unitig edges"] > one["unitig edges"]
        assert all(after[n] == v for n, v in before.items())
