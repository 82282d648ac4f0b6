"""The connected components of the compacted de Bruijn graph on the device, and the small ones taken out (include/dskgpu.h: dskgpu_components /
_components_labels / _components_table / dskgpu_graph_small_components / dskgpu_drop_components; csrc/components.h).

All comparisons are exact.  Tests 1 to 3 compare the device with the restatement of tests/test_components_restatement.py, made of the rows as
the context returns them: the label of every unitig and every row, the five columns of the table, the stats, the small flags and the rows a
drop leaves.  Test 4 needs no oracle and no restatement: identities on a medium-sized count, and the labels against a min-label fixpoint that
torch computes from the edge tensors.  All of it fails before the feature: KmerCounter has no components().
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from tests import test_gpu_unitig_edges as edges_mod      # noqa: E402
from tests import test_gpu_unitigs as unitigs_mod      # noqa: E402
from tests.test_components_restatement import (COLUMNS, COMPONENTS_PINNED, COMPONENTS_STREAM_DROP, COMPONENTS_STREAM_K, COMPONENTS_STREAM_STATS,      # noqa: E402
                                               ComponentRestatement, components_stream, drop_summary)
from tests.test_gpu_unitigs import code_of, count, row_values, stream_of      # noqa: E402

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
N_ROUNDS = 3                          # the header: the labelling is three launches whatever the graph
ZERO = dict(n_components=0, n_single=0, max_unitigs=0, max_rows=0, n_rounds=0)
ZERO_DROP = dict(n_small=0, n_unitigs_dropped=0, n_rows_dropped=0, n_rows_left=0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


_streams, _done = {}, {}


def components_stream_of(k):
    if k not in _streams:
        _streams[k] = components_stream(k)
    return _streams[k]


def restated(key, kc, k, base=None):
    """the restatement of the rows of a context, cached per (input, k, abundance_min, row order) and never changed"""
    if key not in _done:
        kk, ab = kc.rows()
        exp = ComponentRestatement(row_values(kk), ab, k, base=base)
        exp.check_component_facts()
        _done[key] = exp
    return _done[key]


def device_components(kc):
    st = kc.components()
    ucomp, rcomp = kc.components_labels_tensor()
    table = kc.components_table_tensor()
    assert ucomp.dtype == torch.int32 and rcomp.dtype == torch.int32 and table[0].dtype == torch.int32 and all(t.dtype == torch.int64 for t in table[1:])
    return st, ucomp.cpu().numpy().astype(np.int64), rcomp.cpu().numpy().astype(np.int64), [t.cpu().numpy().astype(np.int64) for t in table]


def check_against_restatement(kc, exp):
    st, ucomp, rcomp, table = device_components(kc)
    print("component stats", st, "expected", exp.comp_stats)
    assert len(ucomp) == len(exp.comp) and (ucomp == exp.comp).all(), np.nonzero(ucomp != exp.comp)[0][:8]
    assert len(rcomp) == exp.n and (rcomp == exp.row_comp).all()
    assert len(table[0]) == len(exp.first) and (table[0] == exp.first).all()
    for name, got in zip(COLUMNS, table[1:]):
        assert len(got) == len(exp.first) and (got == exp.table[name]).all(), name
    assert {n: st[n] for n in exp.comp_stats} == exp.comp_stats
    assert st["n_rounds"] == N_ROUNDS
    return st


def check_small(kc, exp, min_rows, max_abundance=0):
    row_drop, comp_small, st = kc.small_components_tensor(min_rows, max_abundance)
    sm, rows, want = exp.small(min_rows, max_abundance)
    print("small components", st, "expected", want)
    assert row_drop.dtype == torch.uint8 and comp_small.dtype == torch.uint8
    assert (comp_small.cpu().numpy() == sm).all() and (row_drop.cpu().numpy() == rows).all()
    assert st == want
    return st


def check_graph_of(kc, exp):
    unitigs_mod.check_against_restatement(kc, exp)
    edges_mod.check_against_restatement(kc, exp)


# ------------------------------------------------------------------ 1. the golden reads against the restatement
@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k,amin", [(31, 2), (63, 2), (96, 2), (15, 1)])
def test_golden_reads_match_the_restatement(oracle, golden_dir, dev, k, amin, partition_order):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, k, abundance_min=amin, partition_order=partition_order) as kc:
        base = edges_mod.restated(kc, "golden", k, amin, partition_order)      # (shared with the edge tests: made once per input)
        exp = restated(("golden", k, amin, partition_order), kc, k, base)
        assert exp.component_summary() == COMPONENTS_PINNED[("golden", k, amin)][0]      # the row order changes the numbering, never the counts
        kk, ab = kc.rows()
        s0 = kc.stats(); u0 = unitigs_mod.device_answer(kc); e0 = edges_mod.device_edges(kc)
        check_against_restatement(kc, exp)
        st = check_small(kc, exp, 2 * k)
        assert drop_summary(st) == COMPONENTS_PINNED[("golden", k, amin)][1]
        # the calls changed nothing: rows, stats, unitigs and edges
        k2, a2 = kc.rows()
        assert (k2 == kk).all() and (a2 == ab).all() and kc.stats() == s0
        for before, after in zip(u0 + e0, unitigs_mod.device_answer(kc) + edges_mod.device_edges(kc)):
            assert (before == after) if isinstance(before, dict) else (before == after).all()


# ------------------------------------------------------------------ 2. the components stream: a comb, circles, a lone k-mer, a lone chain
@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k", COMPONENTS_STREAM_K)
def test_components_stream(dev, k, partition_order):
    """one component of 121 unitigs whose numbers are scattered along a path of 61, a second comb, and four components of one unitig: every
    key width and its boundaries"""
    stream = components_stream_of(k)
    with count(stream, dev, k, abundance_min=1, partition_order=partition_order) as kc:
        kk, ab = kc.rows()
        exp = restated(("stream", k, partition_order), kc, k)
        assert exp.component_summary() == COMPONENTS_STREAM_STATS(k)
        st = check_against_restatement(kc, exp)
        assert st["n_rounds"] == N_ROUNDS
        st = check_small(kc, exp, 2 * k)
        assert drop_summary(st) == COMPONENTS_STREAM_DROP(k)
        assert drop_summary(check_small(kc, exp, 2 * k, 2)) == (2, 2, k + 1)    # the chain, read three times, is above max_abundance = 2
        assert drop_summary(check_small(kc, exp, 2)) == (1, 1, 1)
        key = ("stream drop", k, partition_order)
        if key not in _done:
            _done[key] = exp.drop(2 * k)
        new, want = _done[key]
        total = kc.drop_components(2 * k)
        print("drop stats", total, "expected", want)
        assert total == want
        k2, a2 = kc.rows()
        assert row_values(k2) == new.values and [int(a) for a in a2] == new.ab and kc.result_device()[2] == new.n
        check_graph_of(kc, new)                                             # what the context holds now: the graph of the rows left
        check_against_restatement(kc, new)
        dev0 = kc.result_device()
        again = kc.drop_components(2 * k)                                   # one application is final
        assert again == dict(ZERO_DROP, n_rows_left=new.n) and kc.result_device() == dev0
        check_against_restatement(kc, new)
        kc.count()                                                          # the full graph again
        assert (kc.rows()[0] == kk).all()
        check_against_restatement(kc, exp)


def test_the_table_by_one_add_per_unitig_is_the_same_table(dev, monkeypatch):
    """DSKGPU_CC_PLAIN (read when a context is created): the yardstick form of the table kernel against the restatement and the shipped form"""
    k = 31
    stream = components_stream_of(k)
    monkeypatch.setenv("DSKGPU_CC_PLAIN", "1")
    with count(stream, dev, k, abundance_min=1) as plain:
        monkeypatch.delenv("DSKGPU_CC_PLAIN")
        with count(stream, dev, k, abundance_min=1) as kc:
            exp = restated(("stream", k, False), kc, k)
            check_against_restatement(plain, exp)
            check_against_restatement(kc, exp)
            assert all(bool((a == b).all()) for a, b in zip(plain.components_table_tensor(), kc.components_table_tensor()))


# ------------------------------------------------------------------ 3. after simplify() on the golden reads
def test_after_simplify_on_the_golden_reads(oracle, golden_dir, dev, tmp_path):
    k = 31
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, k, abundance_min=2) as kc:
        s0, h0 = kc.stats(), kc.histogram()
        kc.simplify()
        exp = restated(("golden simplified", k, 2, False), kc, k)
        assert exp.n == 10532 and exp.stats["n_unitigs"] == 75              # (what the bubble tests fix for this input)
        check_against_restatement(kc, exp)
        if "golden simplified drop" not in _done:
            _done["golden simplified drop"] = exp.drop(2 * k)
        new, want = _done["golden simplified drop"]
        assert want["n_small"] > 0
        assert kc.drop_components(2 * k) == want
        gfa = kc.write_gfa(str(tmp_path / "clean.gfa"))
        lines = open(str(tmp_path / "clean.gfa")).read().split("\n")
        assert gfa == dict(n_segments=new.stats["n_unitigs"], n_links=new.edge_stats["n_edges"])
        segs = [ln.split("\t") for ln in lines if ln.startswith("S\t")]
        assert [s[2] for s in segs] == [new.seq(u) for u in range(new.stats["n_unitigs"])]
        links = [(2 * int(f[1]) + (f[2] == "-"), 2 * int(f[3]) + (f[4] == "-")) for f in (ln.split("\t") for ln in lines if ln.startswith("L\t"))]
        assert links == [(U, V) for U, e in enumerate(new.edges) for V in e]
        check_against_restatement(kc, new)
        assert kc.stats() == s0 and (kc.histogram() == h0).all()            # the count's record


# ------------------------------------------------------------------ 4. identities, no oracle, medium size
@pytest.fixture(scope="module")
def reads100k(dev):
    from dsk_amd import synth
    return synth.make_reads(synth.make_genome(300_000, dev), 100_000, 150)


def min_label_fixpoint(src, dst, nu):
    """the smallest unitig number reachable, by scatter_reduce_ over both directions of every entry until nothing changes"""
    lab = torch.arange(nu, dtype=torch.int64, device=src.device)
    a, b = torch.cat([src, dst]), torch.cat([dst, src])
    for _ in range(nu + 1):
        new = lab.clone().scatter_reduce_(0, a, lab[b], "amin")
        new = new[new]                                                      # (a shortcut per round: a label's label is in the same component)
        if bool((new == lab).all()):
            return lab
        lab = new
    raise AssertionError("no fixpoint")


@pytest.mark.parametrize("k,amin", [(31, 2), (21, 1)])
def test_identities_on_the_reads(reads100k, dev, k, amin):
    from dsk_amd import KmerCounter
    with KmerCounter(kmer_size=k, abundance_min=amin) as kc:
        kc.set_reads_device(reads100k.data_ptr(), reads100k.numel())
        kc.count()
        n = kc.result_device()[2]
        assert n > 100_000
        st = kc.components()
        print("component stats", st)
        ucomp, rcomp = (t.to(torch.int64) for t in kc.components_labels_tensor())
        first, unitigs, rows, ab_sum, edges = (t.to(torch.int64) for t in kc.components_table_tensor())
        off, ab_u, _ = kc.unitigs_table_tensor()
        unitig = kc.unitigs_rows_tensor()[0].to(torch.int64)
        e_off, e_tgt, _ = kc.unitig_edges_tensor()
        nu, nc, ne = off.numel() - 1, st["n_components"], int(e_off[-1])
        assert ucomp.numel() == nu and rcomp.numel() == n and first.numel() == nc and st["n_rounds"] == N_ROUNDS
        # the column sums
        assert int(unitigs.sum()) == nu and int(rows.sum()) == n and int(ab_sum.sum()) == int(ab_u.sum()) == int(torch.from_numpy(kc.rows()[1].astype(np.int64)).sum())
        assert int(edges.sum()) == ne == kc.unitig_edges()["n_edges"]
        assert st["n_single"] == int((unitigs == 1).sum()) and st["max_unitigs"] == int(unitigs.max()) and st["max_rows"] == int(rows.max())
        # every entry stays inside a component; the numbering
        src = torch.repeat_interleave(torch.arange(2 * nu, device=dev), e_off[1:] - e_off[:-1]) >> 1
        dst = e_tgt.to(torch.int64) >> 1
        assert src.numel() == ne and bool((ucomp[src] == ucomp[dst]).all())
        assert bool((ucomp[first] == torch.arange(nc, device=dev)).all()) and bool((first[1:] > first[:-1]).all())
        # the labels against the fixpoint
        lab = min_label_fixpoint(src, dst, nu)
        assert bool((first[ucomp] == lab).all())
        assert bool((rcomp == ucomp[unitig]).all())
        # the table against torch's sums over the labels
        L = (off[1:] - off[:-1]) - k
        assert bool((torch.zeros(nc, dtype=torch.int64, device=dev).index_add_(0, ucomp, L) == rows).all())
        assert bool((torch.zeros(nc, dtype=torch.int64, device=dev).index_add_(0, ucomp, ab_u) == ab_sum).all())
        assert bool((torch.zeros(nc, dtype=torch.int64, device=dev).index_add_(0, ucomp[src], torch.ones_like(src)) == edges).all())
        min_rows = 2 * k
        row_drop, comp_small, sm = kc.small_components_tensor(min_rows)
        assert bool((comp_small.to(torch.bool) == (rows < min_rows)).all()) and bool((row_drop == comp_small[rcomp]).all())
        assert sm == dict(n_small=int(comp_small.sum()), n_unitigs_dropped=int(unitigs[comp_small != 0].sum()), n_rows_dropped=int(row_drop.sum()),
                          n_rows_left=n - int(row_drop.sum()))
        total = kc.drop_components(min_rows)
        assert total == sm and kc.result_device()[2] == sm["n_rows_left"]
        assert kc.unitigs()["n_unitigs"] == nu - total["n_unitigs_dropped"]
        after = kc.components()
        assert after["n_components"] == nc - total["n_small"] and after["max_rows"] == st["max_rows"]


# ------------------------------------------------------------------ 5. the edges of the contract
def test_before_any_count_is_a_state_error(dev):
    from dsk_amd import KmerCounter
    buf = torch.zeros(1024, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p = buf.data_ptr()
    with KmerCounter(kmer_size=31) as kc:
        for call in (kc.components, lambda: kc.components_labels(p, 0), lambda: kc.components_table(p, 0, 0, 0, 0), lambda: kc.small_components(62, 0, p, 0),
                     lambda: kc.drop_components(62)):
            assert code_of(call) == E_STATE


def test_parameter_errors_null_pointers_and_guards(dev):
    from dsk_amd.engine import _ComponentDropStats, _ComponentParams
    k = 33
    stream = components_stream_of(k)
    with count(stream, dev, k, abundance_min=1) as kc:
        exp = restated(("stream", k, False), kc, k)
        n, nu, nc = exp.n, exp.stats["n_unitigs"], len(exp.first)
        par, bad, st = _ComponentParams(min_rows=2 * k), _ComponentParams(min_rows=0), _ComponentDropStats()
        buf = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        assert kc._lib.dskgpu_components(kc._h, None) == 0                  # stats may be NULL
        assert kc._lib.dskgpu_components_labels(kc._h, None, None) == E_ARG
        assert kc._lib.dskgpu_components_table(kc._h, None, None, None, None, None) == E_ARG
        assert kc._lib.dskgpu_graph_small_components(kc._h, C.byref(par), None, None, None) == E_ARG
        assert kc._lib.dskgpu_graph_small_components(kc._h, None, buf.data_ptr(), None, C.byref(st)) == E_ARG
        assert kc._lib.dskgpu_graph_small_components(kc._h, C.byref(bad), buf.data_ptr(), None, C.byref(st)) == E_ARG
        assert kc._lib.dskgpu_drop_components(kc._h, None, C.byref(st)) == E_ARG
        assert kc._lib.dskgpu_drop_components(kc._h, C.byref(bad), C.byref(st)) == E_ARG
        assert code_of(lambda: kc.small_components(0)) == E_ARG and code_of(lambda: kc.drop_components(0)) == E_ARG
        assert kc.result_device()[2] == n and (buf == 0).all()              # nothing was removed or written on the way
        assert kc.small_components(2 * k) == exp.small(2 * k)[2]            # stats alone
        G = 8

        def guarded(count_, dtype):
            return torch.full((count_ + 2 * G,), -7 if dtype != torch.uint8 else 249, dtype=dtype, device=dev)

        def inside(x, count_, want):
            fill = 249 if x.dtype == torch.uint8 else -7
            return bool((x[:G] == fill).all()) and bool((x[G + count_:] == fill).all()) and (x[G: G + count_].cpu().numpy().astype(np.int64) == np.asarray(want)).all()

        def untouched(x):
            return bool((x == (249 if x.dtype == torch.uint8 else -7)).all())

        # (G = 8 elements in front: the u32 outputs start 32 bytes, the u8 outputs 8 bytes into their allocation -- both store paths of the row kernels)
        for which in ((0, 1), (0,), (1,)):
            u, r = guarded(nu, torch.int32), guarded(n, torch.int32)
            torch.cuda.synchronize()
            kc.components_labels(u[G:].data_ptr() if 0 in which else 0, r[G:].data_ptr() if 1 in which else 0)
            assert inside(u, nu, exp.comp) if 0 in which else untouched(u)
            assert inside(r, n, exp.row_comp) if 1 in which else untouched(r)
        r = guarded(n + 1, torch.int32)                                    # ... and an output that is 4 bytes off a 16-byte boundary
        torch.cuda.synchronize()
        kc.components_labels(0, r[G + 1:].data_ptr())
        assert bool((r[: G + 1] == -7).all()) and bool((r[G + 1 + n:] == -7).all()) and (r[G + 1: G + 1 + n].cpu().numpy() == exp.row_comp).all()
        want = [exp.first] + [exp.table[name] for name in COLUMNS]
        for which in [tuple(range(5))] + [(i,) for i in range(5)]:
            bufs = [guarded(nc, torch.int32)] + [guarded(nc, torch.int64) for _ in range(4)]
            torch.cuda.synchronize()
            kc.components_table(*(b[G:].data_ptr() if i in which else 0 for i, b in enumerate(bufs)))
            for i, b in enumerate(bufs):
                assert inside(b, nc, want[i]) if i in which else untouched(b)
        sm, rows, _ = exp.small(2 * k)
        for which in ((0, 1), (0,), (1,)):
            for shift in (0, G):                                            # the row flags 16-byte aligned, and 8 bytes off
                rd, cs = torch.full((n + 2 * G + 16,), 249, dtype=torch.uint8, device=dev), guarded(nc, torch.uint8)
                torch.cuda.synchronize()
                a = (-rd.data_ptr()) % 16 + shift
                kc.small_components(2 * k, 0, rd[a:].data_ptr() if 0 in which else 0, cs[G:].data_ptr() if 1 in which else 0)
                if 0 in which:
                    assert bool((rd[:a] == 249).all()) and bool((rd[a + n:] == 249).all()) and (rd[a: a + n].cpu().numpy() == rows).all()
                else:
                    assert untouched(rd)
                assert inside(cs, nc, sm) if 1 in which else untouched(cs)
        assert kc._lib.dskgpu_drop_components(kc._h, C.byref(par), None) == 0   # stats may be NULL
        assert kc.components()["n_components"] == 3


def test_a_result_without_rows(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31, abundance_min=10 ** 6) as kc:
        assert kc.stats()["n_solid"] == 0
        assert kc.components() == ZERO
        r = torch.full((8,), 249, dtype=torch.uint8, device=dev)
        w = torch.full((8,), -7, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        kc.components_labels(w.data_ptr(), w.data_ptr())
        kc.components_table(w.data_ptr(), w.data_ptr(), w.data_ptr(), w.data_ptr(), w.data_ptr())
        assert kc.small_components(62, 0, r.data_ptr(), r.data_ptr()) == ZERO_DROP
        assert (r == 249).all() and (w == -7).all()
        ucomp, rcomp = kc.components_labels_tensor()
        assert ucomp.numel() == 0 and rcomp.numel() == 0 and all(t.numel() == 0 for t in kc.components_table_tensor())
        row_drop, comp_small, st = kc.small_components_tensor(62)
        assert row_drop.numel() == 0 and comp_small.numel() == 0 and st == ZERO_DROP
        assert kc.drop_components(62) == ZERO_DROP


def test_a_rank_of_a_group_is_a_state_error(oracle, golden_dir, dev):
    from dsk_amd import KmerGroup
    s = stream_of("golden", oracle, golden_dir)
    recs = bytes(s).split(b"\n")
    buf = torch.zeros(1024, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p = buf.data_ptr()
    with KmerGroup([0, 0], kmer_size=31, abundance_min=2) as g:
        for r in range(2):
            g.rank(r).push_reads(b"\n".join(recs[r::2]) + b"\n")
        g.count()
        kc = g.rank(0)
        n = kc.stats()["n_solid"]
        assert n > 0
        for call in (kc.components, lambda: kc.components_labels(p, 0), lambda: kc.components_table(p, 0, 0, 0, 0), lambda: kc.small_components(62),
                     lambda: kc.drop_components(62)):
            assert code_of(call) == E_STATE
            assert "world_size" in kc._lib.dskgpu_last_error(kc._h).decode()
        assert kc.result_device()[2] == n


def test_a_new_count_and_a_filter_invalidate(oracle, golden_dir, dev):
    k = 31
    a = stream_of("golden", oracle, golden_dir)
    b = components_stream_of(k)
    from dsk_amd import KmerCounter
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    torch.cuda.synchronize()
    with KmerCounter(kmer_size=k, abundance_min=1) as kc:
        kc.set_reads_device(tb.data_ptr(), tb.numel())
        kc.count()
        exp = restated(("stream", k, False), kc, k)
        st_b = check_against_restatement(kc, exp)
        kc.set_reads_device(ta.data_ptr(), ta.numel())
        assert kc.components() == st_b                                      # new reads alone change nothing: the result is still B's
        kc.count()
        st_a = kc.components()
        assert st_a != st_b and st_a["max_rows"] > 10000 and kc.components_labels_tensor()[0].numel() == kc.unitigs()["n_unitigs"]
        kc.set_reads_device(tb.data_ptr(), tb.numel())
        kc.count()
        check_against_restatement(kc, exp)
        # a filter of the caller's own: the rows of the large comb go, the components are those of the rows left
        big = int(np.argmax(exp.table["unitigs"]))
        keep = torch.from_numpy((exp.row_comp != big).astype(np.uint8)).to(dev)
        assert kc.filter_rows_tensor(keep) == exp.n - int(exp.table["rows"][big])
        st = kc.components()
        assert (st["n_components"], st["n_single"], st["max_unitigs"]) == (5, 4, 17)
        assert int(kc.components_table_tensor()[2].sum()) == kc.result_device()[2]


def test_stage_times_name_the_components(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31, abundance_min=2, timing=True) as kc:
        before = dict(kc.stage_times())
        assert not any(n in before for n in ("components", "small components", "filter rows", "unitig edges"))
        kc.components()
        one = dict(kc.stage_times())
        assert one["components"] > 0 and one["unitig edges"] > 0 and one["unitigs"] > 0 and "small components" not in one and "filter rows" not in one
        kc.components()                                                     # kept: nothing is built again
        assert dict(kc.stage_times())["components"] == one["components"]
        kc.small_components(62)
        two = dict(kc.stage_times())
        assert two["small components"] > 0 and two["components"] == one["components"] and "filter rows" not in two
        kc.drop_components(62)
        after = dict(kc.stage_times())
        assert after["small components"] > two["small components"] and after["filter rows"] > 0 and after["components"] > one["components"]
        assert after["unitig edges"] > one["unitig edges"]
        assert all(after[n] == v for n, v in before.items())


def test_the_component_calls_leave_the_kept_encoding_alone(reads100k, dev):
    """encode_reads() -> the 2-bit form is the only copy of the reads.  Count, components, count again: identical rows, histogram and stats."""
    from dsk_amd import KmerCounter
    buf = reads100k.clone()
    torch.cuda.synchronize()
    with KmerCounter(kmer_size=31, abundance_min=2) as kc:
        kc.set_reads_device(buf.data_ptr(), buf.numel())
        kc.encode_reads()
        buf.zero_(); torch.cuda.synchronize()                              # the bytes are gone
        kc.count()
        k1, a1 = kc.rows(); h1 = kc.histogram(); s1 = kc.stats()
        c1 = kc.components()
        t1 = kc.components_table_tensor()
        kc.small_components(62)
        k1b, a1b = kc.rows()
        assert (k1b == k1).all() and (a1b == a1).all() and kc.stats() == s1    # the result and the stats are untouched
        kc.drop_components(62)
        kc.count()
        k2, a2 = kc.rows()
        assert (k2 == k1).all() and (a2 == a1).all() and (kc.histogram() == h1).all()
        s2 = kc.stats()
        assert (s2["n_kmers"], s2["n_distinct"], s2["n_solid"]) == (s1["n_kmers"], s1["n_distinct"], s1["n_solid"])
        assert kc.components() == c1 and all((x == y).all() for x, y in zip(kc.components_table_tensor(), t1))
