"""The edges between the unitigs (include/dskgpu.h: dskgpu_unitig_edges / _edges_table; csrc/unitigs.h).

All comparisons are exact.  Test 1 compares the device with the string restatement of tests/test_unitig_edges_restatement.py, made of the
rows as the context returns them: offsets, targets in their order, ends and stats.  Test 2 needs no oracle and no restatement: identities
between the edges, the unitig stream and the adjacency bytes of a medium-sized count.  All of it fails before the feature: KmerCounter has
no unitig_edges().
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from tests.test_gpu_unitigs import code_of, count, revcomp_str, row_values, stream_of      # noqa: E402
from tests.test_unitig_edges_restatement import EDGES_PINNED, EdgeRestatement      # noqa: E402

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


_restated = {}


def restated(kc, name, k, amin, order):
    """the restatement of the rows of kc, cached per (input, k, abundance_min, row order) and never changed"""
    key = (name, k, amin, order)
    if key not in _restated:
        kk, ab = kc.rows()
        _restated[key] = EdgeRestatement(row_values(kk), ab, k)
        _restated[key].check_facts()
    return _restated[key]


def device_edges(kc):
    st = kc.unitig_edges()
    off, targets, ends = kc.unitig_edges_tensor()
    assert off.dtype == torch.int64 and targets.dtype == torch.int32 and ends.dtype == torch.int32
    return st, off.cpu().numpy(), targets.cpu().numpy().astype(np.int64), ends.cpu().numpy().astype(np.int64)


def check_against_restatement(kc, exp, pinned=None):
    st, off, targets, ends = device_edges(kc)
    print("unitig edge stats", st, "expected", exp.edge_stats, exp.hist)
    if pinned is not None:
        assert exp.summary() == pinned
    assert kc.unitigs()["n_unitigs"] == exp.stats["n_unitigs"]
    assert len(off) == len(exp.e_offsets) and (off == exp.e_offsets).all()
    assert len(ends) == len(exp.ends) and (ends == exp.ends).all()
    assert len(targets) == len(exp.e_targets) and (targets == exp.e_targets).all()
    assert st == exp.edge_stats
    return st


# ------------------------------------------------------------------ 1. the string restatement, every key width and boundary
@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k,amin", [(15, 2), (31, 2), (63, 2), (64, 2), (65, 2), (96, 2), (15, 1)])
def test_golden_reads_match_the_string_restatement(oracle, golden_dir, dev, k, amin, partition_order):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, k, abundance_min=amin, partition_order=partition_order) as kc:
        exp = restated(kc, "golden", k, amin, partition_order)
        st = check_against_restatement(kc, exp, EDGES_PINNED.get(("golden", k, amin)))
        if amin == 1:
            assert st["max_degree"] == 4


@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k", [1, 2, 15, 16, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128])
def test_handmade_stream(oracle, golden_dir, dev, k, partition_order):
    """the key-width boundaries; palindromes (even k), self-loops (poly-A, poly-C), the hairpin (the AT repeat at odd k) and the cycle (the AC repeat)"""
    name = "hand:%d" % k
    stream = stream_of(name, oracle, golden_dir)
    with count(stream, dev, k, abundance_min=1, partition_order=partition_order) as kc:
        exp = restated(kc, name, k, 1, partition_order)
        check_against_restatement(kc, exp, EDGES_PINNED.get(("hand", k, 1)))


@pytest.mark.parametrize("k", [31, 64, 97])
def test_long_chain_and_two_circles(oracle, golden_dir, dev, k):
    name = "circles:%d" % k
    stream = stream_of(name, oracle, golden_dir)
    with count(stream, dev, k, abundance_min=1) as kc:
        exp = restated(kc, name, k, 1, False)
        st = check_against_restatement(kc, exp, EDGES_PINNED.get(("circles", k, 1)))
        assert st == dict(n_edges=4, n_self=4, n_dead_ends=2, max_degree=1)


# ------------------------------------------------------------------ 2. identities, no oracle, medium size
@pytest.fixture(scope="module")
def reads100k(dev):
    from dsk_amd import synth
    return synth.make_reads(synth.make_genome(300_000, dev), 100_000, 150)


_COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACTG", b"TGAC"):
    _COMP[_a] = _b
_by_order = {}


@pytest.mark.parametrize("kind,kw", [
    ("global", dict()),
    ("partition_order", dict(partition_order=True)),
    ("multi_pass", dict(max_pass_mkeys=2)),
    ("no_sort", dict(sort=False)),
    ("two_banks_min", dict(solidity_kind="min")),
])
def test_edges_agree_with_the_stream_and_the_adjacency(reads100k, dev, kind, kw):
    from dsk_amd import KmerCounter
    k = 31
    with KmerCounter(kmer_size=k, abundance_min=2, **kw) as kc:
        kc.set_reads_device(reads100k.data_ptr(), reads100k.numel())
        if kind == "two_banks_min":
            kc.set_banks([reads100k.numel() // 2 // 151 * 151, reads100k.numel()])
        kc.count()
        if kind == "multi_pass":
            assert kc.stats()["n_passes"] > 1, kc.stats()
        n = kc.stats()["n_solid"]
        assert n > 100_000
        st, eoff, targets, ends = device_edges(kc)
        print("unitig edge stats", kind, st)
        nu = kc.unitigs()["n_unitigs"]
        ne = st["n_edges"]
        assert len(eoff) == 2 * nu + 1 and eoff[0] == 0 and eoff[-1] == ne == len(targets) and len(ends) == 2 * nu
        deg = np.diff(eoff)
        assert (deg >= 0).all() and int(deg.max()) == st["max_degree"] <= 4 and int((deg == 0).sum()) == st["n_dead_ends"]
        assert ends.min() >= 0 and ends.max() < 2 * n and (ne == 0 or (targets.min() >= 0 and targets.max() < 2 * nu))
        if kind == "global":
            assert ne > 1000                                                 # (the reads carry errors: tips and bubbles.  Solid in both banks: hardly any is left)
        src = np.repeat(np.arange(2 * nu, dtype=np.int64), deg)
        assert int(((src >> 1) == (targets >> 1)).sum()) == st["n_self"]

        # (a) the last k - 1 letters of seq(U) are the first k - 1 letters of seq(V)
        text = kc.unitigs_stream_tensor().cpu().numpy()
        off = kc.unitigs_table_tensor()[0].cpu().numpy()
        beg, end = off[:-1], off[1:] - 1                                     # seq(u) = text[beg[u] : end[u]]
        j = np.arange(k - 1, dtype=np.int64)[None, :]
        su, sv = src >> 1, targets >> 1
        tail_fw = text[end[su][:, None] - (k - 1) + j]
        tail_rc = _COMP[text[beg[su][:, None] + (k - 2) - j]]
        head_fw = text[beg[sv][:, None] + j]
        head_rc = _COMP[text[end[sv][:, None] - 1 - j]]
        tail = np.where((src & 1)[:, None] == 1, tail_rc, tail_fw)
        head = np.where((targets & 1)[:, None] == 1, head_rc, head_fw)
        assert (tail == head).all()

        # (b) the edges are the successors of the last nodes: the out-nibble of their rows' adjacency bytes
        adj = kc.graph_adjacency_tensor()[0].cpu().numpy()[ends >> 1].astype(np.int64)
        nib = np.where(ends & 1, adj >> 4, adj & 15)
        pop = np.array([bin(x).count("1") for x in range(16)], dtype=np.int64)
        assert (pop[nib] == deg).all() and int(pop[nib].sum()) == ne

        # (c) U -> V implies flip(V) -> flip(U) where neither unitig is a palindrome
        lens = end - beg
        pal = np.zeros(nu, dtype=bool)
        for u in np.nonzero(lens == k)[0]:
            s = bytes(text[beg[u]: end[u]]).decode()
            pal[u] = s == revcomp_str(s)
        keep = ~pal[su] & ~pal[sv]
        pairs = src * (2 ** 32) + targets
        assert len(np.unique(pairs)) == ne
        mirrored = (targets[keep] ^ 1) * (2 ** 32) + (src[keep] ^ 1)
        assert np.isin(mirrored, pairs).all()

        # (d) the row order changes the numbering, never the graph
        if kind in ("global", "partition_order"):
            _by_order[kind] = (ne, np.bincount(deg, minlength=5).tolist(), st["n_self"])
            if len(_by_order) == 2:
                assert _by_order["global"] == _by_order["partition_order"]


# ------------------------------------------------------------------ 3. GFA
@pytest.mark.parametrize("k", [31, 16])
def test_write_gfa(oracle, golden_dir, dev, k, tmp_path):
    stream = stream_of("hand:%d" % k, oracle, golden_dir)
    path = str(tmp_path / "graph.gfa")
    with count(stream, dev, k, abundance_min=1) as kc:
        kc.write_gfa(path)
        nu, ne = kc.unitigs()["n_unitigs"], kc.unitig_edges()["n_edges"]
        lines = bytes(kc.unitigs_stream_tensor().cpu().numpy()).decode().split("\n")[:-1]
        ab_sum = kc.unitigs_table_tensor()[1].cpu().numpy()
    recs = [ln.split("\t") for ln in open(path).read().split("\n") if ln]
    S = [r for r in recs if r[0] == "S"]
    L = [r for r in recs if r[0] == "L"]
    assert len(S) == nu and len(L) == ne and len(S) + len(L) + sum(1 for r in recs if r[0] == "H") == len(recs)
    assert [r[1] for r in S] == [str(u) for u in range(nu)]
    assert [r[2] for r in S] == lines
    assert [r[3] for r in S] == ["LN:i:%d" % len(s) for s in lines]
    assert [r[4] for r in S] == ["KC:i:%d" % int(a) for a in ab_sum]
    seq = {r[1]: r[2] for r in S}
    for _, u, su, v, sv, cigar in L:
        assert su in "+-" and sv in "+-" and cigar == "%dM" % (k - 1)
        a = seq[u] if su == "+" else revcomp_str(seq[u])
        b = seq[v] if sv == "+" else revcomp_str(seq[v])
        assert a[len(a) - (k - 1):] == b[: k - 1], (u, su, v, sv)


# ------------------------------------------------------------------ 4. lifecycle and errors
def test_before_any_count_is_a_state_error(dev):
    from dsk_amd import KmerCounter
    buf = torch.zeros(1024, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p = buf.data_ptr()
    with KmerCounter(kmer_size=31) as kc:
        for call in (kc.unitig_edges, lambda: kc.unitig_edges_table(p, 0, 0)):
            assert code_of(call) == E_STATE


def test_null_pointers_each_output_alone_and_guards(oracle, golden_dir, dev):
    name = "hand:33"
    stream = stream_of(name, oracle, golden_dir)
    with count(stream, dev, 33, abundance_min=1) as kc:
        exp = restated(kc, name, 33, 1, False)
        assert kc._lib.dskgpu_unitig_edges(kc._h, None) == 0                 # stats may be NULL
        assert kc._lib.dskgpu_unitig_edges_table(kc._h, None, None, None) == E_ARG
        st = kc.unitig_edges()
        assert st == exp.edge_stats                                          # and the context still answers
        n_or, ne = 2 * exp.stats["n_unitigs"], st["n_edges"]
        o = torch.full((n_or + 1 + 8,), -7, dtype=torch.int64, device=dev)
        t = torch.full((ne + 8,), -7, dtype=torch.int32, device=dev)
        e = torch.full((n_or + 8,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        kc.unitig_edges_table(o.data_ptr(), t.data_ptr(), e.data_ptr())
        assert (o[n_or + 1:] == -7).all() and (t[ne:] == -7).all() and (e[n_or:] == -7).all()
        assert (o[: n_or + 1].cpu().numpy() == exp.e_offsets).all() and (t[:ne].cpu().numpy() == exp.e_targets).all() and (e[:n_or].cpu().numpy() == exp.ends).all()
        for which in range(3):                                               # each output alone
            o2, t2, e2 = torch.full_like(o, -7), torch.full_like(t, -7), torch.full_like(e, -7)
            torch.cuda.synchronize()
            ptrs = [x.data_ptr() if i == which else 0 for i, x in enumerate((o2, t2, e2))]
            kc.unitig_edges_table(*ptrs)
            for i, (got, want) in enumerate(((o2, o), (t2, t), (e2, e))):
                assert (got == want).all() if i == which else (got == -7).all()


def test_a_result_without_rows(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31, abundance_min=10 ** 6) as kc:
        assert kc.stats()["n_solid"] == 0
        st = kc.unitig_edges()
        assert st == dict(n_edges=0, n_self=0, n_dead_ends=0, max_degree=0)
        o = torch.full((8,), -7, dtype=torch.int64, device=dev)
        t = torch.full((8,), -7, dtype=torch.int32, device=dev)
        e = torch.full((8,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        kc.unitig_edges_table(o.data_ptr(), t.data_ptr(), e.data_ptr())
        assert o[0] == 0 and (o[1:] == -7).all() and (t == -7).all() and (e == -7).all()
        off, targets, ends = kc.unitig_edges_tensor()
        assert off.tolist() == [0] and targets.numel() == 0 and ends.numel() == 0


def test_a_new_count_invalidates(oracle, golden_dir, dev):
    from dsk_amd import KmerCounter
    a = stream_of("golden", oracle, golden_dir)
    b = stream_of("hand:31", oracle, golden_dir)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    torch.cuda.synchronize()
    with KmerCounter(kmer_size=31, abundance_min=1) as kc:
        kc.set_reads_device(tb.data_ptr(), tb.numel())
        kc.count()
        exp_b = restated(kc, "hand:31", 31, 1, False)
        st_b = check_against_restatement(kc, exp_b)
        kc.set_reads_device(ta.data_ptr(), ta.numel())
        assert kc.unitig_edges() == st_b                                     # new reads alone change nothing: the result is still B's
        kc.count()
        st_a = kc.unitig_edges()
        off_a = kc.unitig_edges_tensor()[0]
        assert st_a != st_b and st_a["n_edges"] > 1000 and off_a.numel() == 2 * kc.unitigs()["n_unitigs"] + 1 and int(off_a[-1]) == st_a["n_edges"]
        kc.set_reads_device(tb.data_ptr(), tb.numel())
        kc.count()
        check_against_restatement(kc, exp_b)


def test_the_edge_calls_leave_the_kept_encoding_alone(reads100k, dev):
    """encode_reads() -> the 2-bit form is the only copy of the reads.  Count, edges, count again: identical rows, histogram and stats."""
    from dsk_amd import KmerCounter
    buf = reads100k.clone()
    torch.cuda.synchronize()
    with KmerCounter(kmer_size=31, abundance_min=2) as kc:
        kc.set_reads_device(buf.data_ptr(), buf.numel())
        kc.encode_reads()
        buf.zero_(); torch.cuda.synchronize()                              # the bytes are gone
        kc.count()
        k1, a1 = kc.rows(); h1 = kc.histogram(); s1 = kc.stats()
        e1 = kc.unitig_edges()
        t1 = kc.unitig_edges_tensor()
        k1b, a1b = kc.rows()
        assert (k1b == k1).all() and (a1b == a1).all() and kc.stats() == s1    # the result and the stats are untouched
        kc.count()
        k2, a2 = kc.rows()
        assert (k2 == k1).all() and (a2 == a1).all() and (kc.histogram() == h1).all()
        s2 = kc.stats()
        assert (s2["n_kmers"], s2["n_distinct"], s2["n_solid"]) == (s1["n_kmers"], s1["n_distinct"], s1["n_solid"])
        assert kc.unitig_edges() == e1 and all((x == y).all() for x, y in zip(kc.unitig_edges_tensor(), t1))


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
        assert kc.stats()["n_solid"] > 0
        for call in (kc.unitig_edges, lambda: kc.unitig_edges_table(p, 0, 0)):
            assert code_of(call) == E_STATE
            assert "world_size" in kc._lib.dskgpu_last_error(kc._h).decode()
        assert int(kc.graph_adjacency().sum()) == kc.stats()["n_solid"]      # the rank's context still answers what it can


def test_stage_times_name_the_edges(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31, timing=True) as kc:
        before = dict(kc.stage_times())
        assert not any(n in before for n in ("unitig edges", "unitigs", "graph", "query index"))
        kc.unitig_edges()
        after = dict(kc.stage_times())
        assert after["unitig edges"] > 0 and after["unitigs"] > 0 and after["query index"] > 0
        assert all(after[n] == v for n, v in before.items())
