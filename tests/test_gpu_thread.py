"""Reads threaded through the compacted de Bruijn graph on the device (include/dskgpu.h: dskgpu_thread_place / _reads / _walks / _support;
csrc/thread.h).

All comparisons are exact.  Part 1 compares the device with the string restatement of tests/test_thread_restatement.py (which the CPU
suite checks first): placements, walks, steps, ends, both supports and the stats.  Part 2 needs no restatement: identities that the
definition implies, on 100 000 reads, among them the edge support against a second count at k + 1.  Part 3 threads the original reads through
a simplified graph.  Part 4 is lifetime and errors.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests.test_gpu_unitigs import code_of, count, revcomp_str, row_values, stream_of      # noqa: E402
from tests.test_thread_restatement import THREAD_PINNED, ThreadRestatement, check_flipped, thread_stream      # noqa: E402

E_ARG, E_STATE = -1, -4
ZERO = dict(n_valid=0, n_placed=0, n_walks=0, n_steps=0, max_steps=0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


_restated, _threaded = {}, {}


def restated(kc, name, k, amin, order):
    """the restatement of the rows of kc, cached per (input, k, abundance_min, row order) and never changed"""
    key = (name, k, amin, order)
    if key not in _restated:
        kk, ab = kc.rows()
        _restated[key] = ThreadRestatement(row_values(kk), ab, k)
    return _restated[key]


def threaded(exp, key, stream):
    if key not in _threaded:
        _threaded[key] = exp.thread(stream)
        exp.check_facts(_threaded[key])
    return _threaded[key]


def on_device(stream, dev, odd=False):
    """the stream as a CUDA tensor; odd: at an odd device address"""
    if not odd:
        t = torch.from_numpy(stream).to(dev)
    else:
        buf = torch.zeros(len(stream) + 1, dtype=torch.uint8, device=dev)
        buf[1:] = torch.from_numpy(stream).to(dev)
        t = buf[1:]
        assert t.data_ptr() % 2 == 1 and t.is_contiguous()
    torch.cuda.synchronize()
    return t


def device_tables(kc):
    off, steps, first, last, ends = kc.thread_walks_tensor()
    assert off.dtype == torch.int64 and steps.dtype == torch.int32 and first.dtype == torch.int64 and last.dtype == torch.int64 and ends.dtype == torch.int32
    us, es = kc.thread_support_tensor()
    assert us.dtype == torch.int64 and es.dtype == torch.int64
    return [x.cpu().numpy().astype(np.int64) for x in (off, steps, first, last, ends, us, es)]


def check_against_restatement(kc, T, t):
    U, j = kc.thread_place_tensor(t)
    assert U.dtype == torch.int32 and j.dtype == torch.int32
    U, j = U.cpu().numpy().astype(np.int64), j.cpu().numpy().astype(np.int64)
    bad = np.nonzero((U != T.U) | (j != T.j))[0]
    assert len(U) == len(T.U) and len(bad) == 0, (len(bad), bad[:5], U[bad[:5]], T.U[bad[:5]], j[bad[:5]], T.j[bad[:5]])
    st = kc.thread_reads_tensor(t)
    print("thread stats", st, "expected", T.stats)
    assert st == T.stats
    off, steps, first, last, ends, us, es = device_tables(kc)
    for name, got, want in (("offsets", off, T.offsets), ("steps", steps, T.steps), ("first", first, T.first), ("last", last, T.last),
                            ("ends", ends, T.ends), ("unitig_support", us, T.unitig_support), ("edge_support", es, T.edge_support)):
        assert got.shape == want.shape and (got == want).all(), name
    return st


# ------------------------------------------------------------------ 1. the string restatement, every key width and boundary
@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k,amin", [(15, 2), (31, 2), (63, 2), (64, 2), (65, 2), (96, 2), (15, 1)])
def test_golden_reads_through_their_own_graph(oracle, golden_dir, dev, k, amin, partition_order):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, k, abundance_min=amin, partition_order=partition_order) as kc:
        exp = restated(kc, "golden", k, amin, partition_order)
        T = threaded(exp, ("golden", k, amin, partition_order), stream)
        if ("golden", k, amin) in THREAD_PINNED:
            assert exp.summary(T) == THREAD_PINNED[("golden", k, amin)]
        check_against_restatement(kc, T, kc._reads_keepalive)


@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k", [1, 2, 15, 16, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128])
def test_handmade_threading_stream(oracle, golden_dir, dev, k, partition_order):
    """the key-width boundaries; fragments of k - 1 and k letters, lower case, N, other separators, no separator at the end, a read and its
    reverse complement, the AC cycle, poly-A, the palindrome (even k), the AT hairpin, a substitution; and a stream shorter than k"""
    name = "hand:%d" % k
    with count(stream_of(name, oracle, golden_dir), dev, k, abundance_min=1, partition_order=partition_order) as kc:
        exp = restated(kc, name, k, 1, partition_order)
        stream, where = thread_stream(k)
        T = threaded(exp, (name, k, 1, partition_order), stream)
        check_flipped(exp, T, where)
        if ("hand", k, 1) in THREAD_PINNED:
            assert exp.summary(T) == THREAD_PINNED[("hand", k, 1)]
        if k >= 15:
            a, n = where["sub"]
            inside = [w for w in range(len(T.first)) if a <= T.first[w] < a + n]
            assert len(inside) == 2 and T.first[inside[1]] - T.last[inside[0]] == k + 1
        check_against_restatement(kc, T, on_device(stream, dev))
        if k > 1:
            short = stream[where["short"][0]: where["short"][0] + k - 1].copy()
            Ts = exp.thread(short)
            assert Ts.stats == ZERO
            check_against_restatement(kc, Ts, on_device(short, dev))


@pytest.mark.parametrize("k", [31, 64, 97])
def test_one_walk_over_many_blocks(oracle, golden_dir, dev, k):
    """one fragment along the long chain of circles_stream(k): 20 000 placed positions, one walk, one step -- the head and the last position
    lie twenty blocks of k_thread_emit apart.  Once from an even and once from an odd device address; nbytes is no multiple of 32."""
    name = "circles:%d" % k
    full = stream_of(name, oracle, golden_dir)
    chain = bytes(full).split(b"\n")[0]
    stream = np.frombuffer(chain + (b"" if len(chain) % 32 else b"\nAC"), dtype=np.uint8).copy()
    assert len(stream) % 32 != 0 and len(chain) == 20000 + k - 1
    with count(full, dev, k, abundance_min=1) as kc:
        exp = restated(kc, name, k, 1, False)
        T = threaded(exp, (name, k, 1, False), stream)
        assert T.stats == dict(n_valid=20000, n_placed=20000, n_walks=1, n_steps=1, max_steps=1)
        check_against_restatement(kc, T, on_device(stream, dev))
        check_against_restatement(kc, T, on_device(stream, dev, odd=True))


def test_every_window_a_walk_head(oracle, golden_dir, dev):
    """more than three blocks' worth of k-letter fragments of the golden reads: every placed position is a walk of its own"""
    k = 31
    golden = stream_of("golden", oracle, golden_dir)
    reads = [r for r in bytes(golden).split(b"\n") if len(r) >= 60]
    rng = np.random.default_rng(31)
    frags = [reads[int(r)][int(o): int(o) + k] for r, o in zip(rng.integers(0, len(reads), 5000), rng.integers(0, 60 - k, 5000))]
    stream = np.frombuffer(b"\n".join(frags), dtype=np.uint8).copy()
    assert len(stream) % 32 != 0
    with count(golden, dev, k, abundance_min=2) as kc:
        exp = restated(kc, "golden", k, 2, False)
        T = threaded(exp, ("fragments", k, 2, False), stream)
        assert T.stats["n_valid"] == 5000 and T.stats["n_walks"] == T.stats["n_placed"] == T.stats["n_steps"] > 3 * 1024 and T.stats["max_steps"] == 1
        check_against_restatement(kc, T, on_device(stream, dev))
        check_against_restatement(kc, T, on_device(stream, dev, odd=True))


# ------------------------------------------------------------------ 2. identities, no restatement, medium size
@pytest.fixture(scope="module")
def reads100k(dev):
    from dsk_amd import synth
    return synth.make_reads(synth.make_genome(300_000, dev), 100_000, 150)


_COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACTG", b"TGAC"):
    _COMP[_a] = _b


class Graph:
    """the tables of the compaction of kc on the host"""

    def __init__(self, kc, k):
        self.k = k
        self.text = kc.unitigs_stream_tensor().cpu().numpy()
        off, ab_sum, _ = kc.unitigs_table_tensor()
        self.off, self.ab_sum = off.cpu().numpy(), ab_sum.cpu().numpy()
        self.L = np.diff(self.off) - k
        eoff, targets, _ = kc.unitig_edges_tensor()
        self.eoff, self.targets = eoff.cpu().numpy(), targets.cpu().numpy().astype(np.int64)

    def text_of(self, U):
        s = bytes(self.text[self.off[U >> 1]: self.off[(U >> 1) + 1] - 1]).decode()
        return revcomp_str(s) if U & 1 else s


def implied_placements(n, L, off, steps, first, last, ends):
    """U and j of every position as the walks say them"""
    U, j = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int64)
    if len(first) == 0:
        return U, j
    ln = L[steps >> 1].copy()
    start = np.zeros(len(steps), dtype=np.int64)
    head, tail = off[:-1], off[1:] - 1
    start[head] = ends[:, 0]
    ln[head] -= ends[:, 0]
    ln[tail] -= L[steps[tail] >> 1] - 1 - ends[:, 1]
    assert (ln > 0).all()
    m = np.zeros(n + 1, dtype=np.int64)
    np.add.at(m, first, 1)
    np.add.at(m, last + 1, -1)
    placed = np.cumsum(m[:-1]) > 0
    assert int(placed.sum()) == int(ln.sum())
    U[placed] = np.repeat(steps, ln)
    within = np.arange(int(ln.sum()), dtype=np.int64) - np.repeat(np.cumsum(ln) - ln, ln)
    j[placed] = np.repeat(start, ln) + within
    return U, j


def check_walk_text(G, stream_np, off, steps, first, last, ends, w):
    k = G.k
    st = [int(U) for U in steps[off[w]: off[w + 1]]]
    glued = G.text_of(st[0]) + "".join(G.text_of(U)[k - 1:] for U in st[1:])
    cut = int(G.L[st[-1] >> 1]) - 1 - int(ends[w, 1])
    assert glued[int(ends[w, 0]): len(glued) - cut] == bytes(stream_np[first[w] - k + 1: last[w] + 1]).decode().upper(), w


def check_identities(kc, reads, k):
    st = kc.thread_reads_tensor(reads)
    off, steps, first, last, ends, us, es = device_tables(kc)
    G = Graph(kc, k)
    nw, ns = st["n_walks"], st["n_steps"]
    assert len(off) == nw + 1 and off[0] == 0 and off[-1] == ns == len(steps) and len(first) == len(last) == len(ends) == nw
    assert nw > 0 and (np.diff(off) >= 1).all() and int(np.diff(off).max()) == st["max_steps"]
    assert (first[1:] > last[:-1] + 1).all() and (first <= last).all()
    # the window count of every walk
    sums = np.add.reduceat(G.L[steps >> 1], off[:-1])
    assert (last - first + 1 == sums - ends[:, 0] - (G.L[steps[off[1:] - 1] >> 1] - 1 - ends[:, 1])).all()
    # the text of a sample of walks and of the walk with the most steps
    stream_np = reads.cpu().numpy()
    sample = np.random.default_rng(2000).choice(nw, size=min(2000, nw), replace=False)
    for w in list(sample) + [int(np.argmax(np.diff(off)))]:
        check_walk_text(G, stream_np, off, steps, first, last, ends, int(w))
    # the supports
    assert int(es.sum()) == ns - nw and int(us.sum()) == st["n_placed"]
    assert len(us) == len(G.ab_sum) and (us == G.ab_sum).all()              # one bank, solidity sum, no abundance_max, the counted reads
    # thread_place says what the walks say
    U, j = kc.thread_place_tensor(reads)
    Ui, ji = implied_placements(len(stream_np), G.L, off, steps, first, last, ends)
    assert (U.cpu().numpy() == Ui).all() and (j.cpu().numpy() == ji).all()
    assert st["n_placed"] == int((Ui >= 0).sum()) <= st["n_valid"]
    return st, G, (off, steps, first, last, ends, us, es)


@pytest.mark.parametrize("kind,kw", [
    ("global", dict()),
    ("partition_order", dict(partition_order=True)),
    ("multi_pass", dict(max_pass_mkeys=2)),
    ("no_sort", dict(sort=False)),
])
def test_identities_on_the_reads(reads100k, dev, kind, kw):
    from dsk_amd import KmerCounter
    k = 31
    with KmerCounter(kmer_size=k, abundance_min=2, **kw) as kc:
        kc.set_reads_device(reads100k.data_ptr(), reads100k.numel())
        kc.count()
        if kind == "multi_pass":
            assert kc.stats()["n_passes"] > 1, kc.stats()
        st, _, _ = check_identities(kc, reads100k, k)
        print("thread stats", kind, st)
        assert st["n_valid"] == kc.stats()["n_kmers"] and st["n_walks"] > 50_000


def test_every_kmer_a_row_places_every_window(reads100k, dev):
    from dsk_amd import KmerCounter
    k = 31
    with KmerCounter(kmer_size=k, abundance_min=1) as kc:
        kc.set_reads_device(reads100k.data_ptr(), reads100k.numel())
        kc.count()
        st = kc.thread_reads_tensor(reads100k)
        b = reads100k.cpu().numpy()
        base = np.isin(b, np.frombuffer(b"ACGTacgt", dtype=np.uint8))
        edge = np.diff(np.concatenate([[0], base.astype(np.int8), [0]]))
        runs = np.nonzero(edge == -1)[0] - np.nonzero(edge == 1)[0]
        assert st["n_placed"] == st["n_valid"] == kc.stats()["n_kmers"] and st["n_walks"] == int((runs >= k).sum())


@pytest.mark.parametrize("k", [31, 63])
def test_edge_support_against_a_second_count(reads100k, dev, k):
    """An edge U -> V is the (k+1)-mer text(U)[-k:] + text(V)[k-1].  Its abundance in a count of the same reads at k + 1 is the support of the
    edge plus that of its mirror V^1 -> U^1, which the reads walk when they come from the other strand; an edge that is its own mirror
    (V == U^1: the palindromic (k+1)-mer) is counted once.  No row is a palindrome at odd k, so every edge has its mirror."""
    from dsk_amd import KmerCounter
    from tests.test_gpu_unitigs import encode
    with KmerCounter(kmer_size=k, abundance_min=2) as kc:
        kc.set_reads_device(reads100k.data_ptr(), reads100k.numel())
        kc.count()
        kc.thread_reads_tensor(reads100k)
        G = Graph(kc, k)
        es = kc.thread_support_tensor()[1].cpu().numpy()
    ne = len(G.targets)
    assert ne == len(es) and ne > 1000
    src = np.repeat(np.arange(len(G.eoff) - 1, dtype=np.int64), np.diff(G.eoff))
    index = {(int(U), int(V)): e for e, (U, V) in enumerate(zip(src, G.targets))}
    texts = {}
    words = (k + 1 + 31) // 32
    keys = np.zeros((ne, words), dtype=np.uint64)
    want = np.zeros(ne, dtype=np.int64)
    for e, (U, V) in enumerate(zip(src, G.targets)):
        U, V = int(U), int(V)
        for X in (U, V):
            if X not in texts:
                texts[X] = G.text_of(X)
        s = texts[U][len(texts[U]) - k:] + texts[V][k - 1]
        v = min(encode(s), encode(revcomp_str(s)))
        for x in range(words):
            keys[e, x] = (v >> (64 * x)) & 0xFFFFFFFFFFFFFFFF
        m = index[(V ^ 1, U ^ 1)]
        want[e] = es[e] if m == e else es[e] + es[m]
    with KmerCounter(kmer_size=k + 1, abundance_min=1) as kc2:
        kc2.set_reads_device(reads100k.data_ptr(), reads100k.numel())
        kc2.count()
        t = torch.from_numpy(keys.view(np.int64)).to(dev)
        got = kc2.query_kmers_tensor(t if words > 1 else t[:, 0].contiguous()).cpu().numpy().astype(np.int64)
    assert (got == want).all(), (int((got != want).sum()), ne)
    assert int(want.max()) > 1


def test_two_pieces_cut_at_a_newline_concatenate(reads100k, dev):
    from dsk_amd import KmerCounter
    k = 31
    n = reads100k.numel()
    cut = 151 * 40_003
    assert int(reads100k[cut - 1]) == ord("\n") and 0 < cut < n
    with KmerCounter(kmer_size=k, abundance_min=2) as kc:
        kc.set_reads_device(reads100k.data_ptr(), reads100k.numel())
        kc.count()
        whole_st = kc.thread_reads_tensor(reads100k)
        whole = device_tables(kc)
        a_st = kc.thread_reads_tensor(reads100k[:cut])
        a = device_tables(kc)
        b_st = kc.thread_reads_tensor(reads100k[cut:])
        b = device_tables(kc)
    for name in ("n_valid", "n_placed", "n_walks", "n_steps"):
        assert whole_st[name] == a_st[name] + b_st[name], name
    assert whole_st["max_steps"] == max(a_st["max_steps"], b_st["max_steps"])
    assert (whole[0] == np.concatenate([a[0], b[0][1:] + a[0][-1]])).all()
    assert (whole[1] == np.concatenate([a[1], b[1]])).all()
    assert (whole[2] == np.concatenate([a[2], b[2] + cut])).all() and (whole[3] == np.concatenate([a[3], b[3] + cut])).all()
    assert (whole[4] == np.concatenate([a[4], b[4]])).all()
    assert (whole[5] == a[5] + b[5]).all() and (whole[6] == a[6] + b[6]).all()


# ------------------------------------------------------------------ 3. after a graph change
def test_the_original_reads_through_the_simplified_graph(oracle, golden_dir, dev):
    k = 31
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, k, abundance_min=2) as kc:
        before = restated(kc, "golden", k, 2, False)
        Tb = threaded(before, ("golden", k, 2, False), stream)
        kc.thread_reads_tensor(kc._reads_keepalive)
        sst = kc.simplify()
        assert 0 < sst["n_rows_left"] < before.n
        for call in (kc.thread_walks_tensor, kc.thread_support_tensor):        # the rows changed: the kept threading went with them
            assert code_of(call) == E_STATE
        kk, ab = kc.rows()
        after = ThreadRestatement(row_values(kk), ab, k)
        Ta = after.thread(stream)
        after.check_facts(Ta)
        check_against_restatement(kc, Ta, kc._reads_keepalive)
    # the walks break exactly at the k-mers that were removed
    gone = (Tb.U >= 0) & (Ta.U < 0)
    assert gone.any() and not ((Ta.U >= 0) & (Tb.U < 0)).any()
    text = Tb.text
    for p in np.nonzero(Tb.U >= 0)[0][:: 97]:
        w = text[p - k + 1: p + 1]
        assert (w in after.where) == (Ta.U[p] >= 0)
    assert int(gone.sum()) == Tb.stats["n_placed"] - Ta.stats["n_placed"]


# ------------------------------------------------------------------ 4. lifetime and errors
def test_before_any_count_is_a_state_error(dev):
    from dsk_amd import KmerCounter
    buf = torch.zeros(1024, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p = buf.data_ptr()
    with KmerCounter(kmer_size=31) as kc:
        for call in (lambda: kc.thread_place(p, 64, p, 0), lambda: kc.thread_reads(p, 64), lambda: kc.thread_reads(0, 0),
                     lambda: kc.thread_walks(p, 0, 0, 0, 0), lambda: kc.thread_support(p, 0)):
            assert code_of(call) == E_STATE


def test_table_calls_need_a_kept_threading(oracle, golden_dir, dev):
    """none yet; dropped by dskgpu_filter_rows; dropped by a new count"""
    stream = stream_of("golden", oracle, golden_dir)
    buf = torch.zeros(1024, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p = buf.data_ptr()
    with count(stream, dev, 31, abundance_min=2) as kc:
        t = kc._reads_keepalive
        tables = (lambda: kc.thread_walks(p, 0, 0, 0, 0), lambda: kc.thread_support(p, 0))
        for call in tables:
            assert code_of(call) == E_STATE
        kc.thread_place_tensor(t)                                            # stateless: keeps nothing
        for call in tables:
            assert code_of(call) == E_STATE
        st = kc.thread_reads_tensor(t)
        assert st["n_walks"] > 0 and kc.thread_walks_tensor()[0].numel() == st["n_walks"] + 1
        n = kc.result_device()[2]
        assert kc.filter_rows_tensor(torch.ones(n, dtype=torch.uint8, device=dev)) == n
        for call in tables:
            assert code_of(call) == E_STATE
        assert kc.thread_reads_tensor(t) == st                               # all rows kept: the same graph
        kc.count()
        for call in tables:
            assert code_of(call) == E_STATE
        assert kc.thread_reads_tensor(t) == st


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
        for call in (lambda: kc.thread_place(p, 64, p, 0), lambda: kc.thread_reads(p, 64)):
            assert code_of(call) == E_STATE
            assert "world_size" in kc._lib.dskgpu_last_error(kc._h).decode()
        for call in (lambda: kc.thread_walks(p, 0, 0, 0, 0), lambda: kc.thread_support(p, 0)):
            assert code_of(call) == E_STATE
        assert int(kc.graph_adjacency().sum()) == kc.stats()["n_solid"]      # the rank's context still answers what it can


def test_null_pointers_and_an_empty_stream(oracle, golden_dir, dev):
    name = "hand:33"
    with count(stream_of(name, oracle, golden_dir), dev, 33, abundance_min=1) as kc:
        exp = restated(kc, name, 33, 1, False)
        stream, _ = thread_stream(33)
        T = threaded(exp, (name, 33, 1, False), stream)
        t = on_device(stream, dev)
        p, n = t.data_ptr(), t.numel()
        out = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        lib, h = kc._lib, kc._h
        assert lib.dskgpu_thread_place(h, None, n, out.data_ptr(), None) == E_ARG
        assert lib.dskgpu_thread_place(h, p, n, None, None) == E_ARG
        assert lib.dskgpu_thread_reads(h, None, n, None) == E_ARG
        assert lib.dskgpu_thread_place(h, None, 0, None, None) == 0          # nothing to do
        assert lib.dskgpu_thread_reads(h, p, n, None) == 0                   # stats may be NULL
        assert lib.dskgpu_thread_walks(h, None, None, None, None, None) == E_ARG
        assert lib.dskgpu_thread_support(h, None, None) == E_ARG
        assert [int(x.sum()) for x in kc.thread_support_tensor()] == [T.stats["n_placed"], T.stats["n_steps"] - T.stats["n_walks"]]
        # an empty stream: all-zero stats, and the tables write offsets[0] = 0 only
        assert kc.thread_reads(0, 0) == ZERO
        o = torch.full((8,), -7, dtype=torch.int64, device=dev)
        others = [torch.full((8,), -7, dtype=torch.int64, device=dev) for _ in range(6)]
        torch.cuda.synchronize()
        kc.thread_walks(o.data_ptr(), *[x.data_ptr() for x in others[:4]])
        kc.thread_support(others[4].data_ptr(), others[5].data_ptr())
        assert o[0] == 0 and (o[1:] == -7).all() and all((x == -7).all() for x in others)
        check_against_restatement(kc, T, t)                                  # and the context still answers


def test_a_result_without_rows(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31, abundance_min=10 ** 6) as kc:
        assert kc.stats()["n_solid"] == 0
        t = kc._reads_keepalive
        U, j = kc.thread_place_tensor(t)
        assert (U == -1).all() and (j == 0).all()
        st = kc.thread_reads_tensor(t)
        assert st == dict(ZERO, n_valid=kc.stats()["n_kmers"]) and st["n_valid"] == 350000
        off, steps, first, last, ends = kc.thread_walks_tensor()
        assert off.tolist() == [0] and steps.numel() == first.numel() == last.numel() == ends.numel() == 0
        us, es = kc.thread_support_tensor()
        assert us.numel() == 0 and es.numel() == 0


def test_writes_stay_inside_their_arrays(oracle, golden_dir, dev):
    """guard words around every output; each output alone"""
    name = "hand:64"
    with count(stream_of(name, oracle, golden_dir), dev, 64, abundance_min=1) as kc:
        exp = restated(kc, name, 64, 1, False)
        stream, _ = thread_stream(64)
        T = threaded(exp, (name, 64, 1, False), stream)
        t = on_device(stream, dev)
        n = t.numel()
        G = 8

        def guarded(count_, dtype):
            return torch.full((count_ + 2 * G,), -7, dtype=dtype, device=dev)

        def inside(x, count_, want):
            return (x[:G] == -7).all() and (x[G + count_:] == -7).all() and (x[G: G + count_].cpu().numpy().astype(np.int64) == np.asarray(want).reshape(-1)).all()

        for which in ((0, 1), (0,), (1,)):
            U, j = guarded(n, torch.int32), guarded(n, torch.int32)
            torch.cuda.synchronize()
            kc.thread_place(t.data_ptr(), n, U[G:].data_ptr() if 0 in which else 0, j[G:].data_ptr() if 1 in which else 0)
            assert inside(U, n, T.U) if 0 in which else (U == -7).all()
            assert inside(j, n, T.j) if 1 in which else (j == -7).all()
        st = kc.thread_reads_tensor(t)
        nw, ns = st["n_walks"], st["n_steps"]
        nu, ne = exp.stats["n_unitigs"], exp.edge_stats["n_edges"]
        sizes = [(nw + 1, torch.int64, T.offsets), (ns, torch.int32, T.steps), (nw, torch.int64, T.first), (nw, torch.int64, T.last),
                 (2 * nw, torch.int32, T.ends)]
        for which in [tuple(range(5))] + [(i,) for i in range(5)]:
            bufs = [guarded(c, d) for c, d, _ in sizes]
            torch.cuda.synchronize()
            kc.thread_walks(*[b[G:].data_ptr() if i in which else 0 for i, b in enumerate(bufs)])
            for i, (b, (c, _, want)) in enumerate(zip(bufs, sizes)):
                assert inside(b, c, want) if i in which else (b == -7).all(), (which, i)
        for which in ((0, 1), (0,), (1,)):
            us, es = guarded(nu, torch.int64), guarded(ne, torch.int64)
            torch.cuda.synchronize()
            kc.thread_support(us[G:].data_ptr() if 0 in which else 0, es[G:].data_ptr() if 1 in which else 0)
            assert inside(us, nu, T.unitig_support) if 0 in which else (us == -7).all()
            assert inside(es, ne, T.edge_support) if 1 in which else (es == -7).all()


def test_threading_leaves_the_kept_encoding_alone(reads100k, dev):
    """encode_reads() -> the 2-bit form is the only copy of the reads.  Count, thread another stream, count again: identical rows, histogram
    and stats."""
    from dsk_amd import KmerCounter
    buf = reads100k.clone()
    torch.cuda.synchronize()
    with KmerCounter(kmer_size=31, abundance_min=2) as kc:
        kc.set_reads_device(buf.data_ptr(), buf.numel())
        kc.encode_reads()
        buf.zero_(); torch.cuda.synchronize()                              # the bytes are gone
        kc.count()
        k1, a1 = kc.rows(); h1 = kc.histogram(); s1 = kc.stats()
        other = reads100k[: 151 * 30_000]
        st = kc.thread_reads_tensor(other)
        kc.thread_place_tensor(other)
        w1 = kc.thread_walks_tensor()
        k1b, a1b = kc.rows()
        assert (k1b == k1).all() and (a1b == a1).all() and kc.stats() == s1    # the result and the stats are untouched
        kc.count()
        k2, a2 = kc.rows()
        assert (k2 == k1).all() and (a2 == a1).all() and (kc.histogram() == h1).all()
        s2 = kc.stats()
        assert (s2["n_kmers"], s2["n_distinct"], s2["n_solid"]) == (s1["n_kmers"], s1["n_distinct"], s1["n_solid"])
        assert kc.thread_reads_tensor(other) == st and all((x == y).all() for x, y in zip(kc.thread_walks_tensor(), w1))


def test_stage_times_name_the_threading(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31, timing=True) as kc:
        before = dict(kc.stage_times())
        assert not any(n in before for n in ("thread place", "thread walks", "unitig edges", "unitigs", "graph", "query index"))
        kc.thread_reads_tensor(kc._reads_keepalive)
        after = dict(kc.stage_times())
        assert after["thread place"] > 0 and after["thread walks"] > 0
        assert after["unitig edges"] > 0 and after["unitigs"] > 0 and after["query index"] > 0
        assert all(after[n] == v for n, v in before.items())
        kc.thread_place_tensor(kc._reads_keepalive)
        assert dict(kc.stage_times())["thread place"] > after["thread place"]


@pytest.mark.parametrize("k", [31, 16])
def test_write_gfa_walks(oracle, golden_dir, dev, k, tmp_path):
    name = "hand:%d" % k
    stream, _ = thread_stream(k)
    plain, walks = str(tmp_path / "graph.gfa"), str(tmp_path / "walks.gfa")
    with count(stream_of(name, oracle, golden_dir), dev, k, abundance_min=1) as kc:
        st = kc.thread_reads_tensor(on_device(stream, dev))
        off, steps, first, last, ends = (x.cpu().numpy() for x in kc.thread_walks_tensor())
        L = np.diff(kc.unitigs_table_tensor()[0].cpu().numpy()) - k
        n_plain = kc.write_gfa(plain)
        n_walks = kc.write_gfa_walks(walks)
    assert n_walks == dict(n_plain, n_paths=st["n_walks"])
    a = open(plain).read().split("\n")
    b = open(walks).read().split("\n")
    assert b[: len(a) - 1] == a[:-1]                                         # the S and L lines are write_gfa's
    P = [ln.split("\t") for ln in b[len(a) - 1:] if ln]
    assert len(P) == st["n_walks"] and all(r[0] == "P" and r[3] == "*" for r in P) and [r[1] for r in P] == ["w%d" % w for w in range(len(P))]
    seq = {r[1]: r[2] for r in (ln.split("\t") for ln in a) if r[0] == "S"}
    text = bytes(stream).decode().upper()
    for w, r in enumerate(P):
        segs = r[2].split(",")
        assert segs == ["%d%s" % (U >> 1, "-" if U & 1 else "+") for U in steps[off[w]: off[w + 1]]]
        parts = [seq[s[:-1]] if s[-1] == "+" else revcomp_str(seq[s[:-1]]) for s in segs]
        glued = parts[0] + "".join(x[k - 1:] for x in parts[1:])
        cut = int(L[int(segs[-1][:-1])]) - 1 - int(ends[w, 1])
        assert glued[int(ends[w, 0]): len(glued) - cut] == text[first[w] - k + 1: last[w] + 1], w
