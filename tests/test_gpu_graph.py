"""The rows' de Bruijn neighbours (include/dskgpu.h: dskgpu_graph_adjacency / dskgpu_graph_neighbors; csrc/graph.h).

All comparisons are exact.  The expected adjacency byte is a restatement on STRINGS, independent of the device's bit arithmetic: decode
the value with kmer_to_string, slice and append to get a neighbour string, reverse-complement the string, encode both, take the
smaller, look it up in a Python set of the oracle's solid values.  Test 4 needs no oracle: it asks the existing lookups instead.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
AMAX = 2147483647
KS = [1, 2, 15, 16, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128]
GOLDEN = "read50x_ref10K_e001.fasta.gz"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


# ------------------------------------------------------------------ the restatement on strings
_DIGITS = str.maketrans("ACTG", "0123")
_COMP = str.maketrans("ACTG", "TGAC")


def encode(s):
    return int(s.translate(_DIGITS), 4)


def revcomp_str(s):
    return s.translate(_COMP)[::-1]


def canonical(s):
    return min(encode(s), encode(revcomp_str(s)))


def adj_of(value, k, solid):
    """adj(value) by the definition, on the string of `value` (canonical or not)"""
    from dsk_amd.engine import kmer_to_string
    s = kmer_to_string(value, k)
    byte = 0
    for b, c in enumerate("ACTG"):
        if canonical(s[1:] + c) in solid:
            byte |= 1 << b
        if canonical(c + s[:-1]) in solid:
            byte |= 16 << b
    return byte


def degree_table(adj):
    adj = np.asarray(adj, dtype=np.uint8)
    pop = np.array([bin(i).count("1") for i in range(16)], dtype=np.int64)
    table = np.zeros((5, 5), dtype=np.uint64)
    np.add.at(table, (pop[adj >> 4], pop[adj & 15]), 1)
    return table


def to_int(row):
    return sum(int(w) << (64 * i) for i, w in enumerate(row))


def to_words(values, nw):
    return np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(nw)] for v in values], dtype=np.uint64).reshape(len(values), nw)


def row_values(kk):
    if kk.shape[1] == 1:
        return [int(v) for v in kk[:, 0]]
    return [to_int(r) for r in kk]


# ------------------------------------------------------------------ streams, references (computed once, shared, never changed)
def handmade_stream(k):
    """self-loops, two-base repeats, a palindrome (even k), a read and its reverse complement as separate reads, reads of k - 1 and k bases"""
    rng = np.random.default_rng(1000 + k)

    def rnd(n):
        return "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    reads = ["A" * (k + 5), "C" * (k + 5), "AT" * ((k + 21) // 2), "AC" * ((k + 21) // 2)]
    if k % 2 == 0:
        h = rnd(k // 2)
        reads.append(rnd(10) + h + revcomp_str(h) + rnd(10))
    r300 = rnd(300)
    reads += [r300, revcomp_str(r300), rnd(k - 1), rnd(k)]
    return np.frombuffer(("\n".join(reads) + "\n").encode(), dtype=np.uint8).copy()


_streams, _refs, _adj = {}, {}, {}


def stream_of(name, oracle, golden_dir, dev):
    if name not in _streams:
        if name == "golden":
            _streams[name] = np.ascontiguousarray(oracle.load_bank(os.path.join(golden_dir, GOLDEN))[0])
        elif name == "tiny2000":
            from dsk_amd import synth
            gl, nr, rl = synth.workload("tiny")
            _streams[name] = synth.make_reads(synth.make_genome(gl, dev), nr, rl).cpu().numpy()[: 151 * 2000].copy()
        else:
            _streams[name] = handmade_stream(int(name.split(":")[1]))
    return _streams[name]


def solid_values(oracle, name, stream, k, amin, amax=AMAX):
    """(list of the solid values as Python ints, the same as a set)"""
    if (name, k) not in _refs:
        ref = oracle.count(stream, k)
        _refs[(name, k)] = ([int(v) for v in ref.values()], ref.ab.copy())
    vals, ab = _refs[(name, k)]
    keep = [v for v, a in zip(vals, ab) if amin <= a <= amax]
    return keep, set(keep)


def expected_rows(oracle, name, stream, k, amin):
    """value -> adjacency byte of every solid row (the same for every row order: computed once)"""
    key = (name, k, amin)
    if key not in _adj:
        vals, solid = solid_values(oracle, name, stream, k, amin)
        _adj[key] = ({v: adj_of(v, k, solid) for v in vals}, solid)
    return _adj[key]


def count(stream, dev, k, **kw):
    from dsk_amd import KmerCounter
    kc = KmerCounter(kmer_size=k, **kw)
    t = torch.from_numpy(stream).to(dev)
    torch.cuda.synchronize()
    kc.set_reads_device(t.data_ptr(), t.numel())
    kc.count()
    kc._reads_keepalive = t
    return kc


def check_rows_against_restatement(kc, k, by_value, n_solid):
    kk, _ = kc.rows()
    assert len(kk) == n_solid == kc.stats()["n_solid"]
    adj, deg = kc.graph_adjacency_tensor()
    got = adj.cpu().numpy()
    exp = np.array([by_value[v] for v in row_values(kk)], dtype=np.uint8)
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, (k, len(bad), bad[:5], got[bad[:5]], exp[bad[:5]])
    assert deg.shape == (5, 5) and deg.dtype == np.uint64
    assert (deg == degree_table(exp)).all(), (k, deg, degree_table(exp))
    assert int(deg.sum()) == n_solid
    assert (kc.graph_adjacency() == deg).all()                            # the degree table alone, no bytes
    return got


# ------------------------------------------------------------------ 1. oracle parity, every key width and boundary
@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k", KS)
def test_adjacency_matches_the_string_restatement(oracle, golden_dir, dev, k, partition_order):
    """Fails before the feature: KmerCounter has no graph_adjacency_tensor."""
    names = (["golden"] if k <= 97 else []) + (["tiny2000"] if k >= 96 else [])
    windows = [2] + ([1] if k in (31, 64, 96) else [])
    for name in names:
        stream = stream_of(name, oracle, golden_dir, dev)
        for amin in windows:
            by_value, solid = expected_rows(oracle, name, stream, k, amin)
            assert len(solid) > 0
            with count(stream, dev, k, abundance_min=amin, partition_order=partition_order) as kc:
                got = check_rows_against_restatement(kc, k, by_value, len(solid))
            if name == "golden" and k == 31 and amin == 2:
                # isolated nodes, tips in both directions and both kinds of branching nodes are all there: one direction or one
                # nucleotide wrong cannot pass
                table = degree_table(got)
                assert len(got) == 13096
                assert table[0, 0] > 0 and table[0, 1] > 0 and table[1, 0] > 0 and table[1, 3] > 0 and table[3, 1] > 0


# ------------------------------------------------------------------ 2. hand-made stream
@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k", KS)
def test_handmade_stream(oracle, golden_dir, dev, k, partition_order):
    name = "hand:%d" % k
    stream = stream_of(name, oracle, golden_dir, dev)
    by_value, solid = expected_rows(oracle, name, stream, k, 1)
    assert canonical("A" * k) in solid and canonical("C" * k) in solid
    assert by_value[encode("A" * k)] & 0x11 == 0x11                       # the self-loop of poly-A: successor A and predecessor A
    with count(stream, dev, k, abundance_min=1, partition_order=partition_order) as kc:
        got = check_rows_against_restatement(kc, k, by_value, len(solid))
    if k <= 2:
        assert len(got) == (4 ** k + (4 ** (k // 2) if k % 2 == 0 else 0)) // 2      # all canonical k-mers are present ...
        assert (got == 0xFF).all()                                          # ... so every node has all eight neighbours


# ------------------------------------------------------------------ 3. graph_neighbors on arbitrary values
def neighbors(kc, values_w, dev, off=0):
    """adjacency bytes of a numpy (n x words) array; the output starts `off` bytes into a sentinel-filled allocation"""
    n = len(values_w)
    t = torch.from_numpy(np.ascontiguousarray(values_w).view(np.int64)).to(dev)
    out = torch.full((off + n + 64,), 249, dtype=torch.uint8, device=dev)                 # (249 = -7 as a byte)
    torch.cuda.synchronize()
    kc.graph_neighbors(t.data_ptr(), n, out.data_ptr() + off)
    res = out.cpu().numpy()
    assert (res[:off] == 249).all() and (res[off + n:] == 249).all(), "graph_neighbors wrote outside its n bytes"
    return res[off: off + n]


@pytest.mark.parametrize("k", [31, 64, 96, 128])
def test_neighbors_of_arbitrary_values(oracle, golden_dir, dev, k):
    name = "golden" if k <= 97 else "tiny2000"
    stream = stream_of(name, oracle, golden_dir, dev)
    by_value, solid = expected_rows(oracle, name, stream, k, 2)
    with count(stream, dev, k, abundance_min=2) as kc:
        kk, _ = kc.rows()
        if len(kk) % 512 == 0:
            kk = kk[:-1]
        vals = row_values(kk)
        nw = kk.shape[1]
        adj = kc.graph_adjacency_tensor()[0].cpu().numpy()[: len(kk)]
        # (a) the rows themselves, (e) at both alignments of the output, n no multiple of a block's share
        for off in (0, 3):
            assert (neighbors(kc, kk, dev, off) == adj).all(), (k, off)
        assert (kc.graph_neighbors_tensor(torch.from_numpy(kk.view(np.int64)).to(dev)).cpu().numpy() == adj).all()
        # (b) the reverse complements of the non-palindromic rows: not canonical, no rows themselves
        rc = [encode(revcomp_str(kmer_string(v, k))) for v in vals]
        rc = [r for r, v in zip(rc, vals) if r != v]
        assert len(rc) > len(vals) // 2 and not any(r in solid for r in rc[:100])
        exp = np.array([adj_of(r, k, solid) for r in rc], dtype=np.uint8)
        got = neighbors(kc, to_words(rc, nw), dev)
        assert (got == exp).all(), (k, int((got != exp).sum()))
        assert (exp != 0).any()
        # (c) one bit flipped (bit 2 * (row % k) + row % 2 of the value: every base position, both bits)
        idx = np.arange(len(kk))
        bit = (2 * (idx % k) + idx % 2).astype(np.uint64)
        flipped = kk.copy()
        flipped[idx, (bit // np.uint64(64)).astype(np.int64)] ^= np.uint64(1) << (bit % np.uint64(64))
        exp = np.array([adj_of(v, k, solid) for v in row_values(flipped)], dtype=np.uint8)
        got = neighbors(kc, flipped, dev, 3)
        assert (got == exp).all(), (k, int((got != exp).sum()))


def kmer_string(v, k):
    from dsk_amd.engine import kmer_to_string
    return kmer_to_string(v, k)


@pytest.mark.parametrize("k", [15, 31, 33, 97])
def test_values_that_are_no_kmers_answer_zero(oracle, golden_dir, dev, k):
    """(d) a value >= 4^k: the rows with one bit at or above 2k set in their ABI words"""
    stream = stream_of("golden", oracle, golden_dir, dev)
    with count(stream, dev, k, abundance_min=2) as kc:
        kk, _ = kc.rows()
        adj = kc.graph_adjacency_tensor()[0].cpu().numpy()
        assert (adj != 0).sum() > len(kk) // 2
        nw = kk.shape[1]
        idx = np.arange(len(kk))
        free = 64 * nw - 2 * k                                              # bits of the ABI words above the k-mer
        bit = (2 * k + idx % free).astype(np.uint64)
        big = kk.copy()
        big[idx, (bit // np.uint64(64)).astype(np.int64)] |= np.uint64(1) << (bit % np.uint64(64))
        assert (neighbors(kc, big, dev) == 0).all()
        assert (neighbors(kc, kk, dev) == adj).all()


# ------------------------------------------------------------------ 4. against the existing lookups, medium size, no oracle
@pytest.fixture(scope="module")
def reads100k(dev):
    from dsk_amd import synth
    return synth.make_reads(synth.make_genome(300_000, dev), 100_000, 150)


def rev_pairs_np(x):
    """reverse the 32 two-bit groups of every uint64"""
    x = x.copy()
    for sh, m in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF)):
        m = np.uint64(m)
        x = ((x >> np.uint64(sh)) & m) | ((x & m) << np.uint64(sh))
    return (x >> np.uint64(32)) | (x << np.uint64(32))


def canonical_np(x, k):
    mask = np.uint64((1 << (2 * k)) - 1)
    rc = (rev_pairs_np(x) >> np.uint64(64 - 2 * k)) ^ (np.uint64(0xAAAAAAAAAAAAAAAA) & mask)
    return np.minimum(x, rc)


def adjacency_by_queries(kc, dev, k):
    """the eight neighbour values of every row in numpy uint64 arithmetic, canonicalised, asked through query_kmers_tensor"""
    assert k <= 31
    x = kc.rows()[0][:, 0]
    mask = np.uint64((1 << (2 * k)) - 1)
    adj = np.zeros(len(x), dtype=np.uint8)
    for b in range(4):
        for j, nb in ((b, ((x << np.uint64(2)) | np.uint64(b)) & mask), (4 + b, (x >> np.uint64(2)) | (np.uint64(b) << np.uint64(2 * k - 2)))):
            q = torch.from_numpy(canonical_np(nb, k).view(np.int64)).to(dev)
            adj |= ((kc.query_kmers_tensor(q).cpu().numpy() != 0).astype(np.uint8) << j).astype(np.uint8)
    return adj


@pytest.mark.parametrize("kind,kw", [
    ("global", dict()),
    ("partition_order", dict(partition_order=True)),
    ("multi_pass", dict(max_pass_mkeys=2)),
    ("no_sort", dict(sort=False)),
    ("two_banks_min", dict(solidity_kind="min")),
])
def test_adjacency_equals_eight_lookups(reads100k, dev, kind, kw):
    from dsk_amd import KmerCounter
    with KmerCounter(kmer_size=31, abundance_min=2, **kw) as kc:
        kc.set_reads_device(reads100k.data_ptr(), reads100k.numel())
        if kind == "two_banks_min":
            kc.set_banks([reads100k.numel() // 2 // 151 * 151, reads100k.numel()])
        kc.count()
        if kind == "multi_pass":
            assert kc.stats()["n_passes"] > 1, kc.stats()
        exp = adjacency_by_queries(kc, dev, 31)
        adj, deg = kc.graph_adjacency_tensor()
        got = adj.cpu().numpy()
        assert len(got) == kc.stats()["n_solid"] > 100_000
        assert (got == exp).all(), (kind, int((got != exp).sum()))
        assert (deg == degree_table(exp)).all()


# ------------------------------------------------------------------ 5. two ranks on one device
@pytest.mark.parametrize("k", [15, 31, 63])
def test_group_adjacency_is_the_or_over_the_ranks(oracle, golden_dir, dev, k):
    from dsk_amd import KmerGroup
    s = stream_of("golden", oracle, golden_dir, dev)
    recs = bytes(s).split(b"\n")
    with count(s, dev, k, abundance_min=2) as kc:
        kk, _ = kc.rows()
        single = kc.graph_adjacency_tensor()[0].cpu().numpy()
    assert (single != 0).any()
    rows_t = torch.from_numpy(kk.view(np.int64)).to(dev)
    with KmerGroup([0, 0], kmer_size=k, abundance_min=2) as g:
        for r in range(2):
            g.rank(r).push_reads(b"\n".join(recs[r::2]) + b"\n")
        g.count()
        per_rank = [g.rank(r).graph_neighbors_tensor(rows_t).cpu().numpy() for r in range(2)]
    assert all((p != 0).any() for p in per_rank)
    assert (per_rank[0] & per_rank[1]).sum() == 0                          # every k-mer has one owner
    assert ((per_rank[0] | per_rank[1]) == single).all()


# ------------------------------------------------------------------ 6. lifecycle
def test_before_any_count_is_a_state_error(dev):
    from dsk_amd import KmerCounter
    from dsk_amd.engine import DskGpuError
    keys = torch.zeros(16, dtype=torch.int64, device=dev)
    out = torch.zeros(64, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with KmerCounter(kmer_size=31) as kc:
        for call in (lambda: kc.graph_adjacency(out.data_ptr()), kc.graph_adjacency,
                     lambda: kc.graph_neighbors(keys.data_ptr(), 16, out.data_ptr())):
            with pytest.raises(DskGpuError) as e:
                call()
            assert e.value.code == E_STATE
        kc.graph_neighbors(keys.data_ptr(), 0, out.data_ptr())              # nothing to do: not an error, even without a result


def test_null_pointers(oracle, golden_dir, dev):
    import ctypes as C
    from dsk_amd.engine import DskGpuError
    stream = stream_of("golden", oracle, golden_dir, dev)
    keys = torch.zeros(16, dtype=torch.int64, device=dev)
    out = torch.full((256,), 249, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with count(stream, dev, 31) as kc:
        assert kc._lib.dskgpu_graph_adjacency(kc._h, None, None) == E_ARG
        for call in (lambda: kc.graph_neighbors(0, 10, out.data_ptr()), lambda: kc.graph_neighbors(keys.data_ptr(), 10, 0)):
            with pytest.raises(DskGpuError) as e:
                call()
            assert e.value.code == E_ARG
        kc.graph_neighbors(keys.data_ptr(), 0, out.data_ptr())
        kc.graph_neighbors(0, 0, 0)
        assert (out.cpu().numpy() == 249).all()                             # n = 0 wrote nothing
        deg = (C.c_uint64 * 25)()
        assert kc._lib.dskgpu_graph_adjacency(kc._h, None, deg) == 0        # and the context still answers
        assert sum(deg) == kc.stats()["n_solid"] > 0


def test_a_result_without_rows(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir, dev)
    out = torch.full((256,), 249, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with count(stream, dev, 31, abundance_min=10 ** 6) as kc:
        assert kc.stats()["n_solid"] == 0
        deg = kc.graph_adjacency(out.data_ptr())
        assert deg.shape == (5, 5) and (deg == 0).all()
        assert (out.cpu().numpy() == 249).all()                             # nothing written
        adj, deg = kc.graph_adjacency_tensor()
        assert adj.numel() == 0 and (deg == 0).all()
        keys = np.arange(40, dtype=np.uint64).reshape(40, 1)
        assert (neighbors(kc, keys, dev) == 0).all()


def test_a_new_count_invalidates(oracle, golden_dir, dev):
    from dsk_amd import KmerCounter
    a = stream_of("golden", oracle, golden_dir, dev)
    b = stream_of("hand:31", oracle, golden_dir, dev)
    exp_a, solid_a = expected_rows(oracle, "golden", a, 31, 1)
    exp_b, solid_b = expected_rows(oracle, "hand:31", b, 31, 1)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    torch.cuda.synchronize()
    with KmerCounter(kmer_size=31, abundance_min=1) as kc:
        kc.set_reads_device(ta.data_ptr(), ta.numel())
        kc.count()
        got_a = check_rows_against_restatement(kc, 31, exp_a, len(solid_a))
        kc.set_reads_device(tb.data_ptr(), tb.numel())
        assert (kc.graph_adjacency_tensor()[0].cpu().numpy() == got_a).all()      # new reads alone change nothing: the result is still A's
        kc.count()
        check_rows_against_restatement(kc, 31, exp_b, len(solid_b))


@pytest.mark.parametrize("mkeys", [0, 2])
def test_the_graph_call_leaves_the_kept_encoding_alone(reads100k, dev, mkeys):
    """encode_reads() -> the 2-bit form is the only copy of the reads.  Count, adjacency, count again: identical rows, histogram and stats."""
    from dsk_amd import KmerCounter
    buf = reads100k.clone()
    torch.cuda.synchronize()
    with KmerCounter(kmer_size=31, abundance_min=1, max_pass_mkeys=mkeys) as kc:
        kc.set_reads_device(buf.data_ptr(), buf.numel())
        kc.encode_reads()
        buf.zero_(); torch.cuda.synchronize()                              # the bytes are gone
        kc.count()
        k1, a1 = kc.rows(); h1 = kc.histogram(); s1 = kc.stats()
        adj, deg = kc.graph_adjacency_tensor()
        assert int(deg.sum()) == s1["n_solid"] == adj.numel() and int((adj != 0).sum()) > adj.numel() // 2
        sub = torch.from_numpy(k1[:5000].view(np.int64)).to(dev)
        assert (kc.graph_neighbors_tensor(sub) == adj[:5000]).all()
        k1b, a1b = kc.rows()
        assert (k1b == k1).all() and (a1b == a1).all() and kc.stats() == s1    # the result and the stats are untouched
        kc.count()
        k2, a2 = kc.rows()
        assert (k2 == k1).all() and (a2 == a1).all() and (kc.histogram() == h1).all()
        s2 = kc.stats()
        assert (s2["n_kmers"], s2["n_distinct"], s2["n_solid"]) == (s1["n_kmers"], s1["n_distinct"], s1["n_solid"])
        assert (kc.graph_adjacency_tensor()[0] == adj).all()


def test_stage_times_name_the_graph(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir, dev)
    with count(stream, dev, 31, timing=True) as kc:
        before = dict(kc.stage_times())
        assert "graph" not in before and "query index" not in before
        kc.graph_adjacency_tensor()
        after = dict(kc.stage_times())
        assert after["graph"] > 0 and after["query index"] > 0
        assert all(after[n] == v for n, v in before.items())
