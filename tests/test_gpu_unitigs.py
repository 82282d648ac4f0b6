"""The rows' de Bruijn graph compacted into unitigs (include/dskgpu.h: dskgpu_unitigs / _rows / _table / _stream; csrc/unitigs.h).

All comparisons are exact.  The expectation is a restatement of the header's definition on STRINGS, independent of the device's bit
arithmetic: decode every row with kmer_to_string, slice, append and reverse-complement strings, look the result up in a dict value ->
row number built from the rows as the context returns them, follow the links one node at a time.  Test 3 needs no oracle and no
restatement: the unitig stream, counted again, must give back exactly the rows, each once.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
GOLDEN = "read50x_ref10K_e001.fasta.gz"
NONE = -1


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


def to_int(row):
    return sum(int(w) << (64 * i) for i, w in enumerate(row))


def row_values(kk):
    if kk.shape[1] == 1:
        return [int(v) for v in kk[:, 0]]
    return [to_int(r) for r in kk]


class Restatement:
    """The unitigs of `values` (the rows' values in row order, Python ints) with abundances `ab`, by the definition."""

    def __init__(self, values, ab, k):
        from dsk_amd.engine import kmer_to_string
        n = len(values)
        self.k, self.n = k, n
        S = [kmer_to_string(v, k) for v in values]
        R = [revcomp_str(s) for s in S]
        row_of = {v: r for r, v in enumerate(values)}
        assert len(row_of) == n
        pal = [S[r] == R[r] for r in range(n)]
        self.n_palindromes = sum(pal)

        def text(o):
            return R[o >> 1] if o & 1 else S[o >> 1]

        def node(s):
            """the oriented node that reads s, or NONE"""
            f, r = encode(s), encode(revcomp_str(s))
            row = row_of.get(min(f, r))
            return NONE if row is None else 2 * row + (0 if f <= r else 1)

        succ = []
        for o in range(2 * n):
            t = text(o)[1:]
            succ.append([p for p in (node(t + b) for b in "ACTG") if p != NONE])
        nxt = []
        for o in range(2 * n):
            p = succ[o][0] if len(succ[o]) == 1 else NONE
            if p != NONE and (len(succ[p ^ 1]) != 1 or (p >> 1) == (o >> 1) or pal[o >> 1] or pal[p >> 1]):
                p = NONE
            nxt.append(p)
        for o in range(2 * n):                                               # the links are symmetric
            if nxt[o] != NONE:
                assert nxt[nxt[o] ^ 1] == o ^ 1, o

        def prev(o):
            return NONE if nxt[o ^ 1] == NONE else nxt[o ^ 1] ^ 1

        seen = [False] * n
        unitigs = []                                                         # (path of oriented nodes, is a cycle)
        for r in range(n):
            if seen[r]:
                continue
            o = 2 * r
            while prev(o) != NONE and prev(o) != 2 * r:
                o = prev(o)
            if prev(o) == NONE:                                              # a chain (or a single node) with head o
                path = [o]
                while nxt[path[-1]] != NONE:
                    path.append(nxt[path[-1]])
                if (path[0] >> 1) > (path[-1] >> 1) or (len(path) == 1 and path[0] & 1):
                    path = [p ^ 1 for p in reversed(path)]
                cyc = False
            else:                                                            # a cycle: r is the smallest row on it (rows ascend here)
                path = [2 * r]
                while nxt[path[-1]] != 2 * r:
                    path.append(nxt[path[-1]])
                assert min(p >> 1 for p in path) == r
                cyc = True
            rows = [p >> 1 for p in path]
            assert len(set(rows)) == len(rows) and not any(seen[x] for x in rows)      # a path never holds a row twice
            for x in rows:
                seen[x] = True
            unitigs.append((path, cyc))
        unitigs.sort(key=lambda u: u[0][0] >> 1)
        self.paths = unitigs
        self.unitig = np.zeros(n, dtype=np.int64)
        self.pos_s = np.zeros(n, dtype=np.int64)
        self.offsets = np.zeros(len(unitigs) + 1, dtype=np.int64)
        self.ab_sum = np.zeros(len(unitigs), dtype=np.int64)
        self.kind = np.zeros(len(unitigs), dtype=np.uint8)
        pieces = []
        for u, (path, cyc) in enumerate(unitigs):
            for i, p in enumerate(path):
                self.unitig[p >> 1] = u
                self.pos_s[p >> 1] = (i << 1) | (p & 1)
            seq = text(path[0]) + "".join(text(p)[-1] for p in path[1:])
            assert len(seq) == k + len(path) - 1
            pieces.append(seq + "\n")
            self.offsets[u + 1] = self.offsets[u] + len(seq) + 1
            self.ab_sum[u] = sum(int(ab[p >> 1]) for p in path)
            self.kind[u] = 1 if cyc else 0
        self.stream = np.frombuffer("".join(pieces).encode(), dtype=np.uint8)
        lens = [len(p) for p, _ in unitigs]
        self.stats = dict(n_unitigs=len(unitigs), n_cycles=int(self.kind.sum()), n_single=sum(1 for x in lens if x == 1),
                          max_nodes=max(lens) if lens else 0, stream_bytes=n + len(unitigs) * k)
        assert self.stats["stream_bytes"] == len(self.stream) == int(self.offsets[-1])


# ------------------------------------------------------------------ streams (computed once, shared, never changed)
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


def circles_stream(k):
    rng = np.random.default_rng(7 + k)

    def rnd(n):
        return "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    chain, c1, c2 = rnd(20000 + k - 1), rnd(4096), rnd(4097)
    return np.frombuffer("\n".join([chain, c1 + c1[:k], c2 + c2[:k - 1], ""]).encode(), dtype=np.uint8).copy()


_streams, _restated = {}, {}


def stream_of(name, oracle, golden_dir):
    if name not in _streams:
        if name == "golden":
            _streams[name] = np.ascontiguousarray(oracle.load_bank(os.path.join(golden_dir, GOLDEN))[0])
        elif name.startswith("hand:"):
            _streams[name] = handmade_stream(int(name.split(":")[1]))
        else:
            _streams[name] = circles_stream(int(name.split(":")[1]))
    return _streams[name]


def count(stream, dev, k, **kw):
    from dsk_amd import KmerCounter
    kc = KmerCounter(kmer_size=k, **kw)
    t = torch.from_numpy(stream).to(dev)
    torch.cuda.synchronize()
    kc.set_reads_device(t.data_ptr(), t.numel())
    kc.count()
    kc._reads_keepalive = t
    return kc


def restated(kc, name, k, amin, order):
    """the restatement of the rows of kc, cached per (input, k, abundance_min, row order)"""
    key = (name, k, amin, order)
    if key not in _restated:
        kk, ab = kc.rows()
        _restated[key] = Restatement(row_values(kk), ab, k)
    return _restated[key]


def device_answer(kc):
    st = kc.unitigs()
    unitig, pos = kc.unitigs_rows_tensor()
    off, ab_sum, kind = kc.unitigs_table_tensor()
    stream = kc.unitigs_stream_tensor()
    return st, unitig.cpu().numpy(), pos.cpu().numpy(), off.cpu().numpy(), ab_sum.cpu().numpy(), kind.cpu().numpy(), stream.cpu().numpy()


def check_against_restatement(kc, exp):
    st, unitig, pos, off, ab_sum, kind, stream = device_answer(kc)
    print("unitig stats", st, "expected", exp.stats)
    assert len(unitig) == len(pos) == exp.n
    bad = np.nonzero((unitig != exp.unitig) | (pos != exp.pos_s))[0]
    assert len(bad) == 0, (len(bad), bad[:5], unitig[bad[:5]], exp.unitig[bad[:5]], pos[bad[:5]], exp.pos_s[bad[:5]])
    assert off.dtype == np.int64 and (off == exp.offsets).all()
    assert (ab_sum == exp.ab_sum).all()
    assert kind.dtype == np.uint8 and (kind == exp.kind).all()
    assert stream.dtype == np.uint8 and len(stream) == len(exp.stream) and (stream == exp.stream).all()
    assert {n: st[n] for n in exp.stats} == exp.stats
    assert 1 <= st["n_rounds"] <= 3 * 33
    return st


# rows, unitigs, longest, single, cycles, palindromes: fixed on the CPU, whatever the row order
PINNED = {
    ("golden", 15): (13000, 719, 278, 37, 0, 0), ("golden", 31): (13096, 442, 303, 21, 0, 0), ("golden", 63): (10945, 125, 935, 5, 0, 0),
    ("golden", 96): (2525, 600, 19, 105, 0, 0),
    ("hand", 1): (2, 2, 1, 2, 0, 0), ("hand", 2): (10, 10, 1, 10, 0, 4), ("hand", 15): (292, 6, 286, 4, 1, 0), ("hand", 16): (313, 10, 285, 6, 1, 3),
    ("hand", 31): (276, 6, 270, 4, 1, 0), ("hand", 32): (297, 10, 269, 6, 1, 3), ("hand", 33): (274, 6, 268, 4, 1, 0),
    ("hand", 64): (263, 11, 237, 6, 1, 3), ("hand", 65): (242, 6, 236, 4, 1, 0), ("hand", 128): (201, 10, 173, 6, 1, 3),
}


def check_pinned(kind, k, exp):
    if (kind, k) in PINNED:
        s = exp.stats
        assert (exp.n, s["n_unitigs"], s["max_nodes"], s["n_single"], s["n_cycles"], exp.n_palindromes) == PINNED[(kind, k)], (kind, k)


# ------------------------------------------------------------------ 1. the string restatement, every key width and boundary
@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k", [15, 16, 31, 32, 33, 63, 64, 65, 96])
def test_golden_reads_match_the_string_restatement(oracle, golden_dir, dev, k, partition_order):
    """Fails before the feature: KmerCounter has no unitigs()."""
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, k, abundance_min=2, partition_order=partition_order) as kc:
        exp = restated(kc, "golden", k, 2, partition_order)
        check_pinned("golden", k, exp)
        st = check_against_restatement(kc, exp)
        assert st["n_unitigs"] > 100 and st["max_nodes"] > 10


@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k", [1, 2, 15, 16, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128])
def test_handmade_stream(oracle, golden_dir, dev, k, partition_order):
    """the AC repeat is the one cycle; poly-A and poly-C (self-loops), the AT repeat at odd k (hairpin) and the palindromes are single nodes"""
    stream = stream_of("hand:%d" % k, oracle, golden_dir)
    with count(stream, dev, k, abundance_min=1, partition_order=partition_order) as kc:
        exp = restated(kc, "hand:%d" % k, k, 1, partition_order)
        check_pinned("hand", k, exp)
        check_against_restatement(kc, exp)
        kk, _ = kc.rows()
        row_of = {v: r for r, v in enumerate(row_values(kk))}
        if k >= 15:
            assert exp.stats["n_cycles"] == 1
            ac = ("AC" * k)[:k]
            r = row_of[min(encode(ac), encode(revcomp_str(ac)))]
            assert exp.kind[exp.unitig[r]] == 1
            singles = ["A" * k, "C" * k] + ([("AT" * k)[:k]] if k % 2 else [])
            for s in singles:
                u = exp.unitig[row_of[min(encode(s), encode(revcomp_str(s)))]]
                assert exp.offsets[u + 1] - exp.offsets[u] == k + 1, s


# ------------------------------------------------------------------ 2. a long chain and two circles: many rounds, cycle lengths 2^12 and 2^12 + 1
@pytest.mark.parametrize("k", [31, 64, 97])
def test_long_chain_and_two_circles(oracle, golden_dir, dev, k):
    name = "circles:%d" % k
    stream = stream_of(name, oracle, golden_dir)
    with count(stream, dev, k, abundance_min=1) as kc:
        st, unitig, pos, off, ab_sum, kind, text = device_answer(kc)
        print("unitig stats", st)
        assert len(unitig) == 28193
        assert st["n_unitigs"] == 3 and st["n_cycles"] == 2 and st["n_single"] == 0 and st["max_nodes"] == 20000
        nodes = np.diff(off) - k
        assert sorted(nodes.tolist()) == [4096, 4097, 20000]
        assert sorted(kind[nodes != 20000].tolist()) == [1, 1] and kind[nodes == 20000].tolist() == [0]
        assert 6 <= st["n_rounds"] <= 3 * 33                                 # three phases, each with a last round that finds nothing new
        for u in range(3):
            first = np.nonzero((unitig == u) & ((pos >> 1) == 0))[0]
            assert len(first) == 1
            if kind[u] == 1:                                                 # a cycle starts at its smallest row number, forward
                assert first[0] == np.nonzero(unitig == u)[0].min() and pos[first[0]] == 0
        check_against_restatement(kc, restated(kc, name, k, 1, False))


# ------------------------------------------------------------------ 3. recount, no oracle, medium size
@pytest.fixture(scope="module")
def reads100k(dev):
    from dsk_amd import synth
    return synth.make_reads(synth.make_genome(300_000, dev), 100_000, 150)


_chain_sets = {}


def sorted_rows(kk):
    return np.sort(kk[:, 0])


@pytest.mark.parametrize("kind,kw", [
    ("global", dict()),
    ("partition_order", dict(partition_order=True)),
    ("multi_pass", dict(max_pass_mkeys=2)),
    ("no_sort", dict(sort=False)),
    ("two_banks_min", dict(solidity_kind="min")),
])
def test_the_stream_counts_back_to_the_rows(reads100k, dev, kind, kw):
    from dsk_amd import KmerCounter
    k = 31
    with KmerCounter(kmer_size=k, abundance_min=2, **kw) as kc:
        kc.set_reads_device(reads100k.data_ptr(), reads100k.numel())
        if kind == "two_banks_min":
            kc.set_banks([reads100k.numel() // 2 // 151 * 151, reads100k.numel()])
        kc.count()
        if kind == "multi_pass":
            assert kc.stats()["n_passes"] > 1, kc.stats()
        kk, ab = kc.rows()
        n = len(kk)
        assert n == kc.stats()["n_solid"] > 100_000
        st = kc.unitigs()
        print("unitig stats", kind, st)
        text = kc.unitigs_stream_tensor()
        unitig, pos = (t.cpu().numpy().astype(np.int64) for t in kc.unitigs_rows_tensor())
        off, ab_sum, kinds = (t.cpu().numpy() for t in kc.unitigs_table_tensor())
        nu = st["n_unitigs"]
        assert int(off[-1]) == st["stream_bytes"] == text.numel() == n + nu * k and off[0] == 0 and len(off) == nu + 1
        nodes = np.diff(off) - k
        assert (nodes >= 1).all() and int(nodes.max()) == st["max_nodes"] and int((nodes == 1).sum()) == st["n_single"]
        assert int(kinds.sum()) == st["n_cycles"]
        assert unitig.min() >= 0 and unitig.max() == nu - 1
        assert len(np.unique(unitig * (2 ** 32) + (pos >> 1))) == n          # every (unitig, position) once ...
        assert ((pos >> 1) < nodes[unitig]).all()                            # ... and inside its unitig
        assert int(ab_sum.sum()) == int(ab.astype(np.int64).sum())
        with KmerCounter(kmer_size=k, abundance_min=1) as again:
            again.set_reads_device(text.data_ptr(), text.numel())
            again.count()
            k2, a2 = again.rows()
            assert again.stats()["n_kmers"] == n
            assert (a2 == 1).all()
            assert len(k2) == n and (sorted_rows(k2) == sorted_rows(kk)).all()
        if kind in ("global", "partition_order"):
            lines = bytes(text.cpu().numpy()).decode().split("\n")
            assert lines[-1] == "" and len(lines) == nu + 1
            _chain_sets[kind] = {min(s, revcomp_str(s)) for s, c in zip(lines, kinds) if c == 0}
            if len(_chain_sets) == 2:                                        # the row order changes numbering and orientation, not the unitigs
                assert _chain_sets["global"] == _chain_sets["partition_order"]


# ------------------------------------------------------------------ 4. lifecycle and errors
def code_of(call):
    from dsk_amd.engine import DskGpuError
    with pytest.raises(DskGpuError) as e:
        call()
    return e.value.code


def test_before_any_count_is_a_state_error(dev):
    from dsk_amd import KmerCounter
    buf = torch.zeros(1024, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p = buf.data_ptr()
    with KmerCounter(kmer_size=31) as kc:
        for call in (kc.unitigs, lambda: kc.unitigs_rows(p, 0), lambda: kc.unitigs_table(p, 0, 0), lambda: kc.unitigs_stream(p, 1024)):
            assert code_of(call) == E_STATE


def test_null_pointers_and_a_small_capacity(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31) as kc:
        st = kc.unitigs()
        nb = st["stream_bytes"]
        assert kc._lib.dskgpu_unitigs(kc._h, None) == 0                      # stats may be NULL
        assert kc._lib.dskgpu_unitigs_rows(kc._h, None, None) == E_ARG
        assert kc._lib.dskgpu_unitigs_table(kc._h, None, None, None) == E_ARG
        assert kc._lib.dskgpu_unitigs_stream(kc._h, None, nb) == E_ARG
        out = torch.full((nb + 64,), 249, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        for cap in (0, nb - 1):
            assert code_of(lambda: kc.unitigs_stream(out.data_ptr(), cap)) == E_ARG
        assert (out.cpu().numpy() == 249).all()                             # nothing written
        assert kc.unitigs() == st                                           # and the context still answers
        # each output alone
        n = kc.stats()["n_solid"]
        u1 = torch.full((n + 8,), -7, dtype=torch.int32, device=dev)
        p1 = torch.full((n + 8,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        kc.unitigs_rows(u1.data_ptr(), 0)
        kc.unitigs_rows(0, p1.data_ptr())
        u2, p2 = kc.unitigs_rows_tensor()
        assert (u1[:n] == u2).all() and (p1[:n] == p2).all() and (u1[n:] == -7).all() and (p1[n:] == -7).all()


def test_writes_stay_inside_their_arrays(oracle, golden_dir, dev):
    stream = stream_of("hand:33", oracle, golden_dir)
    with count(stream, dev, 33, abundance_min=1) as kc:
        exp = restated(kc, "hand:33", 33, 1, False)
        nu, nb = exp.stats["n_unitigs"], exp.stats["stream_bytes"]
        for off in (0, 3):
            out = torch.full((off + nb + 64,), 249, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            kc.unitigs_stream(out.data_ptr() + off, nb + 5)                 # a larger capacity writes no more
            res = out.cpu().numpy()
            assert (res[:off] == 249).all() and (res[off + nb:] == 249).all(), "unitigs_stream wrote outside its stream_bytes"
            assert (res[off: off + nb] == exp.stream).all()
        o = torch.full((nu + 1 + 8,), -7, dtype=torch.int64, device=dev)
        a = torch.full((nu + 8,), -7, dtype=torch.int64, device=dev)
        c = torch.full((nu + 64,), 249, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        kc.unitigs_table(o.data_ptr(), a.data_ptr(), c.data_ptr())
        assert (o[nu + 1:] == -7).all() and (a[nu:] == -7).all() and (c[nu:] == 249).all()
        assert (o[: nu + 1].cpu().numpy() == exp.offsets).all() and (a[:nu].cpu().numpy() == exp.ab_sum).all() and (c[:nu].cpu().numpy() == exp.kind).all()
        a2 = torch.full((nu + 8,), -7, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        kc.unitigs_table(0, a2.data_ptr(), 0)                               # one output alone
        assert (a2 == a).all()


def test_a_result_without_rows(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31, abundance_min=10 ** 6) as kc:
        assert kc.stats()["n_solid"] == 0
        st = kc.unitigs()
        assert all(v == 0 for v in st.values()), st
        o = torch.full((8,), -7, dtype=torch.int64, device=dev)
        a = torch.full((8,), -7, dtype=torch.int64, device=dev)
        c = torch.full((8,), 249, dtype=torch.uint8, device=dev)
        u = torch.full((8,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        kc.unitigs_table(o.data_ptr(), a.data_ptr(), c.data_ptr())
        kc.unitigs_rows(u.data_ptr(), u.data_ptr())
        kc.unitigs_stream(c.data_ptr(), 8)
        assert o[0] == 0 and (o[1:] == -7).all() and (a == -7).all() and (c == 249).all() and (u == -7).all()
        off, ab_sum, kind = kc.unitigs_table_tensor()
        assert off.tolist() == [0] and ab_sum.numel() == 0 and kind.numel() == 0
        assert kc.unitigs_stream_tensor().numel() == 0 and kc.unitigs_rows_tensor()[0].numel() == 0


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
        assert kc.unitigs() == st_b                                          # new reads alone change nothing: the result is still B's
        kc.count()
        st_a = kc.unitigs()
        n = kc.stats()["n_solid"]
        assert n == 99957 and st_a["stream_bytes"] == n + 31 * st_a["n_unitigs"] and st_a != st_b
        kc.set_reads_device(tb.data_ptr(), tb.numel())
        kc.count()
        check_against_restatement(kc, exp_b)


@pytest.mark.parametrize("mkeys", [0, 2])
def test_the_unitig_calls_leave_the_kept_encoding_alone(reads100k, dev, mkeys):
    """encode_reads() -> the 2-bit form is the only copy of the reads.  Count, unitigs, count again: identical rows, histogram and stats."""
    from dsk_amd import KmerCounter
    buf = reads100k.clone()
    torch.cuda.synchronize()
    with KmerCounter(kmer_size=31, abundance_min=2, max_pass_mkeys=mkeys) as kc:
        kc.set_reads_device(buf.data_ptr(), buf.numel())
        kc.encode_reads()
        buf.zero_(); torch.cuda.synchronize()                              # the bytes are gone
        kc.count()
        k1, a1 = kc.rows(); h1 = kc.histogram(); s1 = kc.stats()
        u1 = kc.unitigs()
        text1 = kc.unitigs_stream_tensor()
        assert u1["stream_bytes"] == text1.numel() == len(k1) + 31 * u1["n_unitigs"]
        k1b, a1b = kc.rows()
        assert (k1b == k1).all() and (a1b == a1).all() and kc.stats() == s1    # the result and the stats are untouched
        kc.count()
        k2, a2 = kc.rows()
        assert (k2 == k1).all() and (a2 == a1).all() and (kc.histogram() == h1).all()
        s2 = kc.stats()
        assert (s2["n_kmers"], s2["n_distinct"], s2["n_solid"]) == (s1["n_kmers"], s1["n_distinct"], s1["n_solid"])
        assert kc.unitigs() == u1 and (kc.unitigs_stream_tensor() == text1).all()


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
        for call in (kc.unitigs, lambda: kc.unitigs_rows(p, 0), lambda: kc.unitigs_table(p, 0, 0), lambda: kc.unitigs_stream(p, 1024)):
            assert code_of(call) == E_STATE
        assert "world_size" in kc._lib.dskgpu_last_error(kc._h).decode()
        assert int(kc.graph_adjacency().sum()) == kc.stats()["n_solid"]      # the rank's context still answers what it can


def test_stage_times_name_the_unitigs(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31, timing=True) as kc:
        before = dict(kc.stage_times())
        assert not any(n in before for n in ("unitigs", "unitig stream", "graph", "query index"))
        kc.unitigs_stream_tensor()
        after = dict(kc.stage_times())
        assert after["unitigs"] > 0 and after["unitig stream"] > 0 and after["graph"] > 0 and after["query index"] > 0
        assert all(after[n] == v for n, v in before.items())
