"""Lookups in the last result (include/dskgpu.h: dskgpu_query_prepare / _kmers / _reads; csrc/query.h).

All comparisons are exact.  The expected answer of a read query comes from the CPU oracle alone: its window enumeration of the QUERIED
stream looked up, with numpy, in the oracle's solid rows of the COUNTED stream.  The self-consistency tests need no oracle: the rows a
context hands out are the questions, their abundances the answers.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E_STATE = -4
KS = [1, 15, 31, 32, 33, 63, 64, 65, 96, 127, 128]
WINDOWS = [(1, 2147483647), (2, 2147483647), (2, 5)]          # (abundance_min, abundance_max)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


def synth_reads(dev, name="tiny", seed=None, n_reads=None):
    from dsk_amd import synth
    gl, nr, rl = synth.workload(name)
    if seed is None:
        return synth.make_reads(synth.make_genome(gl, dev), n_reads or nr, rl).cpu().numpy()
    return synth.make_reads(synth.make_genome(gl, dev, seed=seed), n_reads or nr, rl, seed=seed + 1).cpu().numpy()


def messy_stream(reads):
    """N, IUPAC codes, lower case, blank lines, reads of 1 .. 40 bases, a read cut in the middle: built from the first counted reads"""
    rng = np.random.default_rng(17)
    s = np.array(reads[: 151 * 400], dtype=np.uint8)
    for code in b"NRYKMSWnry-":
        s[rng.integers(0, len(s), 25)] = code
    low = rng.integers(0, len(s), 3000)
    s[low] = np.where((s[low] >= 65) & (s[low] <= 90), s[low] + 32, s[low])          # acgt are bases too
    short = []
    for n in (1, 2, 14, 15, 16, 30, 31, 32, 33, 40):
        short += [reads[151 * 500: 151 * 500 + n], np.array([10], np.uint8)]
    tail = reads[151 * 600: 151 * 600 + 97]                                           # ends without a newline, inside a read
    return np.concatenate([np.array([10, 10], np.uint8), s, np.array([10, 10, 10], np.uint8)] + short + [tail]).astype(np.uint8)


@pytest.fixture(scope="module")
def streams(dev, golden_dir, oracle):
    counted = {"tiny": synth_reads(dev)}
    for name in ("readN.fasta", "shortread.fasta"):
        counted[name] = np.ascontiguousarray(oracle.load_bank(os.path.join(golden_dir, name))[0])
    queried = {"absent": synth_reads(dev, seed=4242, n_reads=1500), "messy": messy_stream(counted["tiny"])}
    return counted, queried


def lookup(rows_w, rows_ab, q_w):
    """abundance of every row of q_w (n x W words) among the distinct rows rows_w (m x W), 0 where it is none -- numpy only"""
    m = len(rows_ab)
    out = np.zeros(len(q_w), np.uint32)
    if m == 0 or len(q_w) == 0:
        return out
    if rows_w.shape[1] == 1:
        order = np.argsort(rows_w[:, 0], kind="stable")
        rk, ra = rows_w[order, 0], rows_ab[order]
        at = np.minimum(np.searchsorted(rk, q_w[:, 0]), m - 1)
        hit = rk[at] == q_w[:, 0]
        out[hit] = ra[at[hit]]
        return out
    # several words: number the distinct rows of (rows, questions) word by word, then look the numbers up
    both = np.concatenate([rows_w, q_w])
    ids = np.unique(both[:, 0], return_inverse=True)[1].reshape(-1).astype(np.uint64)
    for c in range(1, both.shape[1]):
        r = np.unique(both[:, c], return_inverse=True)[1].reshape(-1).astype(np.uint64)
        ids = np.unique(ids * np.uint64(len(both) + 1) + r, return_inverse=True)[1].reshape(-1).astype(np.uint64)
    return lookup(ids[:m].reshape(-1, 1), rows_ab, ids[m:].reshape(-1, 1))


_refs, _expected = {}, {}


def ref_of(oracle, name, stream, k):
    if (name, k) not in _refs:
        _refs[(name, k)] = oracle.count(stream, k)
    return _refs[(name, k)]


def expected_reads(oracle, ref, stream, k, amin, amax):
    words, valid = oracle.enumerate_words(stream, k)
    keep = (ref.ab >= amin) & (ref.ab <= amax)
    nw = (k + 31) // 32
    exp = lookup(ref.words()[keep], ref.ab[keep], np.ascontiguousarray(words[:, :nw]))
    exp[valid == 0] = 0
    return exp


def query_reads(kc, stream, dev, in_off=0, out_off=0):
    """query a numpy stream; in_off / out_off: byte / element offsets of the device pointers from their allocations (alignment)"""
    buf = torch.zeros(in_off + len(stream) + 64, dtype=torch.uint8, device=dev)
    buf[in_off: in_off + len(stream)] = torch.from_numpy(np.ascontiguousarray(stream)).to(dev)
    out = torch.full((out_off + len(stream) + 64,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    kc.query_reads(buf.data_ptr() + in_off, len(stream), out.data_ptr() + 4 * out_off)
    res = out.cpu().numpy()
    assert (res[:out_off] == -7).all() and (res[out_off + len(stream):] == -7).all(), "the query wrote outside its output"
    return res[out_off: out_off + len(stream)].view(np.uint32)


def query_kmers(kc, kmers, dev):
    t = torch.from_numpy(np.ascontiguousarray(kmers).view(np.int64)).to(dev)
    return kc.query_kmers_tensor(t).cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------ 1. oracle parity of query_reads
@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k", KS)
def test_query_reads_matches_the_oracle(oracle, streams, dev, k, partition_order):
    """Fails before the feature: KmerCounter has no query_reads."""
    from dsk_amd import KmerCounter
    counted, queried = streams
    for cname, cs in counted.items():
        ref = ref_of(oracle, cname, cs, k)
        t = torch.from_numpy(cs).to(dev)
        for amin, amax in WINDOWS:
            with KmerCounter(kmer_size=k, abundance_min=amin, abundance_max=amax, partition_order=partition_order) as kc:
                kc.set_reads_device(t.data_ptr(), t.numel())
                kc.count()
                n_solid = kc.stats()["n_solid"]
                assert n_solid == int(((ref.ab >= amin) & (ref.ab <= amax)).sum())
                cases = [("itself", cs, 0, 0), ("absent", queried["absent"], 0, 0), ("messy", queried["messy"], 3, 1)]
                for qname, qs, in_off, out_off in cases:
                    got = query_reads(kc, qs, dev, in_off, out_off)
                    key = (cname, qname, k, amin, amax)                  # (the same for both row orders)
                    if key not in _expected:
                        _expected[key] = expected_reads(oracle, ref, qs, k, amin, amax)
                    exp = _expected[key]
                    bad = np.nonzero(got != exp)[0]
                    assert len(bad) == 0, (cname, qname, k, amin, amax, partition_order, len(bad), bad[:5], got[bad[:5]], exp[bad[:5]])
                    if qname == "itself" and amin == 1 and amax == 2147483647:
                        assert int((got != 0).sum()) == ref.total        # every valid window of the counted reads is a row


# ------------------------------------------------------------------ 2. self-consistency on every kind of result
def revcomp(v, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | ((v & 3) ^ 2)
        v >>= 2
    return r


def to_int(row):
    return sum(int(w) << (64 * i) for i, w in enumerate(row))


def to_words(v, nw):
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(nw)]


def check_self_consistency(kc, dev, k):
    kk, ab = kc.rows()
    st = kc.stats()
    assert len(ab) == st["n_solid"] and len(ab) > 0 and (ab > 0).all()
    got = query_kmers(kc, kk, dev)
    assert (got == ab).all(), (k, int((got != ab).sum()))
    kc.query_prepare()                                                    # the index is there: a no-op, same answers
    assert (query_kmers(kc, kk, dev) == ab).all()
    # one bit flipped (bit 2 * (row % k) + row % 2 of the value: every base position, both bits)
    nw = kk.shape[1]
    flipped = kk.copy()
    idx = np.arange(len(kk))
    bit = (2 * (idx % k) + idx % 2).astype(np.uint64)
    flipped[idx, (bit // np.uint64(64)).astype(np.int64)] ^= np.uint64(1) << (bit % np.uint64(64))
    is_row = lookup(kk, np.ones(len(kk), np.uint32), flipped) != 0
    got = query_kmers(kc, flipped, dev)
    assert (got[~is_row] == 0).all(), (k, int((got[~is_row] != 0).sum()))
    assert (got[is_row] == lookup(kk, ab, flipped)[is_row]).all()
    assert (~is_row).sum() > len(kk) // 2
    # the reverse complement of a non-palindromic row is not canonical: not found
    take = np.linspace(0, len(kk) - 1, min(len(kk), 1500)).astype(np.int64)
    rc = [revcomp(to_int(kk[i]), k) for i in take]
    keep = [j for j, i in enumerate(take) if rc[j] != to_int(kk[i])]
    rcw = np.array([to_words(rc[j], nw) for j in keep], dtype=np.uint64).reshape(len(keep), nw)
    assert len(keep) > 0 and (query_kmers(kc, rcw, dev) == 0).all(), k
    return kk, ab


@pytest.fixture(scope="module")
def reads100k(dev):
    from dsk_amd import synth
    return synth.make_reads(synth.make_genome(300_000, dev), 100_000, 150)


@pytest.mark.parametrize("kind,k,kw", [
    ("global", 31, dict(abundance_min=2)),
    ("partition_order", 31, dict(abundance_min=2, partition_order=True)),
    ("partition_order", 63, dict(abundance_min=2, partition_order=True)),
    ("multi_pass", 31, dict(abundance_min=1, max_pass_mkeys=2)),
    ("multi_pass", 63, dict(abundance_min=1, max_pass_mkeys=2)),
    ("multi_pass_partition_order", 31, dict(abundance_min=1, max_pass_mkeys=2, partition_order=True)),
    ("no_sort", 31, dict(abundance_min=2, sort=False)),
    ("no_sort", 63, dict(abundance_min=2, sort=False)),
    ("three_abi_words", 96, dict(abundance_min=2)),
    ("three_abi_words_partition_order", 96, dict(abundance_min=1, partition_order=True)),
    ("four_words", 128, dict(abundance_min=2)),
])
def test_rows_answer_for_themselves(reads100k, dev, kind, k, kw):
    from dsk_amd import KmerCounter
    with KmerCounter(kmer_size=k, **kw) as kc:
        kc.set_reads_device(reads100k.data_ptr(), reads100k.numel())
        kc.count()
        if kind.startswith("multi_pass"):
            assert kc.stats()["n_passes"] > 1, kc.stats()
        check_self_consistency(kc, dev, k)


@pytest.mark.parametrize("k", [31, 70])
def test_rows_of_a_per_bank_count_answer_for_themselves(reads100k, dev, k):
    """two banks, solidity kind min: a query returns what the row's abundance column holds"""
    from dsk_amd import KmerCounter
    with KmerCounter(kmer_size=k, abundance_min=1, solidity_kind="min") as kc:
        kc.set_reads_device(reads100k.data_ptr(), reads100k.numel())
        kc.set_banks([reads100k.numel() // 2 // 151 * 151, reads100k.numel()])
        kc.count()
        check_self_consistency(kc, dev, k)


# ------------------------------------------------------------------ 3. lifecycle
def test_query_before_any_count_is_a_state_error(dev):
    from dsk_amd import KmerCounter
    from dsk_amd.engine import DskGpuError
    buf = torch.zeros(1024, dtype=torch.uint8, device=dev)
    out = torch.zeros(1024, dtype=torch.int32, device=dev)
    keys = torch.zeros(16, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with KmerCounter(kmer_size=31) as kc:
        for call in (kc.query_prepare, lambda: kc.query_reads(buf.data_ptr(), 1024, out.data_ptr()),
                     lambda: kc.query_kmers(keys.data_ptr(), 16, out.data_ptr())):
            with pytest.raises(DskGpuError) as e:
                call()
            assert e.value.code == E_STATE
        kc.query_reads(buf.data_ptr(), 0, out.data_ptr())                 # nothing to do: not an error, even without a result
        kc.query_kmers(keys.data_ptr(), 0, out.data_ptr())


def test_null_pointers_and_empty_calls(streams, dev):
    from dsk_amd import KmerCounter
    from dsk_amd.engine import DskGpuError
    cs = streams[0]["tiny"]
    t = torch.from_numpy(cs).to(dev)
    out = torch.full((256,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with KmerCounter(kmer_size=31) as kc:
        kc.set_reads_device(t.data_ptr(), t.numel())
        kc.count()
        for call in (lambda: kc.query_reads(0, 100, out.data_ptr()), lambda: kc.query_reads(t.data_ptr(), 100, 0),
                     lambda: kc.query_kmers(0, 10, out.data_ptr()), lambda: kc.query_kmers(t.data_ptr(), 10, 0)):
            with pytest.raises(DskGpuError) as e:
                call()
            assert e.value.code == -1
        kc.query_reads(t.data_ptr(), 0, out.data_ptr())
        kc.query_kmers(t.data_ptr(), 0, out.data_ptr())
        assert (out.cpu().numpy() == -7).all()                            # n = 0 wrote nothing
        assert (query_reads(kc, cs[:151 * 20], dev) != 0).any()           # and the context still answers


def test_a_new_count_invalidates_the_index(oracle, streams, dev):
    from dsk_amd import KmerCounter
    a = streams[0]["tiny"]
    b = synth_reads(dev, seed=777, n_reads=4000)
    ref_a, ref_b = oracle.count(a, 31), oracle.count(b, 31)
    probe = np.concatenate([a[: 151 * 300], b[: 151 * 300]])
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    with KmerCounter(kmer_size=31, abundance_min=1) as kc:
        kc.set_reads_device(ta.data_ptr(), ta.numel())
        kc.count()
        got_a = query_reads(kc, probe, dev)
        kc.set_reads_device(tb.data_ptr(), tb.numel())
        assert (query_reads(kc, probe, dev) == got_a).all()               # new reads alone change nothing: the result is still A's
        kc.count()
        got_b = query_reads(kc, probe, dev)
    exp_a, exp_b = expected_reads(oracle, ref_a, probe, 31, 1, 2147483647), expected_reads(oracle, ref_b, probe, 31, 1, 2147483647)
    assert (exp_a != exp_b).any()
    assert (got_a == exp_a).all() and (got_b == exp_b).all()


@pytest.mark.parametrize("mkeys", [0, 2])
def test_a_query_leaves_the_kept_encoding_alone(oracle, dev, mkeys):
    """encode_reads() -> the 2-bit form is the only copy of the reads.  Count, query ANOTHER stream, count again: identical rows and
    histogram (a query that encoded into the context's own buffers would make the second count see the other stream)."""
    from dsk_amd import KmerCounter, synth
    reads = synth.make_reads(synth.make_genome(300_000, dev), 100_000, 150)
    other = synth.make_reads(synth.make_genome(300_000, dev, seed=99), 120_000, 150, seed=100)
    ref = oracle.count(reads.cpu().numpy(), 31)
    buf = reads.clone()
    torch.cuda.synchronize()
    with KmerCounter(kmer_size=31, abundance_min=1, max_pass_mkeys=mkeys) as kc:
        kc.set_reads_device(buf.data_ptr(), buf.numel())
        kc.encode_reads()
        buf.zero_(); torch.cuda.synchronize()                              # the bytes are gone
        kc.count()
        k1, a1 = kc.rows(); h1 = kc.histogram(); s1 = kc.stats()
        assert (k1[:, 0] == ref.lo).all() and (a1 == ref.ab).all()
        got = kc.query_reads_tensor(other).cpu().numpy().view(np.uint32)
        assert (got == expected_reads(oracle, ref, other.cpu().numpy(), 31, 1, 2147483647)).all()
        assert (kc.rows()[0] == k1).all() and kc.stats() == s1            # the result and the stats are untouched
        kc.count()
        k2, a2 = kc.rows()
        assert (k2 == k1).all() and (a2 == a1).all() and (kc.histogram() == h1).all()
        s2 = kc.stats()
        assert (s2["n_kmers"], s2["n_distinct"], s2["n_solid"]) == (s1["n_kmers"], s1["n_distinct"], s1["n_solid"])


def test_a_result_without_rows_answers_zero(streams, dev):
    from dsk_amd import KmerCounter
    cs = streams[0]["tiny"]
    t = torch.from_numpy(cs).to(dev)
    for k, kw in ((31, dict(abundance_min=1000000)), (127, dict(abundance_min=1, partition_order=True))):
        with KmerCounter(kmer_size=k, **kw) as kc:
            if k == 31:
                kc.set_reads_device(t.data_ptr(), t.numel())
            else:
                kc.set_reads_device(t.data_ptr(), 100)                      # one read fragment shorter than k: no window at all
            kc.count()
            assert kc.stats()["n_solid"] == 0
            kc.query_prepare()
            assert (query_reads(kc, cs[: 151 * 50], dev, 1, 3) == 0).all()
            keys = np.arange(40 * kc.words, dtype=np.uint64).reshape(40, kc.words)
            assert (query_kmers(kc, keys, dev) == 0).all()


def test_stage_times_name_the_query(streams, dev):
    from dsk_amd import KmerCounter
    cs = streams[0]["tiny"]
    t = torch.from_numpy(cs).to(dev)
    with KmerCounter(kmer_size=31, timing=True) as kc:
        kc.set_reads_device(t.data_ptr(), t.numel())
        kc.count()
        before = dict(kc.stage_times())
        assert "query" not in before and "query index" not in before
        query_reads(kc, cs, dev)
        after = dict(kc.stage_times())
        assert after["query"] > 0 and after["query index"] > 0
        assert all(after[n] == v for n, v in before.items())


# ------------------------------------------------------------------ 4. two ranks on one device
@pytest.mark.parametrize("k", [31, 63, 15])
def test_group_answer_is_the_sum_over_the_ranks(oracle, golden_dir, dev, k):
    from dsk_amd import KmerCounter, KmerGroup
    s, _ = oracle.load_bank(os.path.join(golden_dir, "read50x_ref10K_e001.fasta.gz"))
    s = np.ascontiguousarray(s)
    recs = bytes(s).split(b"\n")
    with KmerCounter(kmer_size=k, abundance_min=2) as kc:
        kc.push_reads(s)
        kc.count()
        single = query_reads(kc, s, dev).astype(np.int64)
    assert (single != 0).any()
    with KmerGroup([0, 0], kmer_size=k, abundance_min=2) as g:
        for r in range(2):
            g.rank(r).push_reads(b"\n".join(recs[r::2]) + b"\n")
        g.count()
        per_rank = [query_reads(g.rank(r), s, dev).astype(np.int64) for r in range(2)]
    assert all((p != 0).any() for p in per_rank)
    assert ((per_rank[0] != 0) & (per_rank[1] != 0)).sum() == 0            # every k-mer has one owner
    assert (per_rank[0] + per_rank[1] == single).all()


# ------------------------------------------------------------------ 5. full size, identities only
def positions_per_abundance(out, nbins):
    bins = torch.zeros(nbins, dtype=torch.int64, device=out.device)
    step = 1 << 28
    for i in range(0, out.numel(), step):
        a = out[i: i + step].to(torch.int64)
        assert int(a.min()) >= 0
        bins += torch.bincount(torch.clamp(a, max=nbins - 1), minlength=nbins)
    return bins.cpu().numpy()


@pytest.mark.parametrize("partition_order", [False, True])
def test_full_size_identities(dev, partition_order):
    """c2_10Mx150, k = 31, the counted reads queried: a k-mer of abundance a answers a at each of its a windows, so the positions answering
    a number a * histogram[a]; with abundance_min = 2 the windows of the k-mers seen once answer 0 with the invalid positions."""
    from dsk_amd import KmerCounter, synth
    reads, gl, nr, rl = synth.make_workload("c2_10Mx150", dev)
    nbytes = reads.numel()
    torch.cuda.synchronize()
    for amin in (1, 2):
        with KmerCounter(kmer_size=31, abundance_min=amin, partition_order=partition_order) as kc:
            kc.set_reads_device(reads.data_ptr(), nbytes)
            kc.count()
            st, hist = kc.stats(), kc.histogram().astype(np.int64)
            out = kc.query_reads_tensor(reads)
            bins = positions_per_abundance(out, len(hist))
            del out
        assert int(hist[-1]) == 0                                          # nothing saturates the histogram on this workload
        a = np.arange(len(hist), dtype=np.int64)
        assert (bins[amin:-1] == (a * hist)[amin:-1]).all(), (amin, partition_order)
        if amin == 1:
            assert nbytes - int(bins[0]) == st["n_kmers"]
        else:
            assert int(bins[1]) == 0
            assert int(bins[0]) == nbytes - st["n_kmers"] + int(hist[1])
