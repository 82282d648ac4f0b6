"""Rows taken out of a result on the device (include/dskgpu.h: dskgpu_filter_rows; csrc/rowfilter.h: k_rows_compact, k_filter_offsets).

All comparisons are exact.  A seeded random mask keeps about half the rows; afterwards rows() must be rows()[mask], the partitions must
describe the kept rows, the count's stats and histogram must be untouched, and every consumer of the result -- lookups, unitigs, edges --
must answer for the kept rows: the unitigs and the edges are compared with the string restatement of the kept rows.  All of it fails before
the feature: KmerCounter has no filter_rows().
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from tests import test_gpu_unitig_edges as edges_mod      # noqa: E402
from tests import test_gpu_unitigs as unitigs_mod      # noqa: E402
from tests.test_gpu_partition_order_wide import ascending, inside_partitions      # noqa: E402
from tests.test_gpu_unitigs import code_of, count, row_values, stream_of      # noqa: E402
from tests.test_unitig_edges_restatement import EdgeRestatement      # noqa: E402

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def reads100k(dev):
    from dsk_amd import synth
    return synth.make_reads(synth.make_genome(300_000, dev), 100_000, 150)


def random_mask(n, seed):
    return np.random.default_rng(seed).integers(0, 2, n).astype(bool)


def keep_tensor(mask, dev, pad=64):
    """the flags of the rows followed by `pad` non-zero bytes: a filter that read past n_rows would keep more rows than the mask has"""
    t = torch.full((len(mask) + pad,), 255, dtype=torch.uint8, device=dev)
    t[: len(mask)] = torch.from_numpy(mask.astype(np.uint8)).to(dev)
    torch.cuda.synchronize()
    return t


def apply_mask(kc, mask, dev):
    """filter kc by mask and check everything that needs no restatement.  -> (rows before, abundances before, partition offsets before)"""
    kk, ab = kc.rows()
    off, P = kc.partition_offsets().astype(np.int64), kc.num_partitions()
    st, hist = kc.stats(), kc.histogram()
    n = len(kk)
    assert len(mask) == n == kc.result_device()[2]
    t = keep_tensor(mask, dev)
    left = kc.filter_rows(t.data_ptr())
    assert left == int(mask.sum()) == kc.result_device()[2]
    k2, a2 = kc.rows()
    assert k2.shape == (left, kk.shape[1]) and (k2 == kk[mask]).all() and (a2 == ab[mask]).all()
    assert kc.num_partitions() == P and kc.stats() == st and (kc.histogram() == hist).all()
    off2 = kc.partition_offsets().astype(np.int64)
    assert len(off2) == P + 1 and off2[0] == 0 and off2[-1] == left and (np.diff(off2) >= 0).all()
    return kk, ab, off


def check_partitions(kc, mask, off, partition_order):
    """partition order, wherever it was asked for: partition p holds the kept rows of the old partition p, still ascending; the old
    partitions are not the n * p / P ranges of the global order.  Global order: the n * p / P ranges of the rows left."""
    sizes = kc.partition_sizes()
    P, left, n = len(sizes), int(mask.sum()), len(mask)
    print("partitions", P, "partition order" if partition_order else "global order")
    if partition_order:
        assert np.diff(off).tolist() != [n * (p + 1) // P - n * p // P for p in range(P)], "partition order expected, the partitions are the global ranges"
        assert sizes.tolist() == [int(mask[off[p]: off[p + 1]].sum()) for p in range(P)]
        kk, _ = kc.rows()
        assert ascending(kk)[inside_partitions(sizes, len(kk))].all(), "a partition is not ascending"
    else:
        assert sizes.tolist() == [left * (p + 1) // P - left * p // P for p in range(P)]


def check_lookups(kc, kk, ab, mask, dev):
    got = kc.query_kmers_tensor(torch.from_numpy(np.ascontiguousarray(kk).view(np.int64)).to(dev)).cpu().numpy().view(np.uint32)
    assert (got == np.where(mask, ab, 0)).all()


def check_graph(kc, k):
    kk, ab = kc.rows()
    exp = EdgeRestatement(row_values(kk), ab, k)
    exp.check_facts()
    unitigs_mod.check_against_restatement(kc, exp)
    edges_mod.check_against_restatement(kc, exp)
    return exp


# ------------------------------------------------------------------ 1. golden reads: one, two and four words, both row orders
@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k", [31, 63, 96])
def test_golden_reads_filtered(oracle, golden_dir, dev, k, partition_order):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, k, abundance_min=2, partition_order=partition_order) as kc:
        kc.unitig_edges()                                                   # an index, a compaction and edges of the unfiltered rows: all stale afterwards
        mask = random_mask(kc.result_device()[2], 100 + k)
        kk, ab, off = apply_mask(kc, mask, dev)
        check_partitions(kc, mask, off, partition_order)
        check_lookups(kc, kk, ab, mask, dev)
        check_graph(kc, k)


# ------------------------------------------------------------------ 2. the 100 k reads: several passes in partition order (64-bit offsets), no sort
@pytest.mark.parametrize("kind,kw", [
    ("multi_pass_partition_order", dict(max_pass_mkeys=2, partition_order=True)),
    ("partition_order", dict(partition_order=True)),
    ("no_sort", dict(sort=False)),
])
def test_reads_filtered(reads100k, dev, kind, kw):
    from dsk_amd import KmerCounter
    with KmerCounter(kmer_size=31, abundance_min=2, **kw) as kc:
        kc.set_reads_device(reads100k.data_ptr(), reads100k.numel())
        kc.count()
        if kind.startswith("multi_pass"):
            assert kc.stats()["n_passes"] > 1, kc.stats()
        n = kc.result_device()[2]
        assert n > 100_000
        mask = random_mask(n, 7)
        kk, ab, off = apply_mask(kc, mask, dev)
        check_partitions(kc, mask, off, "partition_order" in kind)
        check_lookups(kc, kk, ab, mask, dev)
        st = kc.unitig_edges()                                              # the graph calls answer for the kept rows
        assert kc.unitigs()["stream_bytes"] == int(mask.sum()) + 31 * kc.unitigs()["n_unitigs"] and st["n_dead_ends"] > 0


# ------------------------------------------------------------------ 3. special masks, composition
def test_all_ones_changes_nothing_and_all_zeros_leaves_a_result_without_rows(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31, abundance_min=2, partition_order=True) as kc:
        kk, ab = kc.rows()
        sizes, un, ed = kc.partition_sizes(), kc.unitigs(), kc.unitig_edges()
        n = len(kk)
        apply_mask(kc, np.ones(n, dtype=bool), dev)
        assert (kc.partition_sizes() == sizes).all() and kc.unitigs() == un and kc.unitig_edges() == ed
        apply_mask(kc, np.zeros(n, dtype=bool), dev)
        assert kc.result_device()[2] == 0 and (kc.partition_sizes() == 0).all() and kc.stats()["n_solid"] == n
        assert all(v == 0 for v in kc.unitigs().values())
        assert kc.unitig_edges() == dict(n_edges=0, n_self=0, n_dead_ends=0, max_degree=0)
        off, targets, ends = kc.unitig_edges_tensor()
        assert off.tolist() == [0] and targets.numel() == 0 and ends.numel() == 0
        assert kc.unitigs_stream_tensor().numel() == 0 and kc.unitigs_rows_tensor()[0].numel() == 0
        check_lookups(kc, kk, ab, np.zeros(n, dtype=bool), dev)
        assert kc.filter_rows(0) == 0                                       # a result with zero rows: nothing to do, a null d_keep is fine
        assert kc.graph_tips(31) == dict(n_candidates=0, n_tips=0, n_outranked=0, n_rows_clipped=0, n_rounds=0, n_rows_left=0)
        assert kc.clip_tips()["n_rows_left"] == 0


@pytest.mark.parametrize("partition_order", [False, True])
def test_filtering_twice_composes(oracle, golden_dir, dev, partition_order):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 63, abundance_min=2, partition_order=partition_order) as kc:
        kk, ab = kc.rows()
        m1 = random_mask(len(kk), 1)
        _, _, off = apply_mask(kc, m1, dev)
        check_partitions(kc, m1, off, partition_order)
        m2 = random_mask(int(m1.sum()), 2)
        _, _, off1 = apply_mask(kc, m2, dev)
        check_partitions(kc, m2, off1, partition_order)
        both = m1.copy()
        both[np.nonzero(m1)[0]] = m2
        k2, a2 = kc.rows()
        assert (k2 == kk[both]).all() and (a2 == ab[both]).all()
        if partition_order:
            assert kc.partition_sizes().tolist() == [int(both[off[p]: off[p + 1]].sum()) for p in range(len(off) - 1)]
        m3 = random_mask(int(both.sum()), 3)                                # a third one: back into the first set of buffers
        apply_mask(kc, m3, dev)
        check_lookups(kc, k2, a2, m3, dev)
        check_graph(kc, 63)


def test_bool_and_uint8_tensors(oracle, golden_dir, dev):
    stream = stream_of("hand:33", oracle, golden_dir)
    with count(stream, dev, 33, abundance_min=1) as kc:
        kk, ab = kc.rows()
        mask = random_mask(len(kk), 5)
        assert kc.filter_rows_tensor(torch.from_numpy(mask).to(dev)) == int(mask.sum())
        m2 = random_mask(int(mask.sum()), 6)
        assert kc.filter_rows_tensor(torch.from_numpy(m2.astype(np.uint8) * 7).to(dev)) == int(m2.sum())      # non-zero = keep
        assert (kc.rows()[0] == kk[mask][m2]).all()
        with pytest.raises(ValueError):
            kc.filter_rows_tensor(torch.zeros(3, dtype=torch.uint8, device=dev))
        check_graph(kc, 33)


# ------------------------------------------------------------------ 4. lifecycle and errors
def test_errors(oracle, golden_dir, dev):
    from dsk_amd import KmerCounter
    buf = torch.ones(1 << 16, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with KmerCounter(kmer_size=31) as kc:
        assert code_of(lambda: kc.filter_rows(buf.data_ptr())) == E_STATE    # no result
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31) as kc:
        n = kc.result_device()[2]
        assert n <= buf.numel()
        assert code_of(lambda: kc.filter_rows(0)) == E_ARG                   # a null d_keep while there are rows
        assert kc.result_device()[2] == n
        assert kc._lib.dskgpu_filter_rows(kc._h, buf.data_ptr(), None) == 0  # n_kept may be NULL
        assert kc.result_device()[2] == n


def test_a_new_count_invalidates_the_filter(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31, abundance_min=2, partition_order=True) as kc:
        kk, ab = kc.rows()
        sizes = kc.partition_sizes()
        apply_mask(kc, random_mask(len(kk), 11), dev)
        kc.count()
        k2, a2 = kc.rows()
        assert (k2 == kk).all() and (a2 == ab).all() and (kc.partition_sizes() == sizes).all()
        check_lookups(kc, kk, ab, np.ones(len(kk), dtype=bool), dev)


def test_the_filter_leaves_the_kept_encoding_alone(reads100k, dev):
    """encode_reads() -> the 2-bit form is the only copy of the reads.  Count, filter, count again: the unfiltered rows."""
    from dsk_amd import KmerCounter
    buf = reads100k.clone()
    torch.cuda.synchronize()
    with KmerCounter(kmer_size=31, abundance_min=2) as kc:
        kc.set_reads_device(buf.data_ptr(), buf.numel())
        kc.encode_reads()
        buf.zero_(); torch.cuda.synchronize()                              # the bytes are gone
        kc.count()
        k1, a1 = kc.rows(); h1 = kc.histogram(); s1 = kc.stats()
        apply_mask(kc, random_mask(len(k1), 12), dev)
        kc.count()
        k2, a2 = kc.rows()
        assert (k2 == k1).all() and (a2 == a1).all() and (kc.histogram() == h1).all()
        s2 = kc.stats()
        assert (s2["n_kmers"], s2["n_distinct"], s2["n_solid"]) == (s1["n_kmers"], s1["n_distinct"], s1["n_solid"])


def test_a_rank_of_a_group(oracle, golden_dir, dev):
    """a rank's rows can be filtered; the tip rule has no compaction to work on there"""
    from dsk_amd import KmerGroup
    s = stream_of("golden", oracle, golden_dir)
    recs = bytes(s).split(b"\n")
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with KmerGroup([0, 0], kmer_size=31, abundance_min=2) as g:
        for r in range(2):
            g.rank(r).push_reads(b"\n".join(recs[r::2]) + b"\n")
        g.count()
        kc = g.rank(0)
        n = kc.result_device()[2]
        assert 0 < n <= buf.numel()
        mask = random_mask(n, 13)
        kk, ab, _ = apply_mask(kc, mask, dev)
        check_lookups(kc, kk, ab, mask, dev)
        assert int(kc.graph_adjacency().sum()) == int(mask.sum())
        for call in (lambda: kc.graph_tips(31, 0, buf.data_ptr(), 0), lambda: kc.clip_tips()):
            assert code_of(call) == E_STATE
            assert "world_size" in kc._lib.dskgpu_last_error(kc._h).decode()
        assert kc.result_device()[2] == int(mask.sum())


def test_stage_times_name_the_filter(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31, timing=True) as kc:
        before = dict(kc.stage_times())
        assert "filter rows" not in before
        n = kc.result_device()[2]
        kc.filter_rows_tensor(torch.from_numpy(random_mask(n, 14)).to(dev))
        after = dict(kc.stage_times())
        assert after["filter rows"] > 0
        assert all(after[name] == v for name, v in before.items())
