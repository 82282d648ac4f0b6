"""DSKGPU_F_PARTITION_ORDER for four-word k-mers (65 <= k <= 128; csrc/partsort.h: k_part_sort4).

What a caller at k <= 64 gets holds here too: thousands of output partitions of at most PS4_CAP rows, the rows strictly ascending
inside every partition under the full-width comparison (most significant word first), the partition calls of the C-ABI describing
that layout -- and the exact global order whenever a block cannot order its partition.  Every case is checked against the CPU
oracle: totals, histogram, and the rows as a sorted multiset (every word, with the abundances).

Inputs are those of test_partition_order_is_the_reference_contract (test_gpu_parity.py), so that the two are comparable.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PS4_CAP = 1024          # rows one block of k_part_sort4 orders (include/dskgpu.h, DSKGPU_F_PARTITION_ORDER)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def streams(dev, golden_dir, oracle):
    from dsk_amd import synth
    reads = synth.make_reads(synth.make_genome(600_000, dev), 250_000, 150).cpu().numpy()
    rng = np.random.default_rng(5)
    pa = np.full(300_000, 65, np.uint8)
    hit = rng.random(pa.size) < 0.03
    pa[hit] = rng.choice(np.frombuffer(b"CGT", dtype=np.uint8), size=int(hit.sum()))
    skew = np.concatenate([pa, np.array([10], np.uint8), reads]).astype(np.uint8)
    gold, _ = oracle.load_bank(os.path.join(golden_dir, "read50x_ref10K_e001.fasta.gz"))
    rng = np.random.default_rng(11)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    tiny = np.concatenate([rng.choice(acgt, 150), np.array([10], np.uint8), rng.choice(acgt, 120), np.array([10], np.uint8)]).astype(np.uint8)
    return {"reads": reads, "skew": skew, "gold": np.ascontiguousarray(gold), "tiny": tiny}


@pytest.fixture(scope="module")
def ref_of(oracle, streams):
    cache = {}

    def get(name, k):
        if (name, k) not in cache:
            cache[(name, k)] = oracle.count(np.ascontiguousarray(streams[name]), k)
        return cache[(name, k)]
    return get


def ascending(kk):
    """row i + 1 > row i, all words compared, the last column the most significant"""
    gt = np.zeros(max(len(kk) - 1, 0), dtype=bool)
    eq = np.ones(max(len(kk) - 1, 0), dtype=bool)
    for c in range(kk.shape[1] - 1, -1, -1):
        a, b = kk[1:, c], kk[:-1, c]
        gt |= eq & (a > b)
        eq &= a == b
    return gt


def inside_partitions(sizes, n):
    """mask over the n - 1 neighbour pairs: True where both rows lie in the same partition"""
    inside = np.ones(max(n - 1, 0), dtype=bool)
    starts = np.cumsum(sizes)[:-1]
    inside[starts[(starts > 0) & (starts <= n - 1)] - 1] = False
    return inside


def result(kc):
    sizes = kc.partition_sizes()
    kk, ab = kc.rows()
    return kk, ab, sizes, kc.histogram(), kc.stats()


def run(stream, k, amin, dev, **kw):
    from dsk_amd import KmerCounter
    t = torch.from_numpy(np.ascontiguousarray(stream)).to(dev)
    with KmerCounter(kmer_size=k, abundance_min=amin, partition_order=True, **kw) as kc:
        kc.set_reads_device(t.data_ptr(), t.numel())
        kc.count()
        return result(kc)


def check_parity(res, ref, k, amin):
    """totals, histogram, partition bookkeeping, the rows as a sorted multiset; every partition ascending.  -> (the global 'ascending' mask, oracle rows)"""
    kk, ab, sizes, hist, st = res
    keep = ref.ab >= amin
    want_k, want_a = ref.words()[keep], ref.ab[keep]
    assert st["n_kmers"] == ref.total and st["n_distinct"] == ref.distinct and st["n_solid"] == len(want_a), (k, amin, st)
    assert (hist == ref.histogram(10000)).all(), (k, amin)
    assert kk.shape == (len(want_a), (k + 31) // 32), (k, amin, kk.shape)
    assert sizes.sum() == len(want_a) and st["n_partitions"] == len(sizes), (k, amin, len(sizes))
    assert (sizes >= 0).all()
    order = np.lexsort(kk.T)                                      # (the last key of lexsort is the primary one: the most significant word)
    assert (kk[order] == want_k).all() and (ab[order] == want_a).all(), (k, amin)
    asc = ascending(kk)
    assert asc[inside_partitions(sizes, len(kk))].all(), (k, amin, "a partition is not ascending")
    return asc, want_k, want_a


def check_partitioned(res, ref, k, amin, min_parts=4):
    asc, _, _ = check_parity(res, ref, k, amin)
    sizes = res[2]
    print("k=%d amin=%d: %d rows in %d partitions, largest %d" % (k, amin, len(res[1]), len(sizes), sizes.max()))
    assert len(sizes) > min_parts and sizes.max() <= PS4_CAP, (k, amin, len(sizes), sizes.max())
    assert not asc.all(), (k, amin, "partition order expected, the rows are globally ascending")


def check_global(res, ref, k, amin):
    asc, want_k, want_a = check_parity(res, ref, k, amin)
    kk, ab, sizes, hist, st = res
    assert st["n_partitions"] == 4 and len(sizes) == 4, (k, amin, st)
    assert asc.all(), (k, amin, "global order expected")
    assert (kk == want_k).all() and (ab == want_a).all(), (k, amin)        # row for row, without re-sorting


@pytest.mark.parametrize("k,amin", [(65, 2), (65, 1), (80, 2), (96, 1), (97, 2), (101, 2), (101, 1), (127, 1), (128, 2)])
def test_partition_order_is_honoured_for_four_word_rows(streams, ref_of, dev, k, amin):
    """Fails before k_part_sort4: n_partitions is 4 there and the rows are globally ascending."""
    check_partitioned(run(streams["reads"], k, amin, dev), ref_of("reads", k), k, amin)


@pytest.mark.parametrize("k,amin", [(101, 1), (65, 2)])
def test_skewed_input_in_either_layout(streams, ref_of, dev, k, amin):
    """300 000 bases of poly-A with 3 % substitutions in front of the reads: a block may give up on the poly-A variants by itself --
    parity and the order inside every partition hold whichever layout comes back."""
    res = run(streams["skew"], k, amin, dev)
    check_parity(res, ref_of("skew", k), k, amin)
    print("skew k=%d amin=%d: %d partitions" % (k, amin, len(res[2])))


def test_a_block_that_gives_up_takes_the_global_order(streams, ref_of, dev, monkeypatch):
    """DSKGPU_PS_MAXC=1: two rows in one value bin raise the flag -- the rows the partition pass left dense go through the global sort of
    four-word rows and come back globally ascending."""
    monkeypatch.setenv("DSKGPU_PS_MAXC", "1")
    check_global(run(streams["reads"], 101, 1, dev), ref_of("reads", 101), 101, 1)


def test_several_passes(streams, ref_of, dev, monkeypatch):
    """Every pass orders its partitions on the way into the job's row arrays; a block that gives up in one of them sends the job's rows
    through the global sort."""
    res = run(streams["reads"], 101, 1, dev, max_pass_mkeys=2)
    st = res[4]
    assert st["n_passes"] > 4, st
    check_partitioned(res, ref_of("reads", 101), 101, 1, min_parts=4 * st["n_passes"])
    monkeypatch.setenv("DSKGPU_PS_MAXC", "1")
    res = run(streams["reads"], 101, 1, dev, max_pass_mkeys=2)
    assert res[4]["n_passes"] > 4, res[4]
    check_global(res, ref_of("reads", 101), 101, 1)


def test_switching_the_row_order_on_one_context(streams, ref_of, dev):
    from dsk_amd import KmerCounter
    ref = ref_of("reads", 101)
    t = torch.from_numpy(np.ascontiguousarray(streams["reads"])).to(dev)
    out = []
    with KmerCounter(kmer_size=101, abundance_min=1) as kc:
        kc.set_reads_device(t.data_ptr(), t.numel())
        for part in (False, True, False):
            kc.set_row_order(part)
            kc.count()
            out.append(result(kc))
    check_global(out[0], ref, 101, 1)
    check_partitioned(out[1], ref, 101, 1)
    check_global(out[2], ref, 101, 1)
    assert (out[0][0] == out[2][0]).all() and (out[0][1] == out[2][1]).all()


def test_small_row_sets(streams, ref_of, dev):
    """Fewer rows than one block holds, a bank whose reads are shorter than k (no window, no row), and a small bank: parity in either
    layout; empty partitions and an empty result are handled."""
    ref = ref_of("tiny", 70)
    assert 0 < ref.total < 200
    for amin in (1, 2):
        check_parity(run(streams["tiny"], 70, amin, dev), ref, 70, amin)
    ref = ref_of("gold", 65)
    assert ref.total == 180000 and ref.distinct == 95043
    res = run(streams["gold"], 65, 1, dev)
    check_parity(res, ref, 65, 1)
    assert len(res[1]) == 95043
    ref = ref_of("gold", 101)
    assert ref.total == 0
    kk, ab, sizes, hist, st = res = run(streams["gold"], 101, 1, dev)
    check_parity(res, ref, 101, 1)
    assert kk.shape[0] == 0 and ab.shape[0] == 0 and sizes.sum() == 0 and st["n_solid"] == 0
