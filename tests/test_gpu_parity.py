"""GPU parity tests: HIP path (through the C-ABI) vs the CPU oracle, bit-exact.

Contract: sorted multiset of (kmer, abundance) rows + exact
histogram.  Inputs: the reference's own fixtures (tests/golden/), seeded
synthetic streams, and the edge cases the reference tests (N runs, k = read
length, k > read length, multi-line records, empty input).
"""
import os

import numpy as np
import pytest

from tests.crafted_keys import top_word_twins

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


def gpu_count(stream_np, k, dev, amin=2, amax=2147483647, **kw):
    from dsk_amd import KmerCounter
    t = torch.from_numpy(np.array(stream_np, dtype=np.uint8)).to(dev)
    with KmerCounter(kmer_size=k, abundance_min=amin, abundance_max=amax, **kw) as kc:
        kc.set_reads_device(t.data_ptr(), t.numel())
        kc.count()
        torch.cuda.synchronize()
        kmers, ab = kc.rows()
        return kmers, ab, kc.histogram(), kc.stats()


def check_against_oracle(oracle, stream, k, dev, amin=2, amax=2147483647, **kw):
    kmers, ab, hist, st = gpu_count(stream, k, dev, amin, amax, **kw)
    ref = oracle.count(stream, k)
    lo, hi, rab = ref.solid(amin, amax)
    assert st["n_kmers"] == ref.total
    assert st["n_distinct"] == ref.distinct
    assert st["n_solid"] == len(rab)
    assert (hist == ref.histogram(10000)).all()
    assert kmers.shape[0] == len(rab)
    keep = (ref.ab >= amin) & (ref.ab <= amax)
    assert kmers.shape == (len(rab), (k + 31) // 32)
    assert (kmers == ref.words()[keep]).all()     # ascending order, same as the oracle; every 64-bit word
    assert (ab == rab).all()
    return st


def test_enumerate_matches_oracle(oracle, golden_dir, dev):
    from dsk_amd import KmerCounter
    s, _ = oracle.load_bank(os.path.join(golden_dir, "longread.fasta"))
    s = np.concatenate([s, np.frombuffer(b"ACGTNNNNacgtacgtACGTRYKM" * 7, dtype=np.uint8)])
    for k in (1, 2, 15, 16, 17, 27, 31, 32):
        t = torch.from_numpy(s).to(dev)
        out = torch.zeros(len(s), dtype=torch.int64, device=dev)
        val = torch.zeros(len(s), dtype=torch.uint8, device=dev)
        with KmerCounter(kmer_size=k) as kc:
            kc.k_enumerate(t.data_ptr(), len(s), out.data_ptr(), val.data_ptr())
        lo, hi, valid = oracle.enumerate(s, k)
        assert (val.cpu().numpy() == valid).all(), k
        assert (out.cpu().numpy().view(np.uint64) == lo).all(), k


def test_enumerate_two_words(oracle, golden_dir, dev):
    from dsk_amd import KmerCounter
    s, _ = oracle.load_bank(os.path.join(golden_dir, "longread.fasta"))
    for k in (33, 47, 63, 64):
        t = torch.from_numpy(s).to(dev)
        out = torch.zeros(2 * len(s), dtype=torch.int64, device=dev)
        val = torch.zeros(len(s), dtype=torch.uint8, device=dev)
        with KmerCounter(kmer_size=k) as kc:
            kc.k_enumerate(t.data_ptr(), len(s), out.data_ptr(), val.data_ptr())
        lo, hi, valid = oracle.enumerate(s, k)
        o = out.cpu().numpy().view(np.uint64).reshape(-1, 2)
        assert (val.cpu().numpy() == valid).all(), k
        assert (o[:, 0] == lo).all() and (o[:, 1] == hi).all(), k


@pytest.mark.parametrize("k", [65, 80, 95, 96, 97, 127, 128])
def test_enumerate_four_words(oracle, golden_dir, dev, k):
    """k = 65..128: four-word device keys (gen_kmersN), (k+31)/32 words per k-mer at the ABI."""
    from dsk_amd import KmerCounter
    s, _ = oracle.load_bank(os.path.join(golden_dir, "longread.fasta"))
    rng = np.random.default_rng(5)
    long_runs = rng.choice(np.frombuffer(b"ACGTacgt", dtype=np.uint8), size=30000)
    long_runs[rng.integers(0, 30000, size=40)] = ord("N")                                  # runs of ~750 bases
    s = np.concatenate([s[:30000], np.frombuffer(b"ACGTNNNNacgtacgtACGTRYKM" * 9, dtype=np.uint8), long_runs, s[30000:45000]])
    wo = (k + 31) // 32
    t = torch.from_numpy(s).to(dev)
    out = torch.zeros(wo * len(s), dtype=torch.int64, device=dev)
    val = torch.zeros(len(s), dtype=torch.uint8, device=dev)
    with KmerCounter(kmer_size=k) as kc:
        kc.k_enumerate(t.data_ptr(), len(s), out.data_ptr(), val.data_ptr())
    words, valid = oracle.enumerate_words(s, k)
    assert valid.sum() > 10000
    assert (val.cpu().numpy() == valid).all()
    assert (out.cpu().numpy().view(np.uint64).reshape(-1, wo) == words[:, :wo]).all()
    if wo < 4:
        assert (words[:, wo:] == 0).all()


@pytest.mark.parametrize("k", [65, 80, 96, 97, 127, 128])
def test_four_word_kmers_golden(oracle, golden_dir, dev, k):
    s, _ = oracle.load_bank(os.path.join(golden_dir, "longread.fasta"))
    check_against_oracle(oracle, s, k, dev, amin=1)
    s2, _ = oracle.load_bank(os.path.join(golden_dir, "read50x_ref10K_e001.fasta.gz"))     # 100 bp reads: none for k > 100
    check_against_oracle(oracle, s2, k, dev)


def test_four_word_kmers_synthetic_two_levels(oracle, dev):
    from dsk_amd import synth
    reads = synth.make_reads(synth.make_genome(300_000, dev), 100_000, 150).cpu().numpy()
    st = check_against_oracle(oracle, reads, 101, dev)         # 5 M k-mers of 4 words: two partition levels
    assert st["n_levels"] == 2
    check_against_oracle(oracle, reads[: 151 * 30_000], 72, dev, amin=3, amax=40)
    for k in (127, 128):
        st = check_against_oracle(oracle, reads[: 151 * 30_000], k, dev)
        assert st["n_kmers"] > 500_000


def test_four_word_multi_pass_banks_and_exchange(oracle, golden_dir, dev):
    """The side paths at k > 64: several passes over the key space, per-bank solidity, explicit-key exchange."""
    from dsk_amd import KmerCounter, synth
    reads = synth.make_reads(synth.make_genome(100_000, dev), 40_000, 150).cpu().numpy()
    st = check_against_oracle(oracle, reads, 80, dev, max_pass_mkeys=1)
    assert st["n_passes"] >= 3
    # two banks, solidity "min" (numpy restatement over per-bank oracle counts)
    a, b = reads[: 151 * 15_000], reads[151 * 15_000: 151 * 32_000]
    both = np.concatenate([a, b])
    t = torch.from_numpy(both).to(dev)
    with KmerCounter(kmer_size=70, abundance_min=2, solidity_kind="min") as kc:
        kc.set_reads_device(t.data_ptr(), t.numel())
        kc.set_banks([len(a), len(both)])
        kc.count()
        rows, ab = kc.rows()
    ra, rb = oracle.count(a, 70), oracle.count(b, 70)
    da = {int(v): int(c) for v, c in zip(ra.values(), ra.ab)}
    want = sorted((int(v), da[int(v)] + int(c)) for v, c in zip(rb.values(), rb.ab) if int(v) in da and min(da[int(v)], int(c)) >= 2)
    got = [((int(r[2]) << 128) | (int(r[1]) << 64) | int(r[0]), int(c)) for r, c in zip(rows, ab)]
    assert got == want and len(want) > 1000
    # multi-GPU: k > 64 travels as explicit four-word keys
    recs = bytes(reads[: 151 * 20_000]).split(b"\n")
    ctxs, sends, counts = [], [], []
    for r in range(2):
        shard = torch.from_numpy(np.frombuffer(b"\n".join(recs[r::2]) + b"\n", dtype=np.uint8).copy()).to(dev)
        kc = KmerCounter(kmer_size=90, abundance_min=1, world_size=2, rank=r)
        kc.set_reads_device(shard.data_ptr(), shard.numel())
        send = torch.zeros(kc.mg_send_capacity_words(), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        c = kc.mg_scatter(send.data_ptr(), send.numel())
        assert all(x % 4 == 0 for x in c)
        ctxs.append(kc); sends.append(send); counts.append(c)
    got_rows, got_ab = [], []
    for d in range(2):
        recv = torch.cat([sends[src][sum(counts[src][:d]): sum(counts[src][:d]) + counts[src][d]] for src in range(2)])
        torch.cuda.synchronize()
        ctxs[d].mg_count(recv.data_ptr(), recv.numel())
        rr, aa = ctxs[d].rows()
        got_rows.append(rr); got_ab.append(aa)
    rows = np.concatenate(got_rows); ab = np.concatenate(got_ab)
    ref = oracle.count(reads[: 151 * 20_000], 90)
    order = np.lexsort([rows[:, x] for x in range(3)])
    assert (rows[order] == ref.words()).all() and (ab[order] == ref.ab).all()
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("k", [27, 31])
def test_golden_T1(oracle, golden_dir, dev, k):
    s, _ = oracle.load_bank(os.path.join(golden_dir, "read50x_ref10K_e001.fasta.gz"))
    st = check_against_oracle(oracle, s, k, dev)
    if k == 31:   # BASELINE.json configs[0] known answer
        assert (st["n_kmers"], st["n_distinct"], st["n_solid"]) == (350000, 99957, 13096)


def test_golden_histo_files(oracle, golden_dir, dev):
    from tests.test_oracle_golden import read_histo
    for fasta, k, histo in (("read50x_ref10K_e001.fasta.gz", 27, "k27.histo"),
                            ("longread.fasta", 27, "rlong.histo"),
                            ("readN.fasta", 20, "readN.histo")):
        s, _ = oracle.load_bank(os.path.join(golden_dir, fasta))
        _, _, hist, _ = gpu_count(s, k, dev)
        assert (hist[1:] == read_histo(os.path.join(golden_dir, histo))).all(), fasta


def test_golden_T2_multifile_sum(oracle, golden_dir, dev):
    uri = ",".join(os.path.join(golden_dir, f"c{i}.fasta.gz") for i in (1, 2, 3, 4))
    s, _ = oracle.load_bank(uri)
    check_against_oracle(oracle, s, 27, dev)


def test_golden_T4_T5_short(oracle, golden_dir, dev):
    from dsk_amd.engine import kmer_to_string
    s, _ = oracle.load_bank(os.path.join(golden_dir, "shortread.fasta"))
    kmers, ab, _, _ = gpu_count(s, 15, dev, amin=1)
    lines = [f"{kmer_to_string(int(v), 15)} {a}" for v, a in zip(kmers[:, 0], ab)]
    assert lines == open(os.path.join(golden_dir, "short.parse_results")).read().splitlines()
    kmers, ab, hist, st = gpu_count(s, 16, dev, amin=1)
    assert len(ab) == 0 and st["n_kmers"] == 0 and hist.sum() == 0


def test_iupac_and_lowercase(oracle, golden_dir, dev):
    s, _ = oracle.load_bank(os.path.join(golden_dir, "IUPAC.fasta"))
    check_against_oracle(oracle, s, 21, dev, amin=1)
    s2 = np.frombuffer(b"acgtacgtacgtACGTACGTAAAANNNNacgtTTTTacgtacgt\n" * 50, dtype=np.uint8)
    check_against_oracle(oracle, s2, 11, dev, amin=1)


def test_empty_and_tiny_inputs(oracle, dev):
    for raw in (b"", b"\n", b"A", b"ACGT", b"N" * 100, b"ACGTACGTACGTACGTACGTACGTACGTACGTACGT"):
        s = np.frombuffer(raw, dtype=np.uint8)
        check_against_oracle(oracle, s, 5, dev, amin=1)
        check_against_oracle(oracle, s, 31, dev, amin=1)


def test_poly_a_skew(oracle, dev):
    # one k-mer repeated ~2M times plus noise: a single sub-partition takes all the duplicates
    rng = np.random.default_rng(7)
    noise = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=200_000)
    s = np.concatenate([np.full(2_000_000, 65, np.uint8), [10], noise, [10], np.full(500_000, 84, np.uint8)]).astype(np.uint8)
    check_against_oracle(oracle, s, 31, dev, amin=1)


@pytest.mark.parametrize("k,n_reads", [(31, 40_000), (21, 40_000), (32, 20_000), (9, 20_000)])
def test_synthetic_one_level(oracle, dev, k, n_reads):
    from dsk_amd import synth
    g = synth.make_genome(100_000, dev)
    reads = synth.make_reads(g, n_reads, 150)
    check_against_oracle(oracle, reads.cpu().numpy(), k, dev)


def test_synthetic_two_levels(oracle, dev):
    # > 2^10 * 2048 k-mers forces the two-level partition
    from dsk_amd import synth
    g = synth.make_genome(1_000_000, dev)
    reads = synth.make_reads(g, 40_000 * 5, 150)
    st = check_against_oracle(oracle, reads.cpu().numpy(), 31, dev)
    assert st["n_levels"] == 2


def test_histogram_free_scatters_and_their_fallback(oracle, dev, monkeypatch):
    """One-word keys, two levels: level 1 writes block-owned slices, level 2 owns whole segments and writes
    fixed-capacity regions -- no histogram pass at either level.  A slice / region that overflows must send the
    attempt through the exact histogram + scan path."""
    from dsk_amd import KmerCounter, synth
    reads = synth.make_reads(synth.make_genome(400_000, dev), 120_000, 150)
    ref = oracle.count(reads.cpu().numpy(), 31)

    def run():
        with KmerCounter(kmer_size=31, abundance_min=2, timing=True) as kc:
            kc.set_reads_device(reads.data_ptr(), reads.numel())
            kc.count()
            torch.cuda.synchronize()
            rows, ab = kc.rows()
            return rows, ab, kc.histogram(), kc.stats(), dict(kc.stage_times())

    def check(rows, ab, hist, st):
        keep = ref.ab >= 2
        assert st["n_levels"] == 2 and st["n_kmers"] == ref.total and st["n_distinct"] == ref.distinct
        assert (rows[:, 0] == ref.lo[keep]).all() and (ab == ref.ab[keep]).all() and (hist == ref.histogram(10000)).all()

    rows, ab, hist, st, stages = run()
    check(rows, ab, hist, st)
    assert "hist1" not in stages and "hist2" not in stages and st["n_retries"] == 0    # neither level ran a histogram pass
    monkeypatch.setenv("DSKGPU_OPT_SLICE", "64")                     # level-1 slices far too small: exact level 1, level 2 unchanged
    rows, ab, hist, st, stages = run()
    check(rows, ab, hist, st)
    assert "hist1" in stages and "hist2" not in stages and st["n_retries"] == 1
    monkeypatch.delenv("DSKGPU_OPT_SLICE")
    monkeypatch.setenv("DSKGPU_OPT_CAP", "1024")                     # level-2 regions far too small: every one overflows
    rows, ab, hist, st, stages = run()
    check(rows, ab, hist, st)
    assert "hist1" in stages and "hist2" in stages and st["n_retries"] == 1            # exact path took over at both levels
    monkeypatch.setenv("DSKGPU_NO_OPT2", "1")
    monkeypatch.delenv("DSKGPU_OPT_CAP")
    rows, ab, hist, st, stages = run()
    check(rows, ab, hist, st)
    assert "hist2" in stages and st["n_retries"] == 0


def _reads_with_planted_kmers(rng, n_reads, rl, k, planted):
    """Error-free reads of a random genome (20x) with `planted` = [(copies, seed)] fixed k-mers written over a random
    window of `copies` distinct reads each: k-mers with that many occurrences, spread evenly over the stream."""
    genome = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=max(rl + 1, n_reads * rl // 20))      # 20x coverage
    reads = genome[rng.integers(0, len(genome) - rl, size=n_reads)[:, None] + np.arange(rl)[None, :]]
    free = rng.permutation(n_reads)
    at = 0
    for copies, seed in planted:
        kmer = np.random.default_rng(seed).choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=k)
        rows = free[at: at + copies]; at += copies
        pos = rng.integers(0, rl - k + 1, size=copies)
        reads[rows[:, None], pos[:, None] + np.arange(k)[None, :]] = kmer[None, :]
    return np.concatenate([reads, np.full((n_reads, 1), ord("\n"), np.uint8)], axis=1).reshape(-1)


@pytest.mark.parametrize("k", [31, 63])
def test_region_chains_keep_heavy_kmers_on_the_histogram_free_path(oracle, dev, monkeypatch, k):
    """k-mers with thousands of occurrences outgrow the fixed-capacity region of their sub-partition (4360 one-word / 2180 two-word
    keys).  The level-2 scatter then chains extension regions to it and the count kernel walks the chain (k_count_chained, and
    k_count_chained_mw for two-word keys: k = 63): no retry, no histogram pass, rows and histogram equal the oracle's.  With the
    pool switched off (DSKGPU_MAX_EXT=0) the same input takes the exact path after one retry -- the behaviour before the chains."""
    from dsk_amd import KmerCounter
    rng = np.random.default_rng(42)
    stream = _reads_with_planted_kmers(rng, 50_000, 150, k, [(200, 1), (1500, 2), (2500, 3), (5000, 4), (9000, 5), (14000, 6)])
    ref = oracle.count(stream, k)
    t = torch.from_numpy(stream).to(dev)

    def run():
        with KmerCounter(kmer_size=k, abundance_min=2, timing=True) as kc:
            kc.set_reads_device(t.data_ptr(), t.numel())
            kc.count()
            rows, ab = kc.rows()
            return rows, ab, kc.histogram(), kc.stats(), dict(kc.stage_times())

    def check(rows, ab, hist, st):
        keep = ref.ab >= 2
        assert st["n_levels"] == 2 and st["n_kmers"] == ref.total and st["n_distinct"] == ref.distinct
        assert (rows == ref.words()[keep]).all() and (ab == ref.ab[keep]).all() and (hist == ref.histogram(10000)).all()

    assert ref.ab.max() >= 14000
    rows, ab, hist, st, stages = run()
    check(rows, ab, hist, st)
    assert st["n_retries"] == 0 and "hist1" not in stages and "hist2" not in stages
    assert st["n_ext_regions"] >= 2 + 3 + 1                 # 14000, 9000 and 5000 occurrences need at least 3, 2 and 1 regions more
    monkeypatch.setenv("DSKGPU_MAX_EXT", "2")              # a pool that runs dry: the exact path takes over
    rows, ab, hist, st, stages = run()
    check(rows, ab, hist, st)
    assert st["n_retries"] == 1 and "hist2" in stages
    monkeypatch.setenv("DSKGPU_MAX_EXT", "0")
    rows, ab, hist, st, stages = run()
    check(rows, ab, hist, st)
    assert st["n_retries"] == 1 and "hist2" in stages and st["n_ext_regions"] == 0


@pytest.mark.parametrize("k", [31, 63])
def test_repeat_rich_reads_stay_on_the_histogram_free_path(oracle, dev, monkeypatch, k):
    """A repeat-rich genome (a high-copy family, tandem arrays) plus poly-A reads -- dsk_amd.synth `small_repeats`, the small
    brother of the bench's `c2_repeats_10Mx150`: k-mers with 10^4 .. 10^5 occurrences.  The level-1 slices are sized per bin
    from the sampled loads and the level-2 regions chain extensions, so the count needs no retry and no histogram pass; with
    the sample switched off (slices from the mean load) the same input overflows level 1 and takes the exact path."""
    from dsk_amd import KmerCounter, synth
    reads, gl, nr, rl = synth.make_workload("small_repeats", dev)
    ref = oracle.count(reads.cpu().numpy(), k)
    assert ref.ab.max() > 20_000

    def run():
        with KmerCounter(kmer_size=k, abundance_min=2, timing=True) as kc:
            kc.set_reads_device(reads.data_ptr(), reads.numel())
            kc.count()
            rows, ab = kc.rows()
            return rows, ab, kc.histogram(), kc.stats(), dict(kc.stage_times())

    def check(rows, ab, hist, st):
        keep = ref.ab >= 2
        assert st["n_levels"] == 2 and st["n_kmers"] == ref.total and st["n_distinct"] == ref.distinct
        assert (rows == ref.words()[keep]).all() and (ab == ref.ab[keep]).all() and (hist == ref.histogram(10000)).all()

    rows, ab, hist, st, stages = run()
    check(rows, ab, hist, st)
    assert st["n_retries"] == 0 and "hist1" not in stages and "hist2" not in stages
    assert st["n_ext_regions"] > 0 and st["n_heavy"] >= 1          # (k = 63: two-word keys take the same path -- region chains, the poly-A k-mer counted apart)
    assert st["sort_fallback"] == 0          # (two-word rows: the ~100 error variants of poly-A that share their first 63 bits are ordered by k_fix_long_runs)
    monkeypatch.setenv("DSKGPU_NO_SAMPLE", "1")
    rows, ab, hist, st, stages = run()
    check(rows, ab, hist, st)
    assert st["n_retries"] >= 1 and "hist1" in stages and "hist2" not in stages      # level 1 exact, level 2 still chains


def test_mostly_invalid_stream_with_a_dense_tail(oracle, dev, monkeypatch):
    """A stream that is mostly N with the last blocks' chunks dense in a single repeated k-mer.  The level-1 slices are sized per
    bin from the sampled loads AND their measured spread over the tiles, and the k-mer that is nearly all of its bin is counted
    apart by the level-2 scatter: no retry.  With the sample switched off the slices come from the MEAN number of valid k-mers
    per block and that block's slice of one bin overflows by far: the kernels must keep every write inside the block's own
    slices (the overflow is reported and the exact path takes over)."""
    rng = np.random.default_rng(3)
    n_junk = 6_000_000
    junk = np.full(n_junk, ord("N"), dtype=np.uint8)
    junk[rng.integers(0, n_junk, 40_000)] = ord("A")                # isolated bases: no k-mer
    tail = np.frombuffer(b"A" * 3_000_000, dtype=np.uint8)          # 3 M copies of one k-mer, all in the last blocks' chunks
    some = np.frombuffer(("\n".join("".join(rng.choice(list("ACGT"), 150)) for _ in range(20_000))).encode(), dtype=np.uint8)
    stream = np.concatenate([junk, some, np.frombuffer(b"\n", dtype=np.uint8), tail])
    st = check_against_oracle(oracle, stream, 31, dev, amin=1)
    assert st["n_levels"] == 2 and st["n_retries"] == 0 and st["n_heavy"] == 1
    monkeypatch.setenv("DSKGPU_NO_SAMPLE", "1")
    st = check_against_oracle(oracle, stream, 31, dev, amin=1)
    assert st["n_levels"] == 2 and st["n_retries"] >= 1 and st["n_heavy"] == 0


def finer_partition_retry_case(oracle, reads, k, dev, monkeypatch):
    """the first half of test_table_overflow_retry_partitions_finer for one k: a load limit that the plain plan exceeds and a 2-4x
    finer one meets -> the stats of the repeated count (DSKGPU_TABLE_MAXLOAD stays set)"""
    from dsk_amd import KmerCounter
    with KmerCounter(kmer_size=k) as kc:
        t = torch.from_numpy(reads).to(dev)
        kc.set_reads_device(t.data_ptr(), t.numel())
        kc.count()
        st0 = kc.stats()
    per_sub = st0["n_distinct"] / st0["n_final_bins"]
    monkeypatch.setenv("DSKGPU_TABLE_MAXLOAD", str(max(8, int(per_sub * 0.8))))    # the first plan overflows, a 2-4x finer one fits
    st = check_against_oracle(oracle, reads, k, dev)
    assert 1 <= st["n_retries"] <= 3 and st["n_final_bins"] > st0["n_final_bins"]
    return st


def test_table_overflow_retry_partitions_finer(oracle, dev, monkeypatch):
    """A count table that would hold more distinct keys than its load limit flags overflow and the host repeats the pass
    with twice the sub-partitions (dskgpu.hip: extra_bits).  DSKGPU_TABLE_MAXLOAD lowers the limit so that the first
    plan overflows; the result must be the same and stats.n_retries says how often the plan was refined.  A limit no
    refinement can meet ends with DSKGPU_E_OVERFLOW after three retries."""
    from dsk_amd import synth, DskGpuError
    reads = synth.make_reads(synth.make_genome(300_000, dev), 60_000, 150).cpu().numpy()
    for k in (31, 63):
        finer_partition_retry_case(oracle, reads, k, dev, monkeypatch)
        monkeypatch.setenv("DSKGPU_TABLE_MAXLOAD", "1")
        with pytest.raises(DskGpuError) as e:
            gpu_count(reads, k, dev)
        assert e.value.code == -5
        monkeypatch.delenv("DSKGPU_TABLE_MAXLOAD")


@pytest.mark.parametrize("seed", range(12))
def test_randomized_two_level_inputs(oracle, dev, seed):
    """Seeded random inputs big enough for two partition levels (the histogram-free scatters), varying k (all key
    widths), read length, coverage, invalid-base rate, read order (shuffled / sorted by position: duplicates cluster
    in a block's chunks) and repeat content.  Whatever path the engine takes (slices, regions or the exact fallback)
    the rows and the histogram must equal the oracle's."""
    rng = np.random.default_rng(1000 + seed)
    k = int(rng.choice([15, 21, 27, 31, 32, 33, 41, 55, 63, 64, 70, 96]))
    rl = int(rng.choice([max(k + 5, 80), 150, 251, 1000]))
    n_kmers = int(rng.choice([4_500_000, 6_000_000]))                     # > 1024 sub-partitions for every width, also with 1 % N (the plan counts valid windows)
    if 32 < k <= 64:
        n_kmers *= 2                                                      # (two-word sub-partitions hold 2560 keys)
    n_reads = n_kmers // (rl - k + 1) + 1
    cov = float(rng.choice([1.5, 8.0, 40.0]))
    glen = max(1000, int(n_reads * rl / cov))
    genome = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=glen)
    if rng.random() < 0.4:                                                # a tandem repeat: heavy k-mers
        unit = genome[:37].copy(); genome[glen // 2: glen // 2 + 37 * 400] = np.tile(unit, 400)[: min(37 * 400, glen - glen // 2)]
    starts = rng.integers(0, max(1, glen - rl), size=n_reads)
    if rng.random() < 0.5:
        starts.sort()                                                     # position-sorted reads
    idx = starts[:, None] + np.arange(rl)[None, :]
    reads = genome[np.minimum(idx, glen - 1)]
    bad = rng.random(reads.shape) < float(rng.choice([0.0, 0.001, 0.01]))
    reads = np.where(bad, np.uint8(ord("N")), reads)
    flip = rng.random(n_reads) < 0.5                                      # reverse-complement half of the reads
    comp = np.zeros(256, np.uint8); comp[list(b"ACGTN")] = list(b"TGCAN")
    reads[flip] = comp[reads[flip]][:, ::-1]
    stream = np.concatenate([reads, np.full((n_reads, 1), ord("\n"), np.uint8)], axis=1).reshape(-1)
    amin = int(rng.choice([1, 2, 3]))
    st = check_against_oracle(oracle, stream, k, dev, amin=amin)
    assert st["n_levels"] == 2


@pytest.mark.parametrize("seed,ks", [(208, None), (292, None), (319, None), (304, None), (273, None), (545, (15, 21, 27, 31, 32)), (511, (15, 21, 27, 31, 32))])
def test_randomized_low_complexity_and_tiny_passes(oracle, dev, seed, ks):
    """Inputs of tools/stress_random.py (about a thousand seeds ran against the oracle: profiles/r04_stress/) that took a
    path of their own: a 200 kb low-complexity stretch (180 K rows under one 10-bit prefix: seeds 208 / 292 / 319 made the row sorts'
    'heavy bucket' limit 64 x the mean instead of 16 x), tandem arrays at 200 x coverage, and multi-pass counts of tiny passes whose
    sampled slices overflow (retries, same rows)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from stress_random import make_input
    stream, k, amin, kw, desc = make_input(seed, ks) if ks else make_input(seed)
    st = check_against_oracle(oracle, stream, k, dev, amin=amin, **kw)
    assert st["sort_fallback"] == 0, (desc, st)


@pytest.mark.parametrize("k", [33, 47, 63, 64])
def test_two_word_kmers_golden(oracle, golden_dir, dev, k):
    s, _ = oracle.load_bank(os.path.join(golden_dir, "read50x_ref10K_e001.fasta.gz"))
    st = check_against_oracle(oracle, s, k, dev)
    if k == 63:   # SURVEY.md App. A known answer
        assert (st["n_kmers"], st["n_distinct"], st["n_solid"]) == (190000, 97702, 10945)


def test_two_word_kmers_synthetic_two_levels(oracle, dev):
    from dsk_amd import synth
    g = synth.make_genome(500_000, dev)
    reads = synth.make_reads(g, 150_000, 150)
    st = check_against_oracle(oracle, reads.cpu().numpy(), 63, dev)
    assert st["n_levels"] == 2


@pytest.mark.parametrize("which", ["twins", "sentinel"])
def test_two_word_top_word_table_falls_back_on_what_it_cannot_tell_apart(oracle, dev, which):
    """k_count2v3 keys its table by the mixed top word alone and checks every key's low word afterwards: two different k-mers that
    share the top word, or a k-mer whose top word is the empty-slot value, send the attempt to k_count_mw -- same rows as the oracle."""
    from dsk_amd import synth
    k = 63
    g = synth.make_genome(500_000, dev)
    reads = synth.make_reads(g, 150_000, 150).cpu().numpy()
    st = check_against_oracle(oracle, reads, k, dev)
    assert st["n_levels"] == 2 and st["n_retries"] == 0
    a, b, c = top_word_twins(k, np.random.default_rng(5))
    extra = (a + "\n") * 3 + (b + "\n") * 5 if which == "twins" else (c + "\n") * 4
    stream = np.concatenate([reads, np.frombuffer(extra.encode(), dtype=np.uint8)])
    st = check_against_oracle(oracle, stream, k, dev)
    assert st["n_retries"] == 1          # the verification bit went up once, k_count_mw counted the pass


def test_two_word_top_word_twins_in_several_passes_and_on_the_receive_side(oracle, dev):
    """The same crafted k-mers (two 63-mers with one mixed top word) where the count stage runs per pass: a multi-pass count from the
    reads and the receive side of a two-rank job.  Passes and owners are functions of the MINIMIZER, so the twins may or may
    not meet in one table; either way the rows must be the oracle's, with at most one re-count."""
    from dsk_amd import KmerCounter, synth
    k = 63
    g = synth.make_genome(500_000, dev)
    reads = synth.make_reads(g, 150_000, 150).cpu().numpy()
    a, b, _ = top_word_twins(k, np.random.default_rng(5))
    extra = np.frombuffer(((a + "\n") * 3 + (b + "\n") * 5).encode(), dtype=np.uint8)
    stream = np.concatenate([reads, extra])
    st = check_against_oracle(oracle, stream, k, dev, max_pass_mkeys=4)
    assert st["n_passes"] >= 3 and st["n_retries"] <= 1, st              # (a re-count only when the twins' minimizers put them into the same pass)
    world = 2
    half = (150_000 // 2) * 151
    shards = [np.concatenate([reads[:half], extra[: 3 * 64]]), np.concatenate([reads[half:], extra[3 * 64:]])]      # twin a on rank 0, twin b on rank 1
    ctxs, sends, counts, keep_alive = [], [], [], []
    for r in range(world):
        t = torch.from_numpy(shards[r].copy()).to(dev)
        kc = KmerCounter(kmer_size=k, abundance_min=2, world_size=world, rank=r)
        kc.set_reads_device(t.data_ptr(), t.numel())
        send = torch.zeros(kc.mg_send_capacity_words(), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        counts.append(kc.mg_scatter(send.data_ptr(), send.numel()))
        ctxs.append(kc); sends.append(send); keep_alive.append(t)
    rows_k, rows_a, hist, retries = [], [], np.zeros(10001, np.uint64), 0
    for d in range(world):
        recv = torch.cat([sends[src][sum(counts[src][:d]): sum(counts[src][:d]) + counts[src][d]] for src in range(world)])
        torch.cuda.synchronize()
        ctxs[d].mg_count(recv.data_ptr(), recv.numel())
        kk, aa = ctxs[d].rows()
        rows_k.append(kk); rows_a.append(aa); hist += ctxs[d].histogram(); retries += ctxs[d].stats()["n_retries"]
    kk = np.concatenate(rows_k); aa = np.concatenate(rows_a)
    ref = oracle.count(stream, k)
    keep = ref.ab >= 2
    order = np.lexsort((kk[:, 0], kk[:, 1]))
    assert (hist == ref.histogram(10000)).all()
    assert (kk[order] == ref.words()[keep]).all() and (aa[order] == ref.ab[keep]).all()
    assert retries <= 1              # (1 when both twins have the same owner -- their minimizers decide)
    for c in ctxs:
        c.close()


def test_two_word_edge_cases(oracle, golden_dir, dev):
    s, _ = oracle.load_bank(os.path.join(golden_dir, "longread.fasta"))
    check_against_oracle(oracle, s, 41, dev, amin=1)
    s = np.concatenate([np.full(300_000, 65, np.uint8), np.array([10], np.uint8), np.full(100_000, 67, np.uint8)])
    check_against_oracle(oracle, s, 63, dev, amin=1)          # one k-mer x 300k: oversized sub-partition path
    for raw in (b"", b"ACGT" * 10, b"ACGT" * 16 + b"N" + b"TTGCA" * 20):
        check_against_oracle(oracle, np.frombuffer(raw, dtype=np.uint8), 40, dev, amin=1)


def test_abundance_window_and_histo_max(oracle, dev):
    from dsk_amd import synth, KmerCounter
    g = synth.make_genome(20_000, dev)
    reads = synth.make_reads(g, 10_000, 150).cpu().numpy()
    check_against_oracle(oracle, reads, 25, dev, amin=3, amax=40)
    t = torch.from_numpy(reads).to(dev)
    with KmerCounter(kmer_size=25, histo_max=20) as kc:
        kc.set_reads_device(t.data_ptr(), t.numel())
        kc.count()
        h = kc.histogram()
    assert (h == oracle.count(reads, 25).histogram(20)).all()


def test_push_reads_host_path(oracle, golden_dir, dev):
    from dsk_amd import KmerCounter
    uri = [os.path.join(golden_dir, f"c{i}.fasta.gz") for i in (1, 2, 3, 4)]
    whole, _ = oracle.load_bank(",".join(uri))
    with KmerCounter(kmer_size=27) as kc:
        for u in uri:                     # one push per file: separator implied between pushes
            s, _ = oracle.load_bank(u)
            kc.push_reads(s.tobytes())
        kc.count()
        kmers, ab = kc.rows()
    lo, hi, rab = oracle.count(whole, 27).solid(2)
    assert (kmers[:, 0] == lo).all() and (ab == rab).all()


def test_push_reads_staging_and_reserve(oracle, dev):
    """Host pushes larger than the pinned staging buffers (2 x 32 MB), from bytes and from a numpy array, with the
    device buffer reserved up front, reserved late (after the first push) and not at all: always the same count."""
    from dsk_amd import KmerCounter, synth
    reads = synth.make_reads(synth.make_genome(500_000, dev), 600_000, 150).cpu().numpy()      # 90 MB
    ref = oracle.count(reads, 25)
    cut = [0, 151 * 250_000, 151 * 250_001, len(reads)]
    for mode in ("none", "first", "late"):
        with KmerCounter(kmer_size=25, abundance_min=3) as kc:
            if mode == "first":
                kc.reserve_reads(len(reads) + 64)
            for i in range(3):
                piece = reads[cut[i]: cut[i + 1]]
                kc.push_reads(piece if i != 1 else piece.tobytes())
                if mode == "late" and i == 0:
                    kc.reserve_reads(len(reads) + 64)
            kc.count()
            rows, ab = kc.rows()
            st = kc.stats()
        keep = ref.ab >= 3
        assert st["n_kmers"] == ref.total and (rows[:, 0] == ref.lo[keep]).all() and (ab == ref.ab[keep]).all(), mode
    # piece sizes the staging copy splits over 2, 4 and 8 threads with a remainder: n = T * 4096 * q + 1 (r06: the last byte of such a
    # piece was not copied -- one k-mer in 3 * 10^8 off on a sequencer-like file)
    recs = [0, 15950, 15950 + 65102, 15950 + 65102 + 130638, 600_000]
    assert [151 * (recs[i + 1] - recs[i]) - 1 for i in range(3)] == [2408449, 9830401, 19726337]
    with KmerCounter(kmer_size=25, abundance_min=3) as kc:
        for i in range(4):
            kc.push_reads(reads[151 * recs[i]: 151 * recs[i + 1] - 1])          # (without the last separator: one is implied behind a push)
        kc.count()
        rows, ab = kc.rows()
        st = kc.stats()
    assert st["n_kmers"] == ref.total and (rows[:, 0] == ref.lo[keep]).all() and (ab == ref.ab[keep]).all()


def test_encode_reads_lets_go_of_the_bytes(oracle, dev):
    """dskgpu_encode_reads: the reads become their 2-bit form once and the caller's buffer is never read again -- overwritten here
    with other reads right after the call; single pass, several passes (record-based level 0) and the multi-GPU sender all start from
    the kept encoding.  Per-bank modes need the bytes: DSKGPU_E_STATE.  New reads start a new read set."""
    from dsk_amd import KmerCounter, synth
    from dsk_amd.engine import DskGpuError
    from dsk_amd.multi import scatter_records
    reads = synth.make_reads(synth.make_genome(300_000, dev), 100_000, 150)
    other = synth.make_reads(synth.make_genome(300_000, dev, seed=99), 100_000, 150, seed=100)
    ref = oracle.count(reads.cpu().numpy(), 31)
    buf = reads.clone()
    for mkeys in (0, 2):
        with KmerCounter(kmer_size=31, abundance_min=1, max_pass_mkeys=mkeys) as kc:
            buf.copy_(reads); torch.cuda.synchronize()
            kc.set_reads_device(buf.data_ptr(), buf.numel())
            kc.encode_reads()
            buf.copy_(other); torch.cuda.synchronize()            # the bytes are gone
            for _ in range(2):
                kc.count()
                st = kc.stats()
                assert (st["n_kmers"], st["n_distinct"]) == (ref.total, ref.distinct) and (kc.histogram() == ref.histogram(10000)).all()
                assert (kc.rows()[0][:, 0] == ref.lo).all()
            send, counts = scatter_records(kc, None, dev)           # the sender too
            assert kc.mg_sent_kmers() == [ref.total]
            kc.set_reads_device(buf.data_ptr(), buf.numel())        # a new read set: the other reads
            kc.count()
            assert kc.stats()["n_distinct"] != ref.distinct
    with KmerCounter(kmer_size=31, abundance_min=1, solidity_kind="min") as kc:
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        kc.set_banks([reads.numel() // 2 // 151 * 151, reads.numel()])
        kc.encode_reads()
        with pytest.raises(DskGpuError):
            kc.count()


def test_determinism_and_reuse(dev):
    from dsk_amd import synth, KmerCounter
    g = synth.make_genome(200_000, dev)
    reads = synth.make_reads(g, 60_000, 150)
    with KmerCounter(kmer_size=31) as kc:
        outs = []
        for _ in range(3):                # same ctx reused: buffers recycled, same answer
            kc.set_reads_device(reads.data_ptr(), reads.numel())
            kc.count()
            k, a = kc.rows()
            outs.append((k.copy(), a.copy(), kc.histogram().copy()))
    for k, a, h in outs[1:]:
        assert (k == outs[0][0]).all() and (a == outs[0][1]).all() and (h == outs[0][2]).all()


def full_size_invariants(st, h, kmers, ab, k, reads, nr, rl, dev):
    """Size-independent properties of a finished count: sum(abundance * hist) == n_kmers, sum(hist) == n_distinct,
    strictly ascending rows, solid count == hist tail, hist of the rows == hist tail, n_kmers == number of full ACGT windows."""
    idx = np.arange(len(h), dtype=np.int64)
    assert h[-1] == 0                                   # nothing saturates the last row here
    assert int((h * idx).sum()) == st["n_kmers"]
    assert int(h.sum()) == st["n_distinct"]
    assert int(h[2:].sum()) == st["n_solid"] == len(ab)
    if k <= 32:
        assert (np.diff(kmers[:, 0].astype(np.uint64)) > 0).all()   # strictly ascending, no duplicates
    else:
        hi, lo = kmers[:, 1].astype(np.uint64), kmers[:, 0].astype(np.uint64)
        assert ((hi[1:] > hi[:-1]) | ((hi[1:] == hi[:-1]) & (lo[1:] > lo[:-1]))).all()
    assert (np.bincount(np.minimum(ab, 10000), minlength=10001)[2:] == h[2:]).all()
    # every read position with a full ACGT window contributes exactly one k-mer
    r = reads.view(nr, rl + 1)[:, :rl]
    n_valid = 0
    step = 2_000_000
    for r0 in range(0, nr, step):
        bad = (r[r0:r0 + step] == 78)
        run = torch.zeros(bad.shape[0], dtype=torch.int32, device=dev)
        for j in range(rl):
            run = torch.where(bad[:, j], torch.zeros_like(run), run + 1)
            n_valid += int((run >= k).sum())
    assert n_valid == st["n_kmers"]


@pytest.mark.parametrize("workload,k", [("ecoli50x", 31), ("c2_10Mx150", 31), ("c2_10Mx150", 63),
                                        ("c3_shard_25Mx150", 31), ("c3_shard_25Mx150", 63),
                                        ("c3_200Mx150", 31), ("c3_200Mx150", 63)])
def test_full_size_invariants(oracle, dev, workload, k, monkeypatch):
    """Size-independent properties at BASELINE.json's full sizes.  configs[1] = c2_10Mx150 (the headline workload) is ALSO compared
    with the CPU oracle at full size, row for row and histogram bin for bin, at k = 31 and k = 63 (the oracle counts it in seconds
    on the GPU box's host cores); c3_shard_25Mx150 = one GPU's share (25 M reads, 3.0e9 k-mers at k = 31) of configs[2] (k = 31) and
    configs[3] (k = 63, two-word keys); c3_200Mx150 = the WHOLE volume of configs[2] / configs[3] (200 M reads, 30 GB of reads,
    2.4e10 / 1.76e10 k-mers) on this one GPU, as several passes over the key space -- the 8-GPU topology itself is the driver's
    to run."""
    from dsk_amd import synth, KmerCounter
    gl, nr, rl = synth.workload(workload)
    g = synth.make_genome(gl, dev)
    reads = synth.make_reads(g, nr, rl)
    del g
    def count():
        with KmerCounter(kmer_size=k, abundance_min=2) as kc:
            kc.set_reads_device(reads.data_ptr(), reads.numel())
            kc.count()
            return kc.stats(), kc.histogram().astype(np.int64), kc.rows()
    st, h, (kmers, ab) = count()
    torch.cuda.empty_cache()
    if workload == "c2_10Mx150":      # the histogram-free scatters and the exact histogram + scan path must agree row for row
        monkeypatch.setenv("DSKGPU_NO_OPT2", "1")
        st2, h2, (kmers2, ab2) = count()
        monkeypatch.delenv("DSKGPU_NO_OPT2")
        assert (h2 == h).all() and (kmers2 == kmers).all() and (ab2 == ab).all() and st2["n_distinct"] == st["n_distinct"]
        del kmers2, ab2
        # ... and both must equal the CPU oracle's count of the same 1.51 GB stream (the parity gate)
        ref = oracle.count(reads.cpu().numpy(), k, threads=os.cpu_count())
        keep = ref.ab >= 2
        assert st["n_kmers"] == ref.total and st["n_distinct"] == ref.distinct and st["n_solid"] == int(keep.sum())
        assert (h == ref.histogram(10000).astype(np.int64)).all()
        assert (ab == ref.ab[keep]).all()
        assert (kmers[:, 0] == ref.lo[keep]).all()
        if k > 32:
            assert (kmers[:, 1] == ref.hi[keep]).all()
        del ref, keep
    full_size_invariants(st, h, kmers, ab, k, reads, nr, rl, dev)


def test_full_size_repeat_rich(oracle, dev, monkeypatch):
    """The bench workload's repeat-rich twin (10 M x 150 bp; a 1 % high-copy family, tandem arrays, 0.2 % poly-A reads: k-mers
    with 10^4 .. 1.8 * 10^6 occurrences) at full size: no retry, no sort fallback, one k-mer counted apart, thousands of
    extension regions -- and the rows and the histogram equal both the exact histogram + scan path's (DSKGPU_NO_OPT2) and the
    CPU oracle's."""
    from dsk_amd import KmerCounter, synth
    reads, gl, nr, rl = synth.make_workload("c2_repeats_10Mx150", dev)

    def run():
        with KmerCounter(kmer_size=31, abundance_min=2, timing=True) as kc:
            kc.set_reads_device(reads.data_ptr(), reads.numel())
            kc.count()
            torch.cuda.synchronize()
            rows, ab = kc.rows()
            return rows, ab, kc.histogram(), kc.stats(), dict(kc.stage_times())

    rows, ab, hist, st, stages = run()
    assert st["n_retries"] == 0 and st["sort_fallback"] == 0 and "hist1" not in stages and "hist2" not in stages
    assert st["n_heavy"] == 1 and st["n_ext_regions"] > 1000
    assert (np.diff(rows[:, 0].astype(np.uint64)) > 0).all() and int(hist.sum()) == st["n_distinct"] and hist[10000] > 50     # (the last row saturates here)
    monkeypatch.setenv("DSKGPU_NO_OPT2", "1")
    rows2, ab2, hist2, st2, stages2 = run()
    monkeypatch.delenv("DSKGPU_NO_OPT2")
    assert "hist1" in stages2 and "hist2" in stages2 and st2["n_ext_regions"] == 0 and st2["n_heavy"] == 0
    assert (rows == rows2).all() and (ab == ab2).all() and (hist == hist2).all()
    assert st["n_kmers"] == st2["n_kmers"] and st["n_distinct"] == st2["n_distinct"]
    del rows2, ab2
    ref = oracle.count(reads.cpu().numpy(), 31, threads=os.cpu_count())
    keep = ref.ab >= 2
    assert st["n_kmers"] == ref.total and st["n_distinct"] == ref.distinct and int(ref.ab.max()) > 1_000_000
    assert (hist == ref.histogram(10000)).all() and (rows[:, 0] == ref.lo[keep]).all() and (ab == ref.ab[keep]).all()


def _device_rows(kc, dev):
    """The sorted result of a one-word count as torch tensors (copied out of the context's buffers: they stay valid after it closes)."""
    import ctypes
    kp, ap, n = kc.result_device()
    k = torch.empty(n, dtype=torch.int64, device=dev); a = torch.empty(n, dtype=torch.int32, device=dev)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy(ctypes.c_void_p(k.data_ptr()), ctypes.c_void_p(kp), ctypes.c_size_t(n * 8), 3)
    hip.hipMemcpy(ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(ap), ctypes.c_size_t(n * 4), 3)
    return k, a


def test_human_standin_on_one_gpu(dev):
    """BASELINE.json configs[4] ("30x human short reads (~90 Gbp), k=31, abundance-min=2, ... multi-pass HBM partitioning"), the
    stand-in SURVEY.md section 8(d) allows: 600 M x 150 bp reads of a repeat-rich 3 Gbp genome (one high-copy family, tandem arrays,
    0.2 % poly-A reads: ONE k-mer with 1.4e8 occurrences) counted on ONE GPU -- 7.2e10 k-mers in 60 passes over the key space, the
    passes' super-k-mer records materialised by 2 sweeps over the reads (the reference's own human run took 7 passes over its
    input: doc/human_log:3-4; README.md:126-130 "below 10").  No retry, no sort fallback, every size-independent invariant holds
    (3.4e9 sorted rows checked on the device)."""
    from dsk_amd import KmerCounter, synth
    from tests.full_size import device_invariants, valid_windows
    nr, rl = 600_000_000, 150
    genome = synth.make_genome_repeats(3_000_000_000, dev)
    reads = synth.make_reads(genome, nr, rl, polya_rate=0.002)
    del genome
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    with KmerCounter(kmer_size=31, abundance_min=2) as kc:
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        # the reads are encoded once and their 90 GB of bytes given back (dskgpu_encode_reads): the records of the 60 passes then need two
        # sweeps over the (2-bit) reads instead of three
        n_valid = valid_windows(reads, nr, rl, 31)
        kc.encode_reads()
        del reads
        torch.cuda.empty_cache()
        kc.count()
        st = kc.stats()
        assert st["n_retries"] == 0 and st["sort_fallback"] == 0, st
        assert st["n_passes"] > 20 and 1 <= st["n_read_sweeps"] <= 2, st
        assert st["n_heavy"] >= 1 and st["n_ext_regions"] > 1000, st
        inv = device_invariants(kc, st, kc.histogram(), 31, None, nr, rl, dev, n_valid=n_valid)
        assert inv["rows_checked"] == st["n_solid"] > 3_000_000_000 and inv["saturated_histogram_rows"] > 0
    torch.cuda.empty_cache()


def test_human_standin_shard_against_the_exact_path_and_eight_ranks(dev, monkeypatch):
    """One GPU's share of the same job (75 M reads of the 3 Gbp repeat-rich genome: 9e9 k-mers at 3.75x coverage, several passes):
    the fast path's rows and histogram must equal, row for row, what the exact histogram + scan path gives (DSKGPU_NO_OPT2), with no
    retry on the fast path.  And the topology of the 8-GPU job, emulated: a quarter of that shard split over 8 ranks of one
    in-process group (records by minimizer owner, device copies for the exchange) -- every rank stays on the histogram-free path
    although one of them owns the poly-A k-mer, and the union of the ranks' rows equals the single-GPU count of the same reads."""
    from dsk_amd import KmerCounter, KmerGroup, synth
    from tests.full_size import device_invariants
    nr, rl = 75_000_000, 150
    genome = synth.make_genome_repeats(3_000_000_000, dev)
    reads = synth.make_reads(genome, nr, rl, polya_rate=0.002)
    del genome
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    with KmerCounter(kmer_size=31, abundance_min=2) as kc:
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        kc.count()
        st, hist = kc.stats(), kc.histogram()
        assert st["n_retries"] == 0 and st["sort_fallback"] == 0 and st["n_passes"] > 1, st
        device_invariants(kc, st, hist, 31, reads, nr, rl, dev)
        k1, a1 = _device_rows(kc, dev)
    torch.cuda.empty_cache()
    monkeypatch.setenv("DSKGPU_NO_OPT2", "1")
    with KmerCounter(kmer_size=31, abundance_min=2) as kc:
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        kc.count()
        st2 = kc.stats()
        assert (st2["n_kmers"], st2["n_distinct"], st2["n_solid"]) == (st["n_kmers"], st["n_distinct"], st["n_solid"])
        assert (kc.histogram() == hist).all()
        k2, a2 = _device_rows(kc, dev)
    monkeypatch.delenv("DSKGPU_NO_OPT2")
    assert torch.equal(k1, k2) and torch.equal(a1, a2)
    del k1, a1, k2, a2
    torch.cuda.empty_cache()
    # ---- 8 ranks on a quarter of the shard
    nq = nr // 4
    quarter = reads[: nq * (rl + 1)]
    with KmerCounter(kmer_size=31, abundance_min=2) as kc:
        kc.set_reads_device(quarter.data_ptr(), quarter.numel())
        kc.count()
        sq, hq = kc.stats(), kc.histogram()
        kq, aq = _device_rows(kc, dev)
    torch.cuda.empty_cache()
    ranks = 8
    per = nq // ranks
    with KmerGroup([0] * ranks, kmer_size=31, abundance_min=2, nb_partitions=1, timing=True) as g:
        for r in range(ranks):
            lo, hi = r * per * (rl + 1), (nq if r == ranks - 1 else (r + 1) * per) * (rl + 1)
            g.rank(r).set_reads_device(quarter.data_ptr() + lo, hi - lo)
        g.count()
        sg = g.stats()
        assert (sg["n_kmers"], sg["n_distinct"], sg["n_solid"]) == (sq["n_kmers"], sq["n_distinct"], sq["n_solid"])
        assert (g.histogram() == hq).all()
        per_rank = [g.rank(r).stats() for r in range(ranks)]
        stages = [dict(g.rank(r).stage_times()) for r in range(ranks)]
        assert all(s["n_retries"] == 0 and s["sort_fallback"] == 0 for s in per_rank), per_rank
        assert all("hist1" not in t and "hist2" not in t for t in stages)
        assert sum(s["n_heavy"] for s in per_rank) >= 1
        rows = [_device_rows(g.rank(r), dev) for r in range(ranks)]
    kk = torch.cat([x[0] for x in rows]); aa = torch.cat([x[1] for x in rows])
    del rows
    order = torch.argsort(kk)
    assert torch.equal(kk[order], kq) and torch.equal(aa[order], aq)


def test_full_size_more_than_2_pow_32_rows(dev):
    """More than 2^32 solid rows on one GPU (`-abundance-min 1` keeps every distinct k-mer; the reference streams
    rows to Partition<Count> without a bound, utils/dsk2ascii.cpp:61,77): 60 M x 150 bp reads at 4 % substitutions -- 7.2e9 k-mers,
    > 5e9 distinct, nearly all of them error k-mers seen once -- counted in several passes, the rows ordered by the slab-wise MSD sort
    (sort_rows_huge).  Checked on the device: strictly ascending over all rows, sum of abundances == n_kmers, histogram of the rows
    == the histogram, n_kmers == the closed-form number of valid windows."""
    from dsk_amd import KmerCounter, synth
    from tests.full_size import device_invariants
    nr, rl = 60_000_000, 150
    reads = synth.make_reads(synth.make_genome(180_000_000, dev), nr, rl, error_rate=0.04)
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    with KmerCounter(kmer_size=31, abundance_min=1) as kc:
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        kc.count()
        st = kc.stats()
        assert st["n_solid"] == st["n_distinct"] > (1 << 32), st
        assert st["n_retries"] == 0 and st["sort_fallback"] == 0 and st["n_passes"] > 1, st
        inv = device_invariants(kc, st, kc.histogram(), 31, reads, nr, rl, dev, amin=1)
        assert inv["rows_checked"] == st["n_solid"]
    del reads
    torch.cuda.empty_cache()


def test_full_size_group_with_shards_above_4_gb(dev):
    """a rank's read shard may be of any size (the sender's record positions are 64-bit).  Two ranks of one
    in-process group, each holding 30 M x 150 bp = 4.53 GB of reads (> 2^32 bytes: what `dsk -nb-gpus 2|4` sees on configs[2]'s
    200 M-read file, and a rank of the 8-GPU human job: doc/human_log:3-4): the union of the ranks' rows equals the single-GPU count
    of the same 60 M reads row for row, the histograms add up."""
    from dsk_amd import KmerCounter, KmerGroup, synth
    nr, rl = 60_000_000, 150
    reads = synth.make_reads(synth.make_genome(180_000_000, dev), nr, rl)
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    with KmerCounter(kmer_size=31, abundance_min=2) as kc:
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        kc.count()
        st1, h1 = kc.stats(), kc.histogram()
        k1, a1 = _device_rows(kc, dev)
    torch.cuda.empty_cache()
    ranks, per = 2, nr // 2
    assert per * (rl + 1) > (1 << 32)
    with KmerGroup([0] * ranks, kmer_size=31, abundance_min=2, nb_partitions=1) as g:
        for r in range(ranks):
            g.rank(r).set_reads_device(reads.data_ptr() + r * per * (rl + 1), per * (rl + 1))
        g.count()
        sg = g.stats()
        assert (sg["n_kmers"], sg["n_distinct"], sg["n_solid"]) == (st1["n_kmers"], st1["n_distinct"], st1["n_solid"])
        assert (g.histogram() == h1).all()
        got = [g.rank(r).stats()["n_kmers"] for r in range(ranks)]
        assert max(got) <= 1.1 * (sum(got) / ranks)
        assert g.exchanged_words() * 8 < 0.45 * sg["n_kmers"] * 8 / 2 * 1.2          # records, half of them stay on their rank
        rows = [_device_rows(g.rank(r), dev) for r in range(ranks)]
    kk = torch.cat([x[0] for x in rows]); aa = torch.cat([x[1] for x in rows])
    del rows
    order = torch.argsort(kk)
    assert torch.equal(kk[order], k1) and torch.equal(aa[order], a1)


def test_full_size_sender_on_a_human_rank_shard(dev):
    """ONE rank of the 8-GPU human job as a sender -- the 75 M-read shard of the repeat-rich stand-in,
    11.3 GB of reads (2.6 x the old 32-bit limit) -- through dskgpu_mg_sample -> make_table -> dskgpu_mg_scatter; every owner's
    records are then counted by a context of that owner (one GPU after the other).  The k-mers the sender packed per owner add up to
    the valid windows, every owner's count accepts that figure, and the owners' distinct k-mers and histograms add up to the
    single-GPU count of the same shard (owners are disjoint in k-mer space)."""
    from dsk_amd import KmerCounter, synth
    from dsk_amd.engine import make_table
    from dsk_amd.multi import scatter_records
    world = 8
    reads, gl, nr, rl = synth.make_workload("c5_human30x_shard", dev)
    assert reads.numel() > 11_000_000_000
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    with KmerCounter(kmer_size=31, abundance_min=2) as kc:
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        kc.count()
        st1, h1 = kc.stats(), kc.histogram().astype(np.int64)
    torch.cuda.empty_cache()
    with KmerCounter(kmer_size=31, abundance_min=2, world_size=world, rank=0) as snd:
        snd.set_reads_device(reads.data_ptr(), reads.numel())
        table = make_table(snd.mg_sample(), world)               # (one rank's loads stand for the sum: every shard is a uniform sample of the job)
        snd.mg_set_table(table)
        send, counts = scatter_records(snd, None, dev)
        sent = snd.mg_sent_kmers()
        torch.cuda.synchronize()
    assert sum(sent) == st1["n_kmers"] and len(counts) == world and min(counts) > 0
    assert sum(counts) * 8 < 0.45 * st1["n_kmers"] * 8                                  # super-k-mer records: < 45 % of explicit keys' bytes
    assert max(sent) <= 1.25 * (sum(sent) / world), sent                                # the repartition table balances the owners (poly-A included)
    tot_k = tot_d = tot_s = 0
    hist = np.zeros_like(h1)
    off = 0
    for o in range(world):
        with KmerCounter(kmer_size=31, abundance_min=2, world_size=world, rank=o) as rcv:
            rcv.mg_set_table(table)
            rcv.mg_count(send.data_ptr() + off * 8, counts[o], sent[o])             # (a wrong k-mer figure is refused: DSKGPU_E_ARG)
            s = rcv.stats()
            assert s["sort_fallback"] == 0, (o, s)
            tot_k += s["n_kmers"]; tot_d += s["n_distinct"]; tot_s += s["n_solid"]
            hist += rcv.histogram().astype(np.int64)
        off += counts[o]
        torch.cuda.empty_cache()
    assert (tot_k, tot_d, tot_s) == (st1["n_kmers"], st1["n_distinct"], st1["n_solid"])
    assert (hist == h1).all()


def test_full_size_multi_pass(dev):
    """BASELINE.json configs[4] ("multi-pass HBM partitioning"): a full-size input counted in >= 8 passes over the key
    space (forced with max_pass_mkeys on the 25 M-read shard: 3.0e9 k-mers, <= 400 M per pass) must give row for row
    what the single pass gives, and keep every size-independent invariant."""
    from dsk_amd import synth, KmerCounter
    gl, nr, rl = synth.workload("c3_shard_25Mx150")
    reads = synth.make_reads(synth.make_genome(gl, dev), nr, rl)
    res = []
    for mkeys in (0, 400):
        with KmerCounter(kmer_size=31, abundance_min=2, max_pass_mkeys=mkeys) as kc:
            kc.set_reads_device(reads.data_ptr(), reads.numel())
            kc.count()
            res.append((kc.stats(), kc.histogram().astype(np.int64), kc.rows()))
        torch.cuda.empty_cache()
    (st1, h1, (k1, a1)), (st8, h8, (k8, a8)) = res
    assert st1["n_passes"] == 1 and st8["n_passes"] >= 8
    assert (h1 == h8).all() and (k1 == k8).all() and (a1 == a8).all()
    assert st1["n_kmers"] == st8["n_kmers"] and st1["n_distinct"] == st8["n_distinct"]
    full_size_invariants(st8, h8, k8, a8, 31, reads, nr, rl, dev)


@pytest.mark.parametrize("k", [31, 63])
def test_full_size_eight_ranks_on_one_device(dev, k):
    """configs[2] / configs[3] topology, emulated: the 25 M-read shard split over 8 ranks of one in-process group (all on
    device 0, exchange by device copies), super-k-mer records routed by minimizer owner.  The union of the ranks' rows
    must equal the single-GPU count of the same reads row for row; owners stay balanced on uniform data."""
    from dsk_amd import synth, KmerCounter, KmerGroup
    gl, nr, rl = synth.workload("c3_shard_25Mx150")
    reads = synth.make_reads(synth.make_genome(gl, dev), nr, rl)
    with KmerCounter(kmer_size=k, abundance_min=2) as kc:
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        kc.count()
        st1, h1, (k1, a1) = kc.stats(), kc.histogram().astype(np.int64), kc.rows()
    torch.cuda.empty_cache()
    ranks = 8
    per = nr // ranks
    with KmerGroup([0] * ranks, kmer_size=k, abundance_min=2, nb_partitions=1) as g:
        for r in range(ranks):
            lo, hi = r * per * (rl + 1), (nr if r == ranks - 1 else (r + 1) * per) * (rl + 1)
            g.rank(r).set_reads_device(reads.data_ptr() + lo, hi - lo)
        g.count()
        st = g.stats()
        assert st["n_kmers"] == st1["n_kmers"] and st["n_distinct"] == st1["n_distinct"] and st["n_solid"] == st1["n_solid"]
        assert (g.histogram().astype(np.int64) == h1).all()
        got = [g.rank(r).stats()["n_kmers"] for r in range(ranks)]
        assert max(got) <= 1.1 * (sum(got) / ranks)                # hash of the minimizer: uniform reads spread evenly
        assert g.exchanged_words() * 8 < 0.45 * st["n_kmers"] * 8 * (1 if k <= 32 else 2)       # records, not keys: < 45 % of explicit keys' bytes
        parts = [g.partition(p) for p in range(g.num_partitions())]
    kk = np.concatenate([p[0] for p in parts]); aa = np.concatenate([p[1] for p in parts])
    order = np.argsort(kk[:, 0], kind="stable") if k <= 32 else np.lexsort((kk[:, 0], kk[:, 1]))
    assert (kk[order] == k1).all() and (aa[order] == a1).all()


@pytest.mark.parametrize("k,explicit", [(31, False), (31, True), (63, False), (27, True)])
def test_multi_pass_on_the_receive_side(oracle, dev, k, explicit):
    """Several passes over the key space with the keys coming from an ARRAY or from super-k-mer RECORDS (multi-GPU receive side
    with max_pass_mkeys forcing npass > 1): level 1 is then the aligned scatter with the pass filter (k_scatter_al, MODE 3), where
    every tile has the keys of the other passes as masked slots (their ranks once accumulated over the tiles of a chunk)."""
    from dsk_amd import KmerCounter, synth
    world = 2
    reads = synth.make_reads(synth.make_genome(300_000, dev), 60_000, 150).cpu().numpy()
    recs = bytes(reads).split(b"\n")
    ctxs, sends, counts, shards = [], [], [], []
    for r in range(world):
        shard = torch.from_numpy(np.frombuffer(b"\n".join(recs[r::world]) + b"\n", dtype=np.uint8).copy()).to(dev)
        kc = KmerCounter(kmer_size=k, abundance_min=2, world_size=world, rank=r, mg_explicit=explicit, max_pass_mkeys=1)
        kc.set_reads_device(shard.data_ptr(), shard.numel())
        send = torch.zeros(kc.mg_send_capacity_words(), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        counts.append(kc.mg_scatter(send.data_ptr(), send.numel()))
        ctxs.append(kc); sends.append(send); shards.append(shard)
    rows_k, rows_a, hist = [], [], np.zeros(10001, np.uint64)
    for d in range(world):
        recv = torch.cat([sends[src][sum(counts[src][:d]): sum(counts[src][:d]) + counts[src][d]] for src in range(world)])
        torch.cuda.synchronize()
        ctxs[d].mg_count(recv.data_ptr(), recv.numel())
        assert ctxs[d].stats()["n_passes"] >= 2
        kk, aa = ctxs[d].rows()
        rows_k.append(kk); rows_a.append(aa); hist += ctxs[d].histogram()
    kk = np.concatenate(rows_k); aa = np.concatenate(rows_a)
    ref = oracle.count(reads, k)
    assert (hist == ref.histogram(10000)).all()
    keep = ref.ab >= 2
    order = np.argsort(kk[:, 0]) if k <= 32 else np.lexsort((kk[:, 0], kk[:, 1]))
    assert (kk[order] == ref.words()[keep]).all() and (aa[order] == ref.ab[keep]).all()
    assert sum(c.stats()["n_kmers"] for c in ctxs) == ref.total
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("k,explicit", [(31, False), (31, True), (63, False)])
def test_receive_side_multi_pass_on_the_fast_path(oracle, dev, k, explicit):
    """The receive side of a multi-GPU job whose share of the k-mer space needs several passes (30x human on 8 GPUs: 9e9 k-mers per
    rank), with repeat-rich reads: every pass runs the histogram-free level 1 with the pass filter straight from the RECORDS
    (k_scatter<W, 2, 3>; from the key array for explicit keys), slices sized from the sample, heavy k-mers counted apart, region
    chains at level 2 -- no histogram pass, no retry, rows equal to the oracle's."""
    from dsk_amd import KmerCounter, synth
    world = 2
    reads, gl, nr, rl = synth.make_workload("small_repeats", dev)
    host = reads.cpu().numpy()
    per = nr // world
    ctxs, sends, counts, shards = [], [], [], []
    for r in range(world):
        lo, hi = r * per * (rl + 1), (nr if r == world - 1 else (r + 1) * per) * (rl + 1)
        shard = reads[lo:hi].clone()
        kc = KmerCounter(kmer_size=k, abundance_min=2, world_size=world, rank=r, mg_explicit=explicit, max_pass_mkeys=5, timing=True)
        kc.set_reads_device(shard.data_ptr(), shard.numel())
        send = torch.zeros(kc.mg_send_capacity_words(), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        counts.append(kc.mg_scatter(send.data_ptr(), send.numel()))
        ctxs.append(kc); sends.append(send); shards.append(shard)
    rows_k, rows_a, hist = [], [], np.zeros(10001, np.uint64)
    for d in range(world):
        recv = torch.cat([sends[src][sum(counts[src][:d]): sum(counts[src][:d]) + counts[src][d]] for src in range(world)])
        torch.cuda.synchronize()
        ctxs[d].mg_count(recv.data_ptr(), recv.numel())
        st, stages = ctxs[d].stats(), dict(ctxs[d].stage_times())
        assert st["n_passes"] >= 3 and st["n_levels"] == 2, st
        assert st["n_retries"] == 0 and "hist1" not in stages and "hist2" not in stages, (st, stages)
        kk, aa = ctxs[d].rows()
        rows_k.append(kk); rows_a.append(aa); hist += ctxs[d].histogram()
    assert sum(c.stats()["n_ext_regions"] for c in ctxs) > 0
    kk = np.concatenate(rows_k); aa = np.concatenate(rows_a)
    ref = oracle.count(host, k)
    assert (hist == ref.histogram(10000)).all()
    keep = ref.ab >= 2
    order = np.argsort(kk[:, 0]) if k <= 32 else np.lexsort((kk[:, 0], kk[:, 1]))
    assert (kk[order] == ref.words()[keep]).all() and (aa[order] == ref.ab[keep]).all()
    assert sum(c.stats()["n_kmers"] for c in ctxs) == ref.total
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("world,k,explicit", [(2, 31, False), (4, 27, False), (2, 63, False), (8, 20, False), (4, 46, False), (2, 64, False),
                                              (2, 32, False), (2, 31, True), (2, 63, True), (4, 15, False)])
def test_multi_gpu_path_on_one_device(oracle, golden_dir, dev, world, k, explicit):
    """dskgpu_mg_scatter / dskgpu_mg_count with the exchange done by hand: `world` contexts on the
    same GPU, each fed its shard of the reads; the union of their results must equal the oracle."""
    s, _ = oracle.load_bank(os.path.join(golden_dir, "read50x_ref10K_e001.fasta.gz"))
    multi_gpu_path_case(oracle, s, dev, world, k, explicit)


def multi_gpu_path_case(oracle, s, dev, world, k, explicit):
    """the body of test_multi_gpu_path_on_one_device on the stream s -> per rank (the bytes of its shard, the 64-bit words it received)"""
    from dsk_amd import KmerCounter, DskGpuError
    recs = bytes(s).split(b"\n")
    W = 1 if k <= 32 else 2
    ctxs, sends, counts, shards, kmers, sizes = [], [], [], [], [], []
    for r in range(world):
        shard = torch.from_numpy(np.frombuffer(b"\n".join(recs[r::world]) + b"\n", dtype=np.uint8).copy()).to(dev)
        kc = KmerCounter(kmer_size=k, abundance_min=1, world_size=world, rank=r, mg_explicit=explicit)
        kc.set_reads_device(shard.data_ptr(), shard.numel())
        send = torch.zeros(kc.mg_send_capacity_words(), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()      # the contexts run on their own streams
        c = kc.mg_scatter(send.data_ptr(), send.numel())
        records = not explicit and k >= 20          # super-k-mer records of 2 (k <= 45) or 3 words
        assert all(x % ((2 if k <= 45 else 3) if records else W) == 0 for x in c)
        if records:   # a record carries up to 16 k-mers: far fewer words than one key per k-mer
            assert sum(c) < 0.6 * W * (shard.numel() - len(recs[r::world]) * k)
        ctxs.append(kc); sends.append(send); counts.append(c); shards.append(shard); kmers.append(kc.mg_sent_kmers())
    rows_k, rows_a, hist = [], [], np.zeros(10001, np.uint64)
    for d in range(world):
        parts = []
        for src in range(world):
            off = sum(counts[src][:d])
            parts.append(sends[src][off: off + counts[src][d]])
        recv = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        # the senders' k-mer totals size the receiver (dskgpu_mg_count_sized); a figure that does not match the records is an
        # error, never a wrong result -- one too many (found at the end), half (found when the sized slices overflow)
        hint = sum(kmers[src][d] for src in range(world))
        assert hint > 0
        for wrong in ((hint + 1,) if d == 0 else (hint // 2,) if d == 1 else ()):
            with pytest.raises(DskGpuError):
                ctxs[d].mg_count(recv.data_ptr(), recv.numel(), wrong)
        ctxs[d].mg_count(recv.data_ptr(), recv.numel(), hint if d % 2 == 0 else 0)
        sizes.append((shards[d].numel(), recv.numel()))
        kk, aa = ctxs[d].rows()
        rows_k.append(kk); rows_a.append(aa); hist += ctxs[d].histogram()
    kk = np.concatenate(rows_k); aa = np.concatenate(rows_a)
    ref = oracle.count(s, k)
    assert (hist == ref.histogram(10000)).all()
    if W == 1:
        order = np.argsort(kk[:, 0])
        assert (kk[order, 0] == ref.lo).all() and (aa[order] == ref.ab).all()
    else:
        order = np.lexsort((kk[:, 0], kk[:, 1]))
        assert (kk[order, 0] == ref.lo).all() and (kk[order, 1] == ref.hi).all() and (aa[order] == ref.ab).all()
    assert sum(c.stats()["n_kmers"] for c in ctxs) == ref.total
    for c in ctxs:
        c.close()
    return sizes


@pytest.mark.parametrize("world,k,est_scale", [(4, 31, 1.0), (2, 63, 1.0), (4, 31, 0.5), (2, 31, 3.0)])
def test_step_in_slices_on_one_device(oracle, dev, monkeypatch, world, k, est_scale):
    """The sliced step (dskgpu_mg_slices_prepare / _scatter_slice / _count_sliced / _slices_finish) with the exchange done by hand:
    every sender writes its records in 4 slices (slice-major, owner-major inside), every receiver gets the slices one after the
    other and partitions them with one level-1 launch per slice behind its gate -- gates called in order, each once.  The k-mer
    total that sizes the receiver is an ESTIMATE: halved (the sized slices overflow: the receiver re-plans with the real figure)
    or tripled it must not change the result.  Same rows and histogram as the oracle, and as the one-piece step."""
    from dsk_amd import KmerCounter, synth
    monkeypatch.setenv("DSKGPU_SK_MINSLICE", "1")              # the sampled send layout on a test-sized input
    S = 4
    reads = synth.make_reads(synth.make_genome(2_000_000, dev), 600_000, 150)
    n_reads = 600_000
    per = n_reads // world
    ctxs, sends, words, ests = [], [], [], []
    for r in range(world):
        shard = reads[r * per * 151: (r + 1) * per * 151].clone()
        kc = KmerCounter(kmer_size=k, abundance_min=2, world_size=world, rank=r)
        kc.set_reads_device(shard.data_ptr(), shard.numel())
        ns, w, est = kc.mg_slices_prepare(S)
        assert ns == S and len(w) == S and all(len(x) == world for x in w)
        cap = kc.mg_send_capacity_words()
        assert sum(sum(x) for x in w) + 1 == cap              # the slices tile the send buffer
        send = torch.zeros(cap, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        for sl in range(S):
            kc.mg_scatter_slice(send.data_ptr(), send.numel(), sl)
        ctxs.append((kc, shard)); sends.append(send); words.append(w); ests.append(est)
    torch.cuda.synchronize()
    rows_k, rows_a, hist, nk = [], [], np.zeros(10001, np.uint64), 0
    for d in range(world):
        parts, slice_words = [], []
        for sl in range(S):
            tot = 0
            for src in range(world):
                off = sum(sum(words[src][x]) for x in range(sl)) + sum(words[src][sl][:d])
                parts.append(sends[src][off: off + words[src][sl][d]])
                tot += words[src][sl][d]
            slice_words.append(tot)
        recv = torch.cat(parts)
        torch.cuda.synchronize()
        gates = []
        est = int(sum(ests[src][d] for src in range(world)) * est_scale)
        ctxs[d][0].mg_count_sliced(recv.data_ptr(), slice_words, est, gates.append)
        assert gates == list(range(S))
        kk, aa = ctxs[d][0].rows()
        rows_k.append(kk); rows_a.append(aa); hist += ctxs[d][0].histogram(); nk += ctxs[d][0].stats()["n_kmers"]
        if est_scale == 1.0:                                   # the estimate is good to a few per cent, and the fast path was taken
            real = ctxs[d][0].stats()["n_kmers"]
            assert abs(est - real) < 0.03 * real and ctxs[d][0].stats()["n_retries"] == 0
            assert ctxs[d][0].stats()["n_levels"] == 2          # (two levels: the level-1 scatter ran once per slice, from the records)
    for kc, _ in ctxs:
        assert kc.mg_slices_finish() is False
    ref = oracle.count(reads.cpu().numpy(), k)
    assert nk == ref.total and (hist == ref.histogram(10000)).all()
    kk = np.concatenate(rows_k); aa = np.concatenate(rows_a)
    keep = ref.ab >= 2
    if k <= 32:
        order = np.argsort(kk[:, 0])
        assert (kk[order, 0] == ref.lo[keep]).all() and (aa[order] == ref.ab[keep]).all()
    else:
        order = np.lexsort((kk[:, 0], kk[:, 1]))
        assert (kk[order, 0] == ref.lo[keep]).all() and (kk[order, 1] == ref.hi[keep]).all() and (aa[order] == ref.ab[keep]).all()
    for kc, _ in ctxs:
        kc.close()


def _fmix32(h):
    h = h.astype(np.uint64)
    h ^= h >> np.uint64(16); h = (h * np.uint64(0x85ebca6b)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13); h = (h * np.uint64(0xc2b2ae35)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    return h


@pytest.mark.parametrize("world,k,sliced", [(4, 31, False), (2, 63, False), (8, 27, False), (4, 31, True)])
def test_super_kmer_record_invariants(oracle, golden_dir, dev, monkeypatch, world, k, sliced):
    """The wire format of the multi-GPU exchange, decoded on the host (superkmer.h; DSK v2's super-k-mers, CHANGELOG.md:13):
    every record holds 1..min(32, (64 R - 8) / 2 + 1 - k) k-mers as n + k - 1 packed bases; every k-mer of a record maps to the record's owner under an
    independent numpy restatement of the owner map (owner = hash of the window's minimizer, m-mers ordered by a 32-bit hash
    of their canonical value); zero-length records exist only as slice padding; the multiset of the canonical k-mers of all
    records of all ranks equals the oracle's enumeration of the input."""
    from dsk_amd import KmerCounter
    from dsk_amd.multi import scatter_records
    if sliced:
        monkeypatch.setenv("DSKGPU_SK_MINSLICE", "1")           # the sampled slice layout on a small input
    else:
        monkeypatch.setenv("DSKGPU_SK_EXACT", "1")
    s, _ = oracle.load_bank(os.path.join(golden_dir, "read50x_ref10K_e001.fasta.gz"))
    if sliced:                                                   # slices need >= 8 tiles per chunk: a longer stream
        s = np.concatenate([s] * 12)
    recs = bytes(s).split(b"\n")
    m = min(10, 16, k - 15)
    R = (2 * (k + 15) + 8 + 63) // 64
    nb = 32 * R
    got = []
    for r in range(world):
        shard = torch.from_numpy(np.frombuffer(b"\n".join(recs[r::world]) + b"\n", dtype=np.uint8).copy()).to(dev)
        with KmerCounter(kmer_size=k, abundance_min=1, world_size=world, rank=r) as kc:
            kc.set_reads_device(shard.data_ptr(), shard.numel())
            torch.cuda.synchronize()
            send, counts = scatter_records(kc, None, dev)
            torch.cuda.synchronize()
            words = send[: sum(counts)].cpu().numpy().view(np.uint64).reshape(-1, R)
        dest = np.repeat(np.arange(world), [c // R for c in counts])
        n = (words[:, R - 1] & np.uint64(0xFF)).astype(np.int64)
        nmax = min(32, (64 * R - 8) // 2 + 1 - k)                 # the bases of n k-mers + the header fit the record; never more than one packed word's 32 windows
        assert n.max() <= nmax and n.max() > 16                   # (r06: the two halves of a word join their runs)
        if not sliced:
            assert n.min() >= 1                                  # the exact layout has no padding
        keep = n > 0
        words, dest, n = words[keep], dest[keep], n[keep]
        # bases[:, i] = 2-bit code of base i of the record (first base in the top bits of word 0)
        shifts = np.uint64(62) - np.uint64(2) * np.arange(32, dtype=np.uint64)
        bases = np.concatenate([((words[:, w:w + 1] >> shifts[None, :]) & np.uint64(3)) for w in range(R)], axis=1).astype(np.int64)
        # canonical m-mer hash at every position of the record (m-mer starting at base i)
        npos = nb - m + 1
        fw = np.zeros((len(n), npos), dtype=np.uint64); rv = np.zeros_like(fw)
        for i in range(m):
            fw = (fw << np.uint64(2)) | bases[:, i:i + npos].astype(np.uint64)
            rv = rv | ((bases[:, i:i + npos].astype(np.uint64) ^ np.uint64(2)) << np.uint64(2 * i))
        hm = _fmix32(np.minimum(fw, rv))
        wlen = k - m + 1
        for j in range(32):                                      # k-mer j of every record that has one
            rows = np.nonzero(n > j)[0]
            if len(rows) == 0:
                break
            mn = hm[rows, j:j + wlen].min(axis=1)
            owner = ((mn & np.uint64(0xFFFF)) * np.uint64(world)) >> np.uint64(16)
            assert (owner.astype(np.int64) == dest[rows]).all(), (r, j)
            if k <= 32:
                f = np.zeros(len(rows), dtype=np.uint64); rc = np.zeros(len(rows), dtype=np.uint64)
                for i in range(k):
                    b = bases[rows, j + i].astype(np.uint64)
                    f = (f << np.uint64(2)) | b
                    rc = rc | ((b ^ np.uint64(2)) << np.uint64(2 * i))
                got.append(np.minimum(f, rc))
        # a record is cut where the owner changes, at an invalid base, at the border of a packed word (32 windows) or where it is full
    if k <= 32:
        lo, hi, valid = oracle.enumerate(s, k)
        want = np.sort(lo[valid.astype(bool)])
        have = np.sort(np.concatenate(got))
        assert len(have) == len(want) and (have == want).all()


@pytest.mark.parametrize("k,world", [(31, 8), (63, 4), (31, 64)])
def test_sender_with_compile_time_k_writes_the_same_records(dev, monkeypatch, k, world):
    """Round 6: for the BASELINE configs (k = 31 / 63, m = 10) the sender kernels know k and m at compile time (superkmer.h:
    sk_tile_fx -- immediate shifts, 128-bit LDS reads, one running minimum); DSKGPU_SK_GENERIC selects the run-time form.  Both must
    write the same records for every owner, byte for byte: default table and a balanced table with split buckets (noisy
    poly-A reads), exact and sampled layouts, and the sampled bucket loads must agree too."""
    from dsk_amd import KmerCounter, synth, make_table
    from dsk_amd.multi import scatter_records
    rng = np.random.default_rng(11)
    normal = synth.make_reads(synth.make_genome(300_000, dev), 150_000, 150).cpu().numpy().reshape(-1, 151)
    polya = np.full((30_000, 151), ord("A"), dtype=np.uint8); polya[:, 150] = 10
    noise = rng.random((30_000, 150)) < 0.05
    polya[:, :150][noise] = rng.choice(np.frombuffer(b"CGTN", dtype=np.uint8), int(noise.sum()))
    reads = np.concatenate([normal, polya]); rng.shuffle(reads)
    t = torch.from_numpy(reads.reshape(-1).copy()).to(dev)

    def run(generic, table, exact):
        if generic:
            monkeypatch.setenv("DSKGPU_SK_GENERIC", "1")
        else:
            monkeypatch.delenv("DSKGPU_SK_GENERIC", raising=False)
        if exact:
            monkeypatch.setenv("DSKGPU_SK_EXACT", "1"); monkeypatch.delenv("DSKGPU_SK_MINSLICE", raising=False)
        else:
            monkeypatch.setenv("DSKGPU_SK_MINSLICE", "1"); monkeypatch.delenv("DSKGPU_SK_EXACT", raising=False)
        with KmerCounter(kmer_size=k, abundance_min=1, world_size=world, rank=0) as kc:
            kc.set_reads_device(t.data_ptr(), t.numel())
            loads = kc.mg_sample()
            if table is not None:
                kc.mg_set_table(table)
            send, counts = scatter_records(kc, None, dev)
            torch.cuda.synchronize()
            return loads, counts, send[: sum(counts)].cpu().numpy().copy(), kc.mg_sent_kmers()

    loads, _, _, _ = run(False, None, True)
    table = make_table(loads, world)
    assert (table == 255).sum() >= 1                       # the poly-A bucket is split: the by-k-mer route is exercised
    for tab in (None, table):
        for exact in (True, False):
            la, ca, sa, ka = run(False, tab, exact)
            lb, cb, sb, kb = run(True, tab, exact)
            assert (la == lb).all() and ka == kb and (ca == cb or not exact), (k, world, exact)
            assert sum(ka) > 0
            # the same records for every owner -- as a multiset: the two forms cut the stream into different chunks (three blocks per
            # CU against two), a chunk's records are dealt to slots by LDS atomics, and the sampled layout pads its slices
            R = (2 * (k + 15) + 8 + 63) // 64
            ea, eb = np.cumsum([0] + ca), np.cumsum([0] + cb)
            for o in range(world):
                ra = sa[ea[o]: ea[o + 1]].view(np.uint64).reshape(-1, R); rb = sb[eb[o]: eb[o + 1]].view(np.uint64).reshape(-1, R)
                ra = ra[(ra[:, R - 1] & np.uint64(0xFF)) != 0]; rb = rb[(rb[:, R - 1] & np.uint64(0xFF)) != 0]
                assert len(ra) == len(rb), (k, world, exact, o)
                ia = np.lexsort(ra.T[::-1]); ib = np.lexsort(rb.T[::-1])
                assert (ra[ia] == rb[ib]).all(), (k, world, exact, o, "records differ")


def test_sender_slices_and_their_exact_fallback(oracle, dev, monkeypatch):
    """Multi-GPU sender: the records go to (owner, chunk) slices sized from a sampled count and padded with zero-length
    records; a slice that overflows switches the context to exact counts (which may need a larger send buffer)."""
    from dsk_amd import KmerCounter, synth
    from dsk_amd.multi import scatter_records
    world, k = 4, 31
    reads = synth.make_reads(synth.make_genome(400_000, dev), 600_000, 150)
    monkeypatch.setenv("DSKGPU_SK_MINSLICE", "100")        # (the slice layout is meant for shards of >= 3e8 bases: let it run on this small one)
    ref = oracle.count(reads.cpu().numpy(), k)

    def run():
        ctxs, sends, counts, words = [], [], [], 0
        for r in range(world):
            kc = KmerCounter(kmer_size=k, abundance_min=1, world_size=world, rank=r, timing=True)
            shard = reads[(reads.numel() // 151 // world) * 151 * r: (reads.numel() // 151 // world) * 151 * (r + 1)]
            kc.set_reads_device(shard.data_ptr(), shard.numel())
            torch.cuda.synchronize()
            send, c = scatter_records(kc, None, dev)
            ctxs.append(kc); sends.append(send); counts.append(c); words += sum(c)
        tot, hist = 0, np.zeros(10001, np.uint64)
        for d in range(world):
            recv = torch.cat([sends[s_][sum(counts[s_][:d]): sum(counts[s_][:d]) + counts[s_][d]] for s_ in range(world)])
            torch.cuda.synchronize()
            ctxs[d].mg_count(recv.data_ptr(), recv.numel())
            tot += ctxs[d].stats()["n_kmers"]; hist += ctxs[d].histogram()
        for c in ctxs:
            c.close()
        return tot, hist, words, counts

    tot, hist, words, counts = run()
    assert tot == ref.total and (hist == ref.histogram(10000)).all()
    assert len({tuple(c) for c in counts}) >= 1 and all(len(set(c)) == 1 for c in counts)      # slice layout: equal regions per owner
    monkeypatch.setenv("DSKGPU_SK_SLICE", "8")                                                  # slices far too small -> exact counts
    tot2, hist2, words2, counts2 = run()
    assert tot2 == ref.total and (hist2 == ref.histogram(10000)).all()
    assert any(len(set(c)) > 1 for c in counts2) and words2 < words                            # exact layout: no padding


@pytest.mark.parametrize("k,m", [(31, 10), (21, 8), (63, 10), (11, 4), (16, 16), (5, 1)])
def test_minimizers_match_oracle(oracle, golden_dir, dev, k, m):
    from dsk_amd import KmerCounter
    s, _ = oracle.load_bank(os.path.join(golden_dir, "longread.fasta"))
    s = np.concatenate([s[:20000], np.frombuffer(b"ACGTNNNNacgtacgtACGTRYKMAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA" * 3, dtype=np.uint8)])
    t = torch.from_numpy(s.copy()).to(dev)
    mm = torch.zeros(len(s), dtype=torch.int32, device=dev)
    val = torch.zeros(len(s), dtype=torch.uint8, device=dev)
    with KmerCounter(kmer_size=k, minimizer_size=m) as kc:
        kc.k_minimizers(t.data_ptr(), len(s), mm.data_ptr(), val.data_ptr())
    ref_m, ref_v = oracle.minimizers(s, k, m)
    assert (val.cpu().numpy() == ref_v).all()
    assert (mm.cpu().numpy().view(np.uint32) == ref_m).all()


def test_row_sort_fallback_on_shared_prefixes(oracle, dev):
    """The hand-written row sort (csrc/rowsort.h) places rows by the top 26 value bits (three radix digits) and orders the rows of
    a cell by comparison; more than 64 rows sharing those 13 bases (here: 300 rows sharing 20) go to a block, which orders a
    sub-bucket with such a cell by a bitonic network in LDS -- no full-width fallback; short cells stay on the wave path."""
    from dsk_amd import KmerCounter
    rng = np.random.default_rng(11)
    tails = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(300, 11))
    recs = [b"AAAAAAAAAAAAAAAAAAAC" + t.tobytes() for t in tails]          # 300 31-mers with one 20-base prefix
    noise = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=50_000).tobytes()
    s = np.frombuffer(b"\n".join(recs) + b"\n" + noise + b"\n", dtype=np.uint8)
    t = torch.from_numpy(s.copy()).to(dev)
    with KmerCounter(kmer_size=31, abundance_min=1) as kc:
        kc.set_reads_device(t.data_ptr(), t.numel())
        kc.count()
        kmers, ab = kc.rows()
        st = kc.stats()
    lo, hi, rab = oracle.count(s, 31).solid(1)
    assert st["sort_fallback"] == 0
    assert (kmers[:, 0] == lo).all() and (ab == rab).all()
    # short runs (<= 32 rows per prefix) are fixed in place, no fallback
    recs = [b"AAAAAAAAAAAAAAAAAAAC" + t.tobytes() for t in tails[:20]] + [b"CCCCCCCCCCCCCCCCCCCA" + t.tobytes() for t in tails[:25]]
    s = np.frombuffer(b"\n".join(recs) + b"\n" + noise + b"\n", dtype=np.uint8)
    st = check_against_oracle(oracle, s, 31, dev, amin=1)
    assert st["sort_fallback"] == 0


def test_row_sort_paths_agree(oracle, dev, monkeypatch):
    """One-word rows: the hand-written MSD sort, its large-sub-bucket fallback (forced: no sub-bucket above 512 rows is ordered
    by a block) give the same rows, at k = 31 and at
    small k (fewer than 26 value bits: the lower digits are empty)."""
    from dsk_amd import synth
    g = synth.make_genome(200_000, dev)
    reads = synth.make_reads(g, 60_000, 150).cpu().numpy()
    # skewed values: a third of the stream is poly-A with sparse errors -> thousands of distinct k-mers under one 20-bit prefix
    rng = np.random.default_rng(5)
    pa = np.full(1_500_000, 65, np.uint8)
    hit = rng.random(pa.size) < 0.02
    pa[hit] = rng.choice(np.frombuffer(b"CGT", dtype=np.uint8), size=int(hit.sum()))
    skew = np.concatenate([pa, np.array([10], np.uint8), reads]).astype(np.uint8)
    for k, s in ((31, reads), (11, reads), (4, reads)):
        st = check_against_oracle(oracle, s, k, dev, amin=1)
        assert st["sort_fallback"] == 0
    st = check_against_oracle(oracle, skew, 31, dev, amin=1)
    assert st["sort_fallback"] == 0                                    # sub-buckets above 4096 rows go round again on their remaining bits
    monkeypatch.setenv("DSKGPU_RS_BLOCK_ROWS", "512")                   # ... forced: every sub-bucket above 512 rows does
    st = check_against_oracle(oracle, skew, 31, dev, amin=1)
    assert st["sort_fallback"] == 0
    monkeypatch.delenv("DSKGPU_RS_BLOCK_ROWS")
    monkeypatch.setenv("DSKGPU_RS_HEAVY", "1000")                       # a first-digit bucket "too heavy" for one block: fallback, same rows
    st = check_against_oracle(oracle, reads, 31, dev, amin=1)
    assert st["sort_fallback"] == 1
    monkeypatch.delenv("DSKGPU_RS_HEAVY")
    for bbits in ("9", "10"):                                           # the wider second digits of row sets above 96 M / 192 M rows
        monkeypatch.setenv("DSKGPU_RS_BBITS", bbits)
        for k, s in ((31, reads), (31, skew), (11, reads)):
            check_against_oracle(oracle, s, k, dev, amin=1)
    monkeypatch.delenv("DSKGPU_RS_BBITS")
    # r05: the sort's first step reads the rows where the count kernel left them (default above) -- the same rows through both region
    # layouts (fixed-capacity regions and, with DSKGPU_NO_OPT2, exact offsets), with k-mers counted apart (the dense tail) and with the
    # full-width fallback; the dense copy first (k_compact) is what several passes do (test_multi_pass_*)
    for env in ({"DSKGPU_NO_OPT2": "1"}, {"DSKGPU_RS_HEAVY": "1000"}):
        for name, val in env.items():
            monkeypatch.setenv(name, val)
        for k, s in ((31, reads), (31, skew), (11, reads)):
            check_against_oracle(oracle, s, k, dev, amin=1)
        for name in env:
            monkeypatch.delenv(name)


def test_two_word_row_sort_paths_agree(oracle, dev, monkeypatch):
    """Two-word rows (k = 33..64) go through their own MSD sort as whole rows (rowsort2.h): uniform and skewed values, few value
    bits above the first word (k = 33, 35), sub-buckets that go round again (natural: poly-A variants; forced: every sub-bucket above
    512 rows), the full-width fallback behind a 'heavy' first-digit bucket, the wider second digits -- all the same rows as the oracle."""
    from dsk_amd import synth
    g = synth.make_genome(200_000, dev)
    reads = synth.make_reads(g, 60_000, 150).cpu().numpy()
    rng = np.random.default_rng(5)
    pa = np.full(600_000, 65, np.uint8)
    hit = rng.random(pa.size) < 0.01
    pa[hit] = rng.choice(np.frombuffer(b"CGT", dtype=np.uint8), size=int(hit.sum()))
    skew = np.concatenate([pa, np.array([10], np.uint8), reads]).astype(np.uint8)
    for k, s in ((63, reads), (64, reads), (33, reads), (35, reads), (47, skew)):
        st = check_against_oracle(oracle, s, k, dev, amin=1)
        assert st["sort_fallback"] == 0, (k, st)
    st = check_against_oracle(oracle, skew, 63, dev, amin=1)
    assert st["sort_fallback"] == 0                                    # sub-buckets above 4096 rows go round again on their remaining bits
    monkeypatch.setenv("DSKGPU_RS_BLOCK_ROWS", "512")                   # ... forced: every sub-bucket above 512 rows does
    for k, s in ((63, skew), (35, reads)):
        st = check_against_oracle(oracle, s, k, dev, amin=1)
        assert st["sort_fallback"] == 0, (k, st)
    monkeypatch.delenv("DSKGPU_RS_BLOCK_ROWS")
    monkeypatch.setenv("DSKGPU_RS_HEAVY", "1000")                       # a first-digit bucket "too heavy" for one block: fallback, same rows
    st = check_against_oracle(oracle, reads, 63, dev, amin=1)
    assert st["sort_fallback"] == 1
    monkeypatch.delenv("DSKGPU_RS_HEAVY")
    for bbits in ("9", "10"):
        monkeypatch.setenv("DSKGPU_RS_BBITS", bbits)
        for k, s in ((63, reads), (63, skew), (35, reads)):
            check_against_oracle(oracle, s, k, dev, amin=1)
    monkeypatch.delenv("DSKGPU_RS_BBITS")
    # r05: step A of the two-word sort reads the rows where the count kernel left them, like the one-word sort (default above) -- the
    # same rows through both region layouts (fixed-capacity regions and, with DSKGPU_NO_OPT2, exact offsets), with k-mers counted apart
    # (the skewed input: the dense tail) and with the full-width fallback
    for env in ({"DSKGPU_NO_OPT2": "1"}, {"DSKGPU_RS_HEAVY": "1000"}):
        for name, val in env.items():
            monkeypatch.setenv(name, val)
        for k, s in ((63, reads), (63, skew), (35, reads), (47, skew)):
            check_against_oracle(oracle, s, k, dev, amin=1)
        for name in env:
            monkeypatch.delenv(name)


def test_row_sort_of_huge_row_sets_in_groups(oracle, dev, monkeypatch):
    """Row sets above what the MSD sort takes in one piece (3 * 10^9 solid k-mers of a 30x human run) are split on their top bits
    once and ordered group by group (sort_rows_big): forced here on a small input with DSKGPU_RS_MAX_ROWS -- single pass (scratch
    = srt_*), several passes (scratch inside the level-0 buffer), few value bits, skewed values, and the full-width fallback when
    one top-10-bit bucket alone exceeds the limit."""
    from dsk_amd import synth
    g = synth.make_genome(400_000, dev)
    reads = synth.make_reads(g, 120_000, 150).cpu().numpy()
    rng = np.random.default_rng(7)
    pa = np.full(1_000_000, 65, np.uint8)
    hit = rng.random(pa.size) < 0.02
    pa[hit] = rng.choice(np.frombuffer(b"CGT", dtype=np.uint8), size=int(hit.sum()))
    skew = np.concatenate([pa, np.array([10], np.uint8), reads]).astype(np.uint8)
    monkeypatch.setenv("DSKGPU_RS_MAX_ROWS", "300000")
    for k, s in ((31, reads), (31, skew), (13, reads)):
        st = check_against_oracle(oracle, s, k, dev, amin=1)
        assert st["n_solid"] > 300000 and st["sort_fallback"] == 0, (k, st)
    st = check_against_oracle(oracle, reads, 31, dev, amin=1, max_pass_mkeys=2)         # several passes: rows accumulated, scratch carved from l0buf
    assert st["n_passes"] > 4 and st["n_read_sweeps"] < st["n_passes"] and st["sort_fallback"] == 0
    for k, s in ((63, reads), (35, reads)):                                            # two-word rows: sort_rows2_big (rowsort2.h kernels, the same scheme)
        st = check_against_oracle(oracle, s, k, dev, amin=1)
        assert st["n_solid"] > 300000 and st["sort_fallback"] == 0, (k, st)
    st = check_against_oracle(oracle, skew, 63, dev, amin=1)                           # (at k = 63 nearly every poly-A window is its own k-mer: 900 000 rows
    assert st["n_solid"] > 300000                                                      #  start with AAAAA -- one 10-bit bucket above the limit: the fallback)
    st = check_against_oracle(oracle, reads, 63, dev, amin=1, max_pass_mkeys=2)
    assert st["n_passes"] > 4 and st["sort_fallback"] == 0
    monkeypatch.setenv("DSKGPU_RS_MAX_ROWS", "5000")                                   # a 10-bit bucket of uniform rows holds ~14 000: the fallback orders them
    st = check_against_oracle(oracle, reads, 31, dev, amin=1)
    assert st["sort_fallback"] == 1
    st = check_against_oracle(oracle, reads, 63, dev, amin=1)                          # (two-word rows: the scratch copy goes back to out_* first)
    assert st["sort_fallback"] == 1


def test_row_sort_of_2_pow_32_rows_and_more_slab_by_slab(oracle, dev, monkeypatch):
    """Row sets of >= 2^32 rows (sort_rows_huge: `-abundance-min 1` on a 200 M-read input; the reference streams rows to
    Partition<Count> without a bound, utils/dsk2ascii.cpp:61,77): step A runs slab by slab with 64-bit bucket offsets, then group by
    group.  Forced here on a small input with DSKGPU_RS_SLAB_ROWS (slabs of 100 000 rows: 8-20 of them) -- one- and two-word rows,
    a single pass and several, few value bits, skewed values (a group that takes the per-group library sort), and together with
    small groups (DSKGPU_RS_MAX_ROWS).  The full-size case is test_full_size_more_than_2_pow_32_rows."""
    from dsk_amd import synth
    g = synth.make_genome(400_000, dev)
    reads = synth.make_reads(g, 120_000, 150).cpu().numpy()
    rng = np.random.default_rng(7)
    pa = np.full(1_000_000, 65, np.uint8)
    hit = rng.random(pa.size) < 0.02
    pa[hit] = rng.choice(np.frombuffer(b"CGT", dtype=np.uint8), size=int(hit.sum()))
    skew = np.concatenate([pa, np.array([10], np.uint8), reads]).astype(np.uint8)
    monkeypatch.setenv("DSKGPU_RS_SLAB_ROWS", "100000")
    for k, s in ((31, reads), (13, reads), (63, reads), (35, reads), (31, skew)):
        st = check_against_oracle(oracle, s, k, dev, amin=1)
        assert st["n_solid"] > 300000 and st["sort_fallback"] == 0, (k, st)
    st = check_against_oracle(oracle, reads, 31, dev, amin=1, max_pass_mkeys=2)         # several passes: rows accumulated, scratch carved from l0buf
    assert st["n_passes"] > 4 and st["sort_fallback"] == 0
    monkeypatch.setenv("DSKGPU_RS_MAX_ROWS", "300000")                                  # groups of <= 300 000 rows
    for k, s in ((31, reads), (63, reads)):
        st = check_against_oracle(oracle, s, k, dev, amin=1)
        assert st["sort_fallback"] == 0, (k, st)
    monkeypatch.setenv("DSKGPU_RS_MAX_ROWS", "100000")
    st = check_against_oracle(oracle, skew, 63, dev, amin=1)                            # one 10-bit bucket (900 000 rows under AAAAA) above the group limit:
    assert st["sort_fallback"] == 1, st                                                 #  the full-width order for THAT group, the others by the MSD kernels
    monkeypatch.setenv("DSKGPU_RS_MAX_ROWS", "3000")                                    # (one-word rows: most 10-bit buckets above the limit -> the library
    st = check_against_oracle(oracle, reads, 31, dev, amin=1)                           #  sort bucket by bucket, the MSD kernels for the small ones)
    assert st["sort_fallback"] == 1, st
    # a HEAVY first-digit bucket INSIDE a group's MSD sort (k_rs_split flags it and skips it) -- the per-group
    # library sort then reads the group from the split's output array, which must hold a complete permutation of the group's rows
    monkeypatch.setenv("DSKGPU_RS_MAX_ROWS", "300000")
    monkeypatch.setenv("DSKGPU_RS_HEAVY", "100")                                        # (a group of <= 300 000 rows has ~290 per first-digit bucket)
    for k, s in ((31, reads), (31, skew)):
        st = check_against_oracle(oracle, s, k, dev, amin=1)
        assert st["sort_fallback"] == 1, (k, st)
    monkeypatch.delenv("DSKGPU_RS_SLAB_ROWS")                                           # the same inside sort_rows_big's groups
    st = check_against_oracle(oracle, reads, 31, dev, amin=1)
    assert st["n_solid"] > 300000 and st["sort_fallback"] == 1, st


def test_partition_order_is_the_reference_contract(oracle, golden_dir, dev, monkeypatch):
    """DSKGPU_F_PARTITION_ORDER (csrc/partsort.h): the rows in the order the reference's readers are promised -- ascending INSIDE each
    output partition, partition after partition (utils/dsk2ascii.cpp:61,77,85-104) -- from one pass over the rows instead of the
    three of the global order.  Checked: same multiset of (k-mer, abundance) rows and same histogram as the oracle, every
    partition strictly ascending, no partition above what a block orders, the partition sizes add up; a partition / value bin a
    block cannot order (provoked: DSKGPU_PS_MAXC=1) takes the global sort and the rows come out globally ascending, for one- and
    two-word rows alike; the passes of a multi-pass count order their partitions one pass after the other; four-word rows (k > 64)
    take the flag too (their order: test_gpu_partition_order_wide.py)."""
    from dsk_amd import KmerCounter, synth
    g = synth.make_genome(600_000, dev)
    reads = synth.make_reads(g, 250_000, 150)
    gold, _ = oracle.load_bank(os.path.join(golden_dir, "read50x_ref10K_e001.fasta.gz"))
    rng = np.random.default_rng(5)
    pa = np.full(300_000, 65, np.uint8)
    hit = rng.random(pa.size) < 0.03
    pa[hit] = rng.choice(np.frombuffer(b"CGT", dtype=np.uint8), size=int(hit.sum()))
    skew = np.concatenate([pa, np.array([10], np.uint8), reads.cpu().numpy()]).astype(np.uint8)

    def run(stream, k, amin, **kw):
        t = torch.from_numpy(np.ascontiguousarray(stream)).to(dev)
        with KmerCounter(kmer_size=k, abundance_min=amin, partition_order=True, **kw) as kc:
            kc.set_reads_device(t.data_ptr(), t.numel())
            kc.count()
            sizes = kc.partition_sizes()
            kk, ab = kc.rows()
            return kk, ab, sizes, kc.histogram(), kc.stats()

    def check(stream, k, amin, expect_parts=True, **kw):
        kk, ab, sizes, hist, st = run(stream, k, amin, **kw)
        ref = oracle.count(np.ascontiguousarray(stream), k)
        keep = (ref.ab >= amin)
        want_k, want_a = ref.words()[keep], ref.ab[keep]
        assert st["n_kmers"] == ref.total and st["n_distinct"] == ref.distinct and st["n_solid"] == len(want_a), (k, amin, st)
        assert (hist == ref.histogram(10000)).all()
        assert sizes.sum() == len(want_a) == kk.shape[0] and st["n_partitions"] == len(sizes)
        order = np.lexsort(kk.T)                                  # (word 0 least significant: the last key of lexsort is the primary one)
        assert (kk[order] == want_k).all() and (ab[order] == want_a).all(), (k, amin)
        if kk.shape[1] == 1:
            asc = kk[1:, 0] > kk[:-1, 0]
            starts = np.cumsum(sizes)[:-1]
            inside = np.ones(len(asc), dtype=bool); inside[starts[(starts > 0) & (starts <= len(asc))] - 1] = False
            assert asc[inside].all(), (k, amin, "a partition is not ascending")
            if expect_parts is True:
                assert len(sizes) > 4 and sizes.max() <= 4096 and not asc.all(), (k, amin, len(sizes), sizes.max())
            elif expect_parts is False:
                assert asc.all(), (k, amin, "global order expected")
        return st

    for k, amin in ((31, 2), (31, 1), (21, 2), (13, 1), (32, 2)):
        check(reads.cpu().numpy(), k, amin)
    check(gold, 27, 1)
    check(skew, 31, 1)
    check(skew, 31, 2)
    check(reads.cpu().numpy(), 5, 1, expect_parts=None)           # (512 distinct 5-mers: a tiny row set, either layout)
    monkeypatch.setenv("DSKGPU_PS_MAXC", "1")                      # two rows in one value bin: the block gives up, the global sort takes over
    st = check(reads.cpu().numpy(), 31, 1, expect_parts=False)
    assert st["n_partitions"] == 4
    monkeypatch.delenv("DSKGPU_PS_MAXC")
    # several passes: every pass orders its partitions on the way into the job's row arrays (one launch per pass instead of the compaction,
    # no sort at the end); the partitions of the passes follow each other
    st = check(reads.cpu().numpy(), 31, 1, expect_parts=True, max_pass_mkeys=2)
    assert st["n_passes"] > 4
    st = check(skew, 31, 2, expect_parts=None, max_pass_mkeys=2)  # (the poly-A variants of a pass share a value bin: a block gives up on its own, the job's rows are sorted globally)
    assert st["n_passes"] > 4
    monkeypatch.setenv("DSKGPU_PS_MAXC", "1")                      # ... and a block that gives up in one of the passes: the global sort over all passes' rows
    st = check(reads.cpu().numpy(), 31, 1, expect_parts=False, max_pass_mkeys=2)
    assert st["n_passes"] > 4 and st["n_partitions"] == 4
    monkeypatch.delenv("DSKGPU_PS_MAXC")
    # two-word rows (33 <= k <= 64): 2048 rows per partition; every partition ascending on (high word, low word)
    for k, amin in ((63, 2), (63, 1), (33, 1), (40, 2), (64, 1)):
        kk, ab, sizes, hist, st = run(reads.cpu().numpy(), k, amin)
        ref = oracle.count(reads.cpu().numpy(), k)
        keep = ref.ab >= amin
        order = np.lexsort(kk.T)
        assert (kk[order] == ref.words()[keep]).all() and (ab[order] == ref.ab[keep]).all() and (hist == ref.histogram(10000)).all(), (k, amin)
        assert len(sizes) > 4 and sizes.max() <= 2048 and sizes.sum() == kk.shape[0] == st["n_solid"], (k, amin, len(sizes), sizes.max())
        asc = (kk[1:, 1] > kk[:-1, 1]) | ((kk[1:, 1] == kk[:-1, 1]) & (kk[1:, 0] > kk[:-1, 0]))
        starts = np.cumsum(sizes)[:-1]
        inside = np.ones(len(asc), dtype=bool); inside[starts[(starts > 0) & (starts <= len(asc))] - 1] = False
        assert asc[inside].all() and not asc.all(), (k, amin)
    check(skew, 63, 1, expect_parts=None)
    monkeypatch.setenv("DSKGPU_PS_MAXC", "1")                      # two-word rows whose blocks give up: the global sort reads the same sparse rows
    kk, ab, sizes, hist, st = run(reads.cpu().numpy(), 63, 1)
    monkeypatch.delenv("DSKGPU_PS_MAXC")
    ref = oracle.count(reads.cpu().numpy(), 63)
    assert (kk == ref.words()).all() and (ab == ref.ab).all() and (hist == ref.histogram(10000)).all()
    assert ((kk[1:, 1] > kk[:-1, 1]) | ((kk[1:, 1] == kk[:-1, 1]) & (kk[1:, 0] > kk[:-1, 0]))).all(), "global order expected"
    assert st["n_partitions"] == 4 and sizes.sum() == kk.shape[0] == st["n_solid"], st
    kk, ab, sizes, hist, st = run(reads.cpu().numpy(), 63, 1, max_pass_mkeys=2)          # two-word rows, several passes
    ref = oracle.count(reads.cpu().numpy(), 63)
    order = np.lexsort(kk.T)
    assert st["n_passes"] > 4 and (kk[order] == ref.words()).all() and (ab[order] == ref.ab).all() and sizes.max() <= 2048 and len(sizes) > 4 * st["n_passes"]
    check(reads.cpu().numpy(), 101, 2, expect_parts=None)                        # four-word rows: partition order as well (rows and histogram here, the order in test_gpu_partition_order_wide.py)


def test_multi_pass_count_leaves_the_sender_state_alone(oracle, dev):
    """the record-based level 0 of a multi-pass count has a sender state of its own (owners = passes, a
    repartition table for that many owners) and leaves the exchange's alone: a later dskgpu_mg_* call on the same world_size = 1
    context sees ONE owner (when the level 0 borrowed the exchange's state, such a call once looped over up to 64 owners into the
    caller's one-entry arrays)."""
    from dsk_amd import KmerCounter, synth
    from dsk_amd.multi import scatter_records
    reads = synth.make_reads(synth.make_genome(300_000, dev), 100_000, 150)
    ref = oracle.count(reads.cpu().numpy(), 31)
    with KmerCounter(kmer_size=31, abundance_min=1, max_pass_mkeys=2) as kc:
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        kc.count()
        st = kc.stats()
        assert st["n_passes"] > 4 and st["n_read_sweeps"] < st["n_passes"]            # the record-based level 0 ran
        assert st["n_kmers"] == ref.total and st["n_distinct"] == ref.distinct
        send, counts = scatter_records(kc, None, dev)                                 # the degenerate exchange: every record to owner 0
        assert len(counts) == 1 and counts[0] > 0
        assert kc.mg_sent_kmers() == [ref.total]
        torch.cuda.synchronize()
        kc.mg_count(send.data_ptr(), counts[0], ref.total)
        st2 = kc.stats()
        assert st2["n_kmers"] == ref.total and st2["n_distinct"] == ref.distinct
        assert (kc.histogram() == ref.histogram(10000)).all()
        kc.count()                                                                    # ... and the multi-pass count again, afterwards
        assert kc.stats()["n_distinct"] == ref.distinct


def test_multi_pass_count_keeps_the_callers_repartition_table(oracle, dev):
    """The record-based level 0 builds a repartition table for its passes; the table the caller set for the exchange (mg_set_table) is
    another one and survives the count: all buckets split -- every window a one-k-mer record -- sends the same records before and after,
    and more of them than the default table does."""
    from dsk_amd import KmerCounter, synth
    from dsk_amd.engine import MG_BUCKETS
    from dsk_amd.multi import scatter_records
    reads = synth.make_reads(synth.make_genome(300_000, dev), 100_000, 150)
    ref = oracle.count(reads.cpu().numpy(), 31)
    with KmerCounter(kmer_size=31, abundance_min=1) as kc:                            # what the default table sends for these reads
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        _, default_counts = scatter_records(kc, None, dev)
    with KmerCounter(kmer_size=31, abundance_min=1, max_pass_mkeys=2) as kc:
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        kc.mg_set_table(np.full(MG_BUCKETS, 255, dtype=np.uint8))
        _, counts = scatter_records(kc, None, dev)
        sent = kc.mg_sent_kmers()
        assert sent == [ref.total]
        kc.count()
        st = kc.stats()
        assert st["n_passes"] > 4 and st["n_read_sweeps"] < st["n_passes"]            # the record-based level 0 ran
        assert st["n_kmers"] == ref.total and st["n_distinct"] == ref.distinct
        _, counts2 = scatter_records(kc, None, dev)
        assert counts2 == counts and kc.mg_sent_kmers() == sent
        assert counts[0] > default_counts[0]


@pytest.mark.parametrize("k", [40, 63, 70, 100])
def test_multiword_row_sort_prefix_runs_and_fallback(oracle, dev, k):
    """Multi-word rows are ordered as (top 63 value bits, row index) pairs by the hand-written sort, rows that share all 63 bits
    by a tie pass with full comparison: 25 or 300 rows sharing a 20-base prefix stay on that path (the 300 in one cell are
    ordered by the block path's bitonic network); more than 32 rows that share ALL 63 bits are listed and ordered by one block per
    run (up to 4096 rows; beyond: the full-width fallback)."""
    rng = np.random.default_rng(12)
    tails = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(300, k - 20))
    noise = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=60_000).tobytes()
    head = b"AAAAAAAAAAAAAAAAAAAC"
    for nshare, fallback in ((25, 0), (300, 0)):
        recs = [head + t.tobytes() for t in tails[:nshare]]
        s = np.frombuffer(b"\n".join(recs) + b"\n" + noise + b"\n", dtype=np.uint8)
        st = check_against_oracle(oracle, s, k, dev, amin=1)
        assert st["sort_fallback"] == fallback
    # rows that share MORE than the 63 bits the sort looks at (36 leading bases): equal sort keys, ordered by the tie pass
    long_head = b"AAAAAAAAAAAAAAAAAAACAAAAAAAAAAAAAAAC"
    recs = [long_head + t.tobytes()[: k - 36] for t in tails[:25]]
    s = np.frombuffer(b"\n".join(recs) + b"\n" + noise + b"\n", dtype=np.uint8)
    st = check_against_oracle(oracle, s, k, dev, amin=1)
    assert st["sort_fallback"] == 0
    if k >= 63:      # 60 / 300 rows with equal sort keys: beyond what the tie pass orders in place -- listed, and ordered by one block each (k_fix_long_runs)
        for nshare in (60, 300):
            recs = [long_head + t.tobytes()[: k - 36] for t in tails[:nshare]]
            s = np.frombuffer(b"\n".join(recs) + b"\n" + noise + b"\n", dtype=np.uint8)
            st = check_against_oracle(oracle, s, k, dev, amin=1)
            assert st["sort_fallback"] == 0


@pytest.mark.parametrize("k,mkeys,n_reads", [(31, 2, 100_000), (27, 1, 60_000), (63, 1, 60_000)])
def test_multi_pass_over_key_space(oracle, dev, k, mkeys, n_reads):
    """Inputs with more k-mers than one pass may hold are counted in several passes over the key
    space (BASELINE.json configs[4] "multi-pass HBM partitioning"); forced here with a tiny pass size."""
    from dsk_amd import synth
    g = synth.make_genome(300_000, dev)
    reads = synth.make_reads(g, n_reads, 150).cpu().numpy()
    st = check_against_oracle(oracle, reads, k, dev, max_pass_mkeys=mkeys)
    assert st["n_passes"] >= st["n_kmers"] // (mkeys * 1_000_000)          # (sized from the valid k-mer windows, not from the bytes)
    assert st["n_passes"] > 1
    st1 = check_against_oracle(oracle, reads, k, dev)
    assert st1["n_passes"] == 1


def test_multi_pass_skewed_key_space(oracle, dev, monkeypatch):
    """Millions of copies of one k-mer land in ONE pass whatever the pass count.  On the sampled path that pass just gets longer
    slices (and the k-mer is counted apart); on the exact path (DSKGPU_NO_OPT2) the pass-capacity check must give the passes the
    capacity that pass needs -- more passes would not make it smaller -- and never write out of bounds."""
    from dsk_amd import synth
    g = synth.make_genome(200_000, dev)
    noise = synth.make_reads(g, 40_000, 150).cpu().numpy()
    s = np.concatenate([np.full(3_000_000, 65, np.uint8), np.array([10], np.uint8), noise]).astype(np.uint8)
    for exact in (False, True):
        if exact:
            monkeypatch.setenv("DSKGPU_NO_OPT2", "1")
        st = check_against_oracle(oracle, s, 31, dev, amin=1, max_pass_mkeys=2)      # 7.8 M k-mers / 2 M per pass, one pass holds 3 M + its share
        assert st["n_passes"] == 4
    monkeypatch.delenv("DSKGPU_NO_OPT2")
    t = np.full(3_000_000, 65, np.uint8)                                             # one k-mer x 3 M, 1 M per pass: three passes, two of them empty
    st = check_against_oracle(oracle, t, 31, dev, amin=1, max_pass_mkeys=1)
    assert st["n_passes"] == 3 and st["n_distinct"] == 1


def _bank_reference(oracle, streams, k, kind, amin, amax, mask, hmax=10000):
    """numpy restatement of the multi-bank semantics of include/dskgpu.h (DSKGPU_SOLIDITY_*), from per-bank oracle counts."""
    B = len(streams)
    per = [oracle.count(s, k) for s in streams]
    keys = np.unique(np.concatenate([p.values() if k > 32 else p.lo for p in per]))
    counts = np.zeros((len(keys), B), dtype=np.int64)
    for b, p in enumerate(per):
        kb = p.values() if k > 32 else p.lo
        idx = np.searchsorted(keys, kb)
        counts[idx, b] = p.ab
    tot = counts.sum(1)
    inwin = (counts >= amin) & (counts <= amax)
    if kind == "sum":
        solid = (tot >= amin) & (tot <= amax)
    elif kind == "min":
        solid = (counts.min(1) >= amin) & (counts.min(1) <= amax)
    elif kind == "max":
        solid = (counts.max(1) >= amin) & (counts.max(1) <= amax)
    elif kind == "one":
        solid = inwin.any(1)
    elif kind == "all":
        solid = inwin.all(1)
    else:
        m = np.array([(mask >> b) & 1 for b in range(B)], dtype=bool)
        solid = (counts[:, m] >= amin).all(1) & (counts[:, ~m] == 0).all(1)
    hist = np.bincount(np.minimum(tot, hmax), minlength=hmax + 1).astype(np.uint64)
    h2d = np.zeros((hmax + 1, 11), dtype=np.uint64)
    np.add.at(h2d, (np.minimum(tot - counts[:, 0], hmax), np.minimum(counts[:, 0], 10)), 1)
    return keys[solid], tot[solid], hist, h2d, sum(p.total for p in per)


@pytest.mark.parametrize("kind,mask", [("min", 0), ("max", 0), ("one", 0), ("all", 0), ("custom", 0b0101), ("sum", 0)])
def test_solidity_kinds_and_histo2d(oracle, golden_dir, dev, kind, mask):
    """-solidity-kind / -histo2D over several banks (unpinned by the reference's tests:
    checked against a numpy restatement built from per-bank oracle counts)."""
    from dsk_amd import KmerCounter
    streams = [oracle.load_bank(os.path.join(golden_dir, f"c{i}.fasta.gz"))[0] for i in (1, 2, 3, 4)]
    k, amin, amax = 27, 2, 40
    want_k, want_a, want_h, want_h2, want_total = _bank_reference(oracle, streams, k, kind, amin, amax, mask)
    whole = torch.from_numpy(np.concatenate(streams)).to(dev)
    ends = list(np.cumsum([len(s) for s in streams]))
    with KmerCounter(kmer_size=k, abundance_min=amin, abundance_max=amax, solidity_kind=kind, solidity_custom=mask, histo2d=True) as kc:
        kc.set_reads_device(whole.data_ptr(), whole.numel())
        kc.set_banks([int(e) for e in ends])
        kc.count()
        kmers, ab = kc.rows()
        st = kc.stats()
        assert (kc.histogram() == want_h).all()
        assert (kc.histogram2d() == want_h2).all()
    assert st["n_kmers"] == want_total and st["n_solid"] == len(want_k)
    assert (kmers[:, 0] == want_k).all() and (ab == want_a).all()


def test_solidity_two_word_and_push_path(oracle, golden_dir, dev):
    from dsk_amd import KmerCounter
    streams = [oracle.load_bank(os.path.join(golden_dir, f"c{i}.fasta.gz"))[0] for i in (1, 2)]
    k = 41
    want_k, want_a, want_h, want_h2, _ = _bank_reference(oracle, streams, k, "all", 1, 2**31 - 1, 0)
    with KmerCounter(kmer_size=k, abundance_min=1, solidity_kind="all", histo2d=True) as kc:
        for s in streams:                       # host path: one bank per push, separated by next_bank()
            kc.push_reads(s.tobytes())
            kc.next_bank()
        kc.count()
        kmers, ab = kc.rows()
        assert (kc.histogram() == want_h).all() and (kc.histogram2d() == want_h2).all()
    vals = np.array([(int(h) << 64) | int(l) for l, h in zip(kmers[:, 0], kmers[:, 1])], dtype=object)
    assert (vals == want_k).all() and (ab == want_a).all()


@pytest.mark.parametrize("ranks,k,transport,explicit", [(2, 31, "copy", False), (4, 27, "copy", False), (2, 63, "copy", False), (8, 20, "copy", False),
                                                        (2, 31, "copy", True), (1, 31, "rccl", False), (1, 63, "rccl", False), (1, 31, "copy", False)])
def test_group_count_in_one_process(oracle, golden_dir, dev, monkeypatch, ranks, k, transport, explicit):
    """dskgpu_group_*: what `dsk -nb-gpus N` runs -- N ranks inside one process, the exchange inside the library.  On the
    1-GPU box several ranks share device 0 (transport "copy"); the single-rank cases with transport "rccl" push the
    degenerate exchange (every record to owner 0) through librccl's grouped ncclSend / ncclRecv."""
    s, _ = oracle.load_bank(os.path.join(golden_dir, "read50x_ref10K_e001.fasta.gz"))
    group_count_case(oracle, s, monkeypatch, ranks, k, transport, explicit)


def group_count_case(oracle, s, monkeypatch, ranks, k, transport, explicit):
    """the body of test_group_count_in_one_process on the stream s"""
    from dsk_amd import KmerGroup
    monkeypatch.setenv("DSKGPU_GROUP_TRANSPORT", transport)
    recs = bytes(s).split(b"\n")
    ref = oracle.count(s, k)
    with KmerGroup([0] * ranks, kmer_size=k, abundance_min=2, nb_partitions=3, mg_explicit=explicit) as g:
        assert g.transport() == transport
        for r in range(ranks):
            g.rank(r).push_reads(b"\n".join(recs[r::ranks]) + b"\n")
        for rep in range(2):                                     # a second count reuses the buffers
            g.count()
            st = g.stats()
            assert st["n_kmers"] == ref.total and st["n_distinct"] == ref.distinct
            assert (g.histogram() == ref.histogram(10000)).all()
            assert g.num_partitions() == 3 * ranks
            ks, abs_ = [], []
            for p in range(g.num_partitions()):
                kk, aa = g.partition(p)
                key = kk[:, 0] if k <= 32 else kk[:, 1].astype(object) * (1 << 64) + kk[:, 0].astype(object)
                assert all(key[i] < key[i + 1] for i in range(len(key) - 1))      # ascending inside every partition
                ks.append(kk); abs_.append(aa)
            kk = np.concatenate(ks); aa = np.concatenate(abs_)
            order = np.argsort(kk[:, 0]) if k <= 32 else np.lexsort((kk[:, 0], kk[:, 1]))
            lo, hi, rab = ref.solid(2)
            assert (kk[order, 0] == lo).all() and (aa[order] == rab).all()
            if k > 32:
                assert (kk[order, 1] == hi).all()
            if ranks > 1:
                assert g.exchanged_words() > 0
                per_rank = [g.rank(r).stats()["n_kmers"] for r in range(ranks)]
                assert sum(per_rank) == ref.total and min(per_rank) > 0


@pytest.mark.parametrize("ranks,k,slices", [(4, 31, "4"), (4, 31, "0"), (2, 63, "4")])
def test_receive_side_stays_on_the_fast_path_with_repeats(oracle, dev, monkeypatch, ranks, k, slices):
    """The repeat machinery on the path the multi-GPU metric takes: every rank of a group receives super-k-mer RECORDS, and its
    level 1 reads them directly.  With a repeat-rich input (`small_repeats`: a high-copy family, tandem arrays, poly-A reads -- one
    rank owns a k-mer with 10^5 occurrences) the slices of that level are sized per bin from a positional sample of the records
    (k_sk_sample_keys; from the first slice when the exchange runs in slices), the dominant k-mer is counted apart (one-word
    keys), level 2 chains extension regions (two-word keys too): no rank retries, none takes a histogram pass, and the union
    of the ranks' rows equals the oracle's."""
    from dsk_amd import KmerGroup, synth
    monkeypatch.setenv("DSKGPU_GROUP_SLICES", slices)
    monkeypatch.setenv("DSKGPU_SK_MINSLICE", "1")
    reads, gl, nr, rl = synth.make_workload("small_repeats", dev)
    ref = oracle.count(reads.cpu().numpy(), k)
    per = nr // ranks
    with KmerGroup([0] * ranks, kmer_size=k, abundance_min=2, nb_partitions=1, timing=True) as g:
        for r in range(ranks):
            lo, hi = r * per * (rl + 1), (nr if r == ranks - 1 else (r + 1) * per) * (rl + 1)
            g.rank(r).set_reads_device(reads.data_ptr() + lo, hi - lo)
        g.count()
        st = g.stats()
        assert st["n_kmers"] == ref.total and st["n_distinct"] == ref.distinct
        assert (g.histogram() == ref.histogram(10000)).all()
        if slices != "0":
            assert g.sliced_steps() == 1
        per_rank = [g.rank(r).stats() for r in range(ranks)]
        stages = [dict(g.rank(r).stage_times()) for r in range(ranks)]
        assert all(s["n_retries"] == 0 for s in per_rank), per_rank
        assert all("hist1" not in t and "hist2" not in t for t in stages), stages
        assert sum(s["n_ext_regions"] for s in per_rank) > 0
        assert sum(s["n_heavy"] for s in per_rank) >= 1            # the poly-A k-mer, counted apart by its owner (one- and two-word keys)
        parts = [g.partition(p) for p in range(g.num_partitions())]
    kk = np.concatenate([p[0] for p in parts]); aa = np.concatenate([p[1] for p in parts])
    order = np.argsort(kk[:, 0], kind="stable") if k <= 32 else np.lexsort((kk[:, 0], kk[:, 1]))
    keep = ref.ab >= 2
    assert (kk[order] == ref.words()[keep]).all() and (aa[order] == ref.ab[keep]).all()


@pytest.mark.parametrize("ranks,k,mode", [(4, 31, "slices"), (2, 63, "slices"), (4, 31, "one_piece"), (4, 31, "one_rank_small"),
                                          (4, 31, "send_overflow")])
def test_group_step_in_slices(oracle, dev, monkeypatch, ranks, k, mode):
    """dskgpu_group_count with the exchange in slices (second stream + events per rank; the level-1 scatter of slice i - 1 and the
    sender of slice i + 1 run beside the exchange of slice i).  Collective fall-backs to the step in one piece: a rank whose input
    is too small for the sampled send layout, and a send slice that overflows (the sliced attempt is discarded and repeated)."""
    from dsk_amd import KmerGroup, synth
    monkeypatch.setenv("DSKGPU_SK_MINSLICE", "1")
    if mode == "one_piece":
        monkeypatch.setenv("DSKGPU_GROUP_SLICES", "1")
    if mode == "send_overflow":
        monkeypatch.setenv("DSKGPU_SK_SLICE", "300")            # records per (owner, chunk) slice: far too few
    n_reads = 600_000
    reads = synth.make_reads(synth.make_genome(2_000_000, dev), n_reads, 150).cpu().numpy()
    per = n_reads // ranks
    shards = [reads[r * per * 151: (r + 1) * per * 151] for r in range(ranks)]
    if mode == "one_rank_small":
        shards[1] = shards[1][: 2000 * 151]
        reads = np.concatenate(shards)
    ref = oracle.count(reads, k)
    with KmerGroup([0] * ranks, kmer_size=k, abundance_min=2, nb_partitions=2) as g:
        for r in range(ranks):
            g.rank(r).push_reads(shards[r].tobytes())
        for rep in range(2):
            g.count()
            assert g.sliced_steps() == (1 if mode == "slices" else 0)
            st = g.stats()
            assert st["n_kmers"] == ref.total and st["n_distinct"] == ref.distinct
            assert (g.histogram() == ref.histogram(10000)).all()
            ks, abs_ = [], []
            for p in range(g.num_partitions()):
                kk, aa = g.partition(p)
                ks.append(kk); abs_.append(aa)
            kk = np.concatenate(ks); aa = np.concatenate(abs_)
            order = np.argsort(kk[:, 0]) if k <= 32 else np.lexsort((kk[:, 0], kk[:, 1]))
            lo, hi, rab = ref.solid(2)
            assert (kk[order, 0] == lo).all() and (aa[order] == rab).all()
            if k > 32:
                assert (kk[order, 1] == hi).all()
            assert g.exchanged_words() > 0


@pytest.mark.parametrize("k", [15, 27, 63])
def test_group_with_idle_ranks(oracle, golden_dir, dev, k):
    """More ranks than reads: ranks that send nothing, receive nothing, or both (records for k >= 20, explicit keys below)."""
    from dsk_amd import KmerGroup
    s, _ = oracle.load_bank(os.path.join(golden_dir, "longread.fasta"))
    recs = [r for r in bytes(s).split(b"\n") if r][:3]                  # three long reads, eight ranks
    stream = np.frombuffer(b"\n".join(recs) + b"\n", dtype=np.uint8)
    ref = oracle.count(stream, k)
    with KmerGroup([0] * 8, kmer_size=k, abundance_min=1, nb_partitions=1) as g:
        for r, rec in enumerate(recs):
            g.rank(2 * r + 1).push_reads(rec + b"\n")
        g.count()
        assert g.stats()["n_kmers"] == ref.total and g.stats()["n_distinct"] == ref.distinct
        assert (g.histogram() == ref.histogram(10000)).all()
        parts = [g.partition(p) for p in range(g.num_partitions())]
    kk = np.concatenate([p[0] for p in parts]); aa = np.concatenate([p[1] for p in parts])
    order = np.argsort(kk[:, 0]) if k <= 32 else np.lexsort((kk[:, 0], kk[:, 1]))
    assert (kk[order, 0] == ref.lo).all() and (aa[order] == ref.ab).all()


@pytest.mark.parametrize("n_normal,n_polya,sliced", [(60_000, 20_000, False), (450_000, 150_000, True)])
def test_repartition_table_balances_heavy_minimizers(oracle, dev, monkeypatch, n_normal, n_polya, sliced):
    """Minimizer repartition (gatb-core's RepartitorAlgorithm, src/DSK.cpp:63): a quarter of the reads are noisy poly-A, so
    one minimizer (A^10) carries ~ 25 % of all windows.  With the default owner map (hash of the minimizer scaled to the
    world) one of four ranks receives far more than its share; with the table built from sampled bucket loads (heavy
    buckets split by k-mer, the rest placed largest first) max / mean of the received k-mers stays <= 1.5.  Same rows,
    same histogram either way."""
    from dsk_amd import KmerGroup, synth, make_table, KmerCounter
    rng = np.random.default_rng(7)
    if sliced:                                                    # the sampled slice layout of the sender together with split buckets
        monkeypatch.setenv("DSKGPU_SK_MINSLICE", "1")
    normal = synth.make_reads(synth.make_genome(300_000, dev), n_normal, 150).cpu().numpy().reshape(-1, 151)
    polya = np.full((n_polya, 151), ord("A"), dtype=np.uint8); polya[:, 150] = 10
    noise = rng.random((n_polya, 150)) < 0.05
    polya[:, :150][noise] = rng.choice(np.frombuffer(b"CGT", dtype=np.uint8), int(noise.sum()))
    reads = np.concatenate([normal, polya]); rng.shuffle(reads)
    stream = reads.reshape(-1)
    ref = oracle.count(stream, 31)
    lo, hi, rab = ref.solid(2)
    world, per = 4, len(reads) // 4
    ratios = {}
    for balance in ("0", "1"):
        monkeypatch.setenv("DSKGPU_GROUP_BALANCE", balance)
        with KmerGroup([0] * world, kmer_size=31, abundance_min=2, nb_partitions=1) as g:
            for r in range(world):
                g.rank(r).push_reads(reads[r * per: (r + 1) * per if r < world - 1 else len(reads)].reshape(-1))
            g.count()
            got = [g.rank(r).stats()["n_kmers"] for r in range(world)]
            assert sum(got) == ref.total and (g.histogram() == ref.histogram(10000)).all()
            parts = [g.partition(p) for p in range(g.num_partitions())]
            kk = np.concatenate([p[0][:, 0] for p in parts]); aa = np.concatenate([p[1] for p in parts])
            order = np.argsort(kk)
            assert (kk[order] == lo).all() and (aa[order] == rab).all()
            ratios[balance] = max(got) / (sum(got) / world)
    assert ratios["0"] > 1.5, ratios            # the skew is real without the table ...
    assert ratios["1"] <= 1.5, ratios           # ... and gone with it
    # the table itself: deterministic, names only owners of the world, splits the heavy bucket
    with KmerCounter(kmer_size=31, world_size=world, rank=0) as kc:
        t = torch.from_numpy(stream.copy()).to(dev)
        kc.set_reads_device(t.data_ptr(), t.numel())
        loads = kc.mg_sample()
    table = make_table(loads, world)
    assert (make_table(loads, world) == table).all() and (table == 255).sum() >= 1 and table[table != 255].max() < world
    assert loads.sum() > 0.5 * ref.total and loads.sum() < 2.0 * ref.total        # sampled estimate of all windows


def test_exchange_over_rccl_single_rank(oracle, golden_dir, dev):
    """The `nccl` branch of dsk_amd.multi.exchange (variable-size all_to_all_single on device tensors) and the whole
    ShardedCounter step under init_process_group("nccl", world_size=1): ragged, empty and repeated exchanges."""
    import socket
    import torch.distributed as dist
    from dsk_amd import KmerCounter
    from dsk_amd.multi import ShardedCounter, exchange, gather_histogram
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", world_size=1, rank=0, device_id=dev)
    try:
        assert dist.get_backend() == "nccl"
        for n in (0, 1, 7, 100_003):
            send = torch.arange(n + 5, dtype=torch.int64, device=dev)
            out, rc = exchange(send, [n])
            assert rc == [n] and out.numel() == n and (out == send[:n]).all()
        recv = torch.empty(10, dtype=torch.int64, device=dev)          # a receive buffer that is too small is replaced
        out, rc = exchange(torch.arange(1000, dtype=torch.int64, device=dev), [1000], recv=recv)
        assert out.numel() == 1000 and int(out[-1]) == 999
        s, _ = oracle.load_bank(os.path.join(golden_dir, "read50x_ref10K_e001.fasta.gz"))
        t = torch.from_numpy(s).to(dev)
        for k in (31, 63, 15):
            ref = oracle.count(s, k)
            with KmerCounter(kmer_size=k, abundance_min=2, world_size=1, rank=0, stream=torch.cuda.current_stream().cuda_stream) as kc:
                kc.set_reads_device(t.data_ptr(), t.numel())
                sc = ShardedCounter(kc, dev)
                for _ in range(2):
                    sc.count()
                    kk, aa = kc.rows()
                    lo, hi, rab = ref.solid(2)
                    assert (kk[:, 0] == lo).all() and (aa == rab).all()
                    h = gather_histogram(torch.from_numpy(kc.histogram().astype(np.int64)).to(dev))
                    assert (h.cpu().numpy().astype(np.uint64) == ref.histogram(10000)).all()
                    assert sc.last_send_counts == sc.last_recv_counts and sum(sc.last_send_counts) > 0
                    assert not sc.last_step_sliced                  # (this input is too small for the sampled send layout)
        # a step in slices over RCCL: asynchronous all_to_all_single per slice on the process group's stream, the sender of
        # the next slice and the level-1 scatter of the previous one on the context's (= torch's current) stream
        from dsk_amd import synth
        os.environ["DSKGPU_SK_MINSLICE"] = "1"
        try:
            reads = synth.make_reads(synth.make_genome(1_000_000, dev), 300_000, 150)
            for k in (31, 63):
                ref = oracle.count(reads.cpu().numpy(), k)
                with KmerCounter(kmer_size=k, abundance_min=2, world_size=1, rank=0, stream=torch.cuda.current_stream().cuda_stream) as kc:
                    kc.set_reads_device(reads.data_ptr(), reads.numel())
                    sc = ShardedCounter(kc, dev, slices=4)
                    for it in range(2):
                        sc.count()
                        assert sc.last_step_sliced
                        st = kc.stats()
                        assert (st["n_kmers"], st["n_distinct"]) == (ref.total, ref.distinct), (k, it, st)
                        assert st["n_retries"] == 0                      # the level-1 launches per slice took everything
                        kk, aa = kc.rows()
                        lo, hi, rab = ref.solid(2)
                        assert len(kk) == len(lo), (k, it, st)
                        assert (kk[:, 0] == lo).all() and (aa == rab).all()
                        assert (kc.histogram() == ref.histogram(10000)).all()
        finally:
            del os.environ["DSKGPU_SK_MINSLICE"]
    finally:
        dist.destroy_process_group()


def test_failed_slice_gate_stops_the_count(dev, monkeypatch):
    """A gate that fails (the wait for a slice of the exchange timed out or was aborted) must not turn into counts of records that
    never arrived: the engine stops enqueuing work, still calls the remaining gates, returns an error and holds no result; the
    Python binding re-raises the gate's own exception (ctypes would have printed and swallowed it: ADVICE r03)."""
    from dsk_amd import KmerCounter, synth
    from dsk_amd.engine import DskGpuError
    monkeypatch.setenv("DSKGPU_SK_MINSLICE", "1")
    reads = synth.make_reads(synth.make_genome(1_000_000, dev), 300_000, 150)
    with KmerCounter(kmer_size=31, abundance_min=2, world_size=1, rank=0) as kc:
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        ns, w, est = kc.mg_slices_prepare(4)
        assert ns == 4
        send = torch.zeros(kc.mg_send_capacity_words(), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        for sl in range(4):
            kc.mg_scatter_slice(send.data_ptr(), send.numel(), sl)
        torch.cuda.synchronize()
        slice_words = [sum(x) for x in w]
        seen = []

        def gate(s):
            seen.append(s)
            if s == 1:
                raise TimeoutError("slice 1 never arrived")
        with pytest.raises(TimeoutError):
            kc.mg_count_sliced(send.data_ptr(), slice_words, est[0], gate)
        assert seen == [0, 1, 2, 3]                      # every gate was passed (the caller's work handles are all waited for)
        with pytest.raises(DskGpuError):
            kc.stats()                                   # no result
        assert kc.mg_slices_finish() is False
        # the context is still usable: the same step with working gates
        ns, w, est = kc.mg_slices_prepare(4)
        for sl in range(4):
            kc.mg_scatter_slice(send.data_ptr(), send.numel(), sl)
        torch.cuda.synchronize()
        kc.mg_count_sliced(send.data_ptr(), [sum(x) for x in w], est[0], lambda s: None)
        with KmerCounter(kmer_size=31, abundance_min=2) as one:
            one.set_reads_device(reads.data_ptr(), reads.numel())
            one.count()
            assert kc.stats()["n_kmers"] == one.stats()["n_kmers"] and kc.stats()["n_distinct"] == one.stats()["n_distinct"]
            assert (kc.histogram() == one.histogram()).all()


@pytest.mark.parametrize("world,k", [(2, 31), (4, 63)])
def test_sliced_step_with_real_processes(dev, world, k):
    """tools/check_multi.py: `world` processes under torch.distributed.run sharing cuda:0, the exchange over gloo (every slice staged
    through host memory): the whole protocol of ShardedCounter -- counts round, slice layouts of several real senders, gates,
    collective flags -- with the real engine; the sum over the ranks equals a single-context count of all the reads."""
    import gc, socket, subprocess, sys
    gc.collect(); torch.cuda.empty_cache()          # the child processes share this GPU: give back what earlier tests left in torch's cache
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DSKGPU_SK_MINSLICE="1")
    # (no retry: the intermittent r03 failure was the tool's own reference count reading the concatenated reads before torch had
    #  written them -- tools/stress_multi.py, profiles/r04_stress/, NOTEBOOK.md section 5 -- and a red here is a red)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(root, "tools", "check_multi.py"), str(k), "400000"],
                       cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0 and f"multi ok: world={world} k={k} sliced=True" in out, out


@pytest.mark.parametrize("world,k", [(4, 63)])
def test_sharded_count_stress_with_real_processes(dev, world, k):
    """tools/stress_multi.py: the same processes, 12 sliced steps in a row with send and receive buffers poisoned with valid records
    of other reads before every step; every step must equal the one-piece step and the (synchronised) single-context count, and
    every rank reports its own exception."""
    import gc, socket, subprocess, sys
    gc.collect(); torch.cuda.empty_cache()
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(root, "tools", "stress_multi.py"), str(k), "300000", "12"],
                       cwd=root, env=dict(os.environ), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0 and f"stress ok: world={world} k={k} iters=12" in out, out


def test_buffer_placement_keeps_results(dev):
    """DSKGPU_F_PLACE (best-placed of 8 candidate allocations for every big device buffer) is a matter of speed only: same rows and
    histogram as a context on plain hipMalloc buffers.  Last in the file: the flag is process-wide once a context asked for it."""
    from dsk_amd import synth, KmerCounter
    reads = synth.make_reads(synth.make_genome(6_000_000, dev), 2_000_000, 150)
    with KmerCounter(kmer_size=31) as kc:
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        kc.count()
        k0, a0 = kc.rows()
        h0, st0 = kc.histogram(), kc.stats()
    with KmerCounter(kmer_size=31, place=True) as kc:
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        for _ in range(2):
            kc.count()
            k1, a1 = kc.rows()
            assert (k1 == k0).all() and (a1 == a0).all() and (kc.histogram() == h0).all()
            assert kc.stats()["n_kmers"] == st0["n_kmers"] and kc.stats()["n_retries"] == 0
