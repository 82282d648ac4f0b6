"""The abundance window and the histogram of a count, at the corner points of every kernel that decides them.

A pass ends in a sweep: every distinct k-mer's count c goes to histogram bin min(c, histo_max) -- bins below CNT_LH = 512 through an
LDS array that is flushed at the end, higher bins straight to global memory, abundance 1 counted apart by ballot -- and becomes a row
when abundance_min <= c <= abundance_max.  csrc/kernels.h holds this sweep once per count kernel (k_count1, k_count1v3,
k_count_chained, k_count_mw, k_count2v3, k_count_chained_mw), and k_heavy_rows and k_merge_banks (MB_LH = 256, MB_L2 = 32, bank-0
column clamped at 10) restate its rules.  The tests here put planted k-mers of exact abundances on these constants and the window's
edges into the dense part of the abundance distribution, path by path; the facts from stats() / stage_times() say which kernel ran.

Every comparison is exact, against the CPU oracle: rows in order, every 64-bit word, abundances, the whole histogram of
histo_max + 1 bins, n_kmers, n_distinct and n_solid.  Every test first asserts, on the oracle result alone, that the edges its window
names are populated: a planted value with exactly one k-mer, or at least 20 k-mers.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MAX = 2147483647
RL = 150
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


def planted_kmer(seed, k):
    return np.random.default_rng(seed).choice(ACGT, size=k)


def reads_with_planted_kmers(rng, n_reads, rl, k, planted, genome=None):
    """The recipe of tests/test_gpu_parity.py (_reads_with_planted_kmers), restated: error-free reads of a random genome (20x) with
    `planted` = [(copies, seed)] fixed k-mers written over a random window of `copies` distinct reads each.  genome: reads of this
    genome instead of a fresh one (the banks of one count share theirs)."""
    if genome is None:
        genome = rng.choice(ACGT, size=max(rl + 1, n_reads * rl // 20))
    reads = genome[rng.integers(0, len(genome) - rl, size=n_reads)[:, None] + np.arange(rl)[None, :]]
    free = rng.permutation(n_reads)
    at = 0
    for copies, seed in planted:
        rows = free[at: at + copies]; at += copies
        assert len(rows) == copies, "more planted copies than reads"
        pos = rng.integers(0, rl - k + 1, size=copies)
        reads[rows[:, None], pos[:, None] + np.arange(k)[None, :]] = planted_kmer(seed, k)[None, :]
    return np.concatenate([reads, np.full((n_reads, 1), ord("\n"), np.uint8)], axis=1).reshape(-1)


# ------------------------------------------------------------------ streams: the smallest that take each path (make_plan goes to two
# levels above 1024 x 2900 one-word, 1024 x 2560 two-word and 1024 x 640 four-word keys)
ONE_LEVEL = (255, 256, 257, 510, 511, 512, 513, 599, 600, 601)
TWO_LEVELS = ONE_LEVEL + (5119, 5120, 5121)          # these three outgrow their region: the chained kernels count them
STREAMS = {                                          # name: (k, reads, planted abundances)
    "k31_one": (31, 8_000, ONE_LEVEL),
    "k31_two": (31, 30_000, TWO_LEVELS),
    "k63_one": (63, 8_000, ONE_LEVEL),
    "k63_two": (63, 34_000, TWO_LEVELS),
    "k97_one": (97, 8_000, ONE_LEVEL),
    "k97_two": (97, 14_000, (100, 200, 300)),        # a four-word region holds 1090 keys and has no chains: nothing larger
}
_streams, _refs, _on_device = {}, {}, {}


def stream_of(name):
    if name not in _streams:
        k, n_reads, planted = STREAMS[name]
        _streams[name] = reads_with_planted_kmers(np.random.default_rng(7), n_reads, RL, k, [(a, 100 + i) for i, a in enumerate(planted)])
    return _streams[name]


def ref_of(oracle, name, stream, k):
    if (name, k) not in _refs:
        _refs[(name, k)] = oracle.count(stream, k)
    return _refs[(name, k)]


def device_bytes(name, stream, dev):
    if name not in _on_device:
        _on_device[name] = torch.from_numpy(np.ascontiguousarray(stream)).to(dev)
    return _on_device[name]


# ------------------------------------------------------------------ windows (abundance_min, abundance_max, histo_max); m = the most
# frequent abundance >= 4 of the stream, from the oracle
WINDOWS = {
    "w1_1_max_h10000": lambda m: (1, MAX, 10000),             # singletons become rows: the ballot-counted abundance 1
    "w2_m-1_m+1_hm": lambda m: (m - 1, m + 1, m),             # both edges and the clamp in the dense part, inside the LDS bins
    "w3_m_m_hm-1": lambda m: (m, m, m - 1),                   # one value, the histogram clamped below it
    "w4_1_1_h1": lambda m: (1, 1, 1),                         # every c > 1 clamps into the bin of the ballot-counted ones
    "w5_2_512_h512": lambda m: (2, 512, 512),                 # histo_max == CNT_LH: bin 511 in LDS, 512 global, 513 clamps to 512
    "w6_513_max_h511": lambda m: (513, MAX, 511),             # histo_max == CNT_LH - 1: the whole tail in the last LDS bin
    "w7_512_600_h600": lambda m: (512, 600, 600),             # window and clamp wholly above the LDS bins
    "w8_256_256_h256": lambda m: (256, 256, 256),             # one planted row, at the MB_LH-sized neighbour of the constant
    "w9_5120_5120_h5120": lambda m: (5120, 5120, 5120),       # the k-mer the chained kernels count
    "w200_200_200_h200": lambda m: (200, 200, 200),           # four-word keys on two levels: their planted row
}
W_1_8 = list(WINDOWS)[:8]
W_1_9 = list(WINDOWS)[:9]
W_K97_TWO = W_1_8[:4] + ["w200_200_200_h200"]
ONE_LEVEL_CASES = [(s, w) for s in ("k31_one", "k63_one", "k97_one") for w in W_1_8]
TWO_LEVEL_CASES = [(s, w) for s in ("k31_two", "k63_two") for w in W_1_9] + [("k97_two", w) for w in W_K97_TWO]


def case_ids(cases):
    return [f"{s}-{w}" for s, w in cases]


def mode_of(ref):
    """the most frequent abundance >= 4"""
    return 4 + int(np.argmax(np.bincount(ref.ab)[4:]))


def require_edges(ref, planted, amin, amax, hmax, neighbours=True):
    """Precondition, on the oracle result alone: every abundance the window names is populated -- a planted value with exactly one
    k-mer, or at least 20 k-mers -- and so is the value just outside each edge, so that no window passes over an empty edge."""
    edges = {amin}
    if amax != MAX: edges.add(amax)
    if hmax != 10000: edges.add(hmax)
    if neighbours:
        edges |= ({amin - 1} if amin > 1 else set()) | ({amax + 1} if amax != MAX else set()) | ({hmax + 1} if hmax != 10000 else set())
    counts = np.bincount(ref.ab)
    for e in sorted(edges):
        n = int(counts[e]) if e < len(counts) else 0
        assert n == 1 if e in planted else n >= 20, f"abundance {e}: {n} k-mers in the reference"
    for a in planted:
        assert counts[a] == 1, f"planted abundance {a}: {counts[a]} k-mers in the reference"


def run_count(t, k, amin, amax, hmax, **kw):
    from dsk_amd import KmerCounter
    with KmerCounter(kmer_size=k, abundance_min=amin, abundance_max=amax, histo_max=hmax, timing=True, **kw) as kc:
        kc.set_reads_device(t.data_ptr(), t.numel())
        kc.count()
        torch.cuda.synchronize()
        rows, ab = kc.rows()
        return rows, ab, kc.histogram(), kc.stats(), dict(kc.stage_times())


def check_exact(ref, k, got, amin, amax, hmax):
    rows, ab, hist, st, _ = got
    keep = (ref.ab >= amin) & (ref.ab <= amax)
    n = int(keep.sum())
    assert st["n_kmers"] == ref.total and st["n_distinct"] == ref.distinct
    assert st["n_solid"] == n
    want = ref.histogram(hmax)
    assert hist.shape == want.shape == (hmax + 1,)
    bad = np.flatnonzero(hist != want)
    assert bad.size == 0, f"histogram bins {bad[:8]}: got {hist[bad[:8]]}, want {want[bad[:8]]}"
    assert rows.shape == (n, (k + 31) // 32) and ab.shape == (n,)
    assert (rows == ref.words()[keep]).all()          # the oracle's order, every 64-bit word
    assert (ab == ref.ab[keep]).all()


def planted_case(oracle, dev, name, window):
    """-> (stats, stages) of one count of stream `name` under `window`, checked against the oracle"""
    k, _, planted = STREAMS[name]
    stream = stream_of(name)
    ref = ref_of(oracle, name, stream, k)
    amin, amax, hmax = WINDOWS[window](mode_of(ref))
    # (k97_two plants 100, 200 and 300 only: nothing lies next to its one-value window)
    require_edges(ref, planted, amin, amax, hmax, neighbours=window != "w200_200_200_h200")
    got = run_count(device_bytes(name, stream, dev), k, amin, amax, hmax)
    check_exact(ref, k, got, amin, amax, hmax)
    return got[3], got[4]


# ------------------------------------------------------------------ 1. one level: k_count1<false>, k_count_mw<2, false>, k_count_mw<4, false>
@pytest.mark.parametrize("name,window", ONE_LEVEL_CASES, ids=case_ids(ONE_LEVEL_CASES))
def test_one_level(oracle, dev, name, window):
    st, _ = planted_case(oracle, dev, name, window)
    assert st["n_levels"] == 1


# ------------------------------------------------------------------ 2. two levels, fixed-capacity regions: k_count1v3 (k = 31), k_count2v3
# (k = 63), k_count_mw<4, true> (k = 97); the planted 5119 .. 5121 go through k_count_chained / k_count_chained_mw
def histogram_free(st, stages, k):
    assert st["n_levels"] == 2 and st["n_retries"] == 0
    assert "hist1" not in stages and "hist2" not in stages
    if k <= 64:
        assert st["n_ext_regions"] > 0


@pytest.mark.parametrize("name,window", TWO_LEVEL_CASES, ids=case_ids(TWO_LEVEL_CASES))
def test_two_levels(oracle, dev, name, window):
    st, stages = planted_case(oracle, dev, name, window)
    histogram_free(st, stages, STREAMS[name][0])


# ------------------------------------------------------------------ 3. two levels, exact offsets behind the histogram and the scan:
# k_count1<false> / k_count_mw<W, false> over sub-partitions of a two-level plan
@pytest.mark.parametrize("name,window", TWO_LEVEL_CASES, ids=case_ids(TWO_LEVEL_CASES))
def test_two_levels_exact_offsets(oracle, dev, monkeypatch, name, window):
    monkeypatch.setenv("DSKGPU_NO_OPT2", "1")
    st, stages = planted_case(oracle, dev, name, window)
    assert st["n_levels"] == 2 and st["n_retries"] == 0 and "hist2" in stages


# ------------------------------------------------------------------ 4. two levels, regions above the list-free kernels' limit:
# k_count1<true> (cap > CNT_V3_KEYS * CNT_NT = 5120) and k_count_mw<2, true> (cap > C2V_NKEYS * CNT_NT = 4096).  Both caps are
# multiples of the level-2 scatter's aligned group (8 one-word, 4 two-word keys), which is all k_scatter_al asks of a region size.
LARGE_REGION_CASES = [(s, c, w) for s, c in (("k31_two", 6144), ("k63_two", 4608)) for w in W_1_9]


@pytest.mark.parametrize("name,cap,window", LARGE_REGION_CASES, ids=[f"{s}-cap{c}-{w}" for s, c, w in LARGE_REGION_CASES])
def test_two_levels_large_regions(oracle, dev, monkeypatch, name, cap, window):
    monkeypatch.setenv("DSKGPU_OPT_CAP", str(cap))
    st, stages = planted_case(oracle, dev, name, window)
    histogram_free(st, stages, STREAMS[name][0])


# ------------------------------------------------------------------ 5. k_heavy_rows<1>, <2>: the k-mer counted apart by the level-1 scatter
# (a third of that stream: with half of this again the plan has one level and no k-mer is counted apart)
HEAVY_JUNK, HEAVY_READS, HEAVY_TAIL = 2_000_000, 20_000, 1_000_000


def heavy_stream():
    """the stream of test_mostly_invalid_stream_with_a_dense_tail (tests/test_gpu_parity.py), shrunk: mostly N, some random reads,
    and a tail that is one repeated k-mer (poly-A), nearly all of its level-1 bin"""
    if "heavy" not in _streams:
        rng = np.random.default_rng(3)
        junk = np.full(HEAVY_JUNK, ord("N"), dtype=np.uint8)
        junk[rng.integers(0, HEAVY_JUNK, 40_000)] = ord("A")                # isolated bases: no k-mer
        some = np.concatenate([rng.choice(ACGT, size=(HEAVY_READS, RL)), np.full((HEAVY_READS, 1), ord("\n"), np.uint8)], axis=1).reshape(-1)
        tail = np.full(HEAVY_TAIL, ord("A"), dtype=np.uint8)
        _streams["heavy"] = np.concatenate([junk, some, tail])
    return _streams["heavy"]


HEAVY_WINDOWS = {
    "c_c_h10000": lambda c: (c, c, 10000),          # the only row; its bin is the clamped one
    "c+1_max_hc": lambda c: (c + 1, MAX, c),        # no row; the last bin
    "1_c-1_hc+1": lambda c: (1, c - 1, c + 1),      # every row but this one; the bin before the last
}


def heavy_case(oracle, dev, k, window):
    """one count of the heavy stream under `window`, exact against the oracle -> stats"""
    stream = heavy_stream()
    ref = ref_of(oracle, "heavy", stream, k)
    at = int(np.argmax(ref.ab))
    c = int(ref.ab[at])
    assert c == HEAVY_TAIL - k + 1 and (ref.words()[at] == 0).all() and int((ref.ab == c).sum()) == 1      # poly-A: the value 0
    assert int(np.sort(ref.ab)[-2]) < 10000                                                                  # nothing else near it
    amin, amax, hmax = HEAVY_WINDOWS[window](c)
    got = run_count(device_bytes("heavy", stream, dev), k, amin, amax, hmax)
    check_exact(ref, k, got, amin, amax, hmax)
    rows, ab, hist, st, _ = got
    assert st["n_levels"] == 2 and st["n_retries"] == 0
    assert hist[min(c, hmax)] == 1 and (hmax <= c or hist[hmax] == 0)      # the clamped bin, the last one, the one before the last
    assert int((ab == c).sum()) == (1 if window == "c_c_h10000" else 0)
    return st


@pytest.mark.parametrize("window", list(HEAVY_WINDOWS))
@pytest.mark.parametrize("k", [31, 63])
def test_heavy_rows(oracle, dev, k, window):
    assert heavy_case(oracle, dev, k, window)["n_heavy"] == 1


# ------------------------------------------------------------------ 6. k_merge_banks: solidity kinds, histogram and 2-D histogram of
# three banks.  Planted k-mers with per-bank copies (bank 0, 1, 2); window (20, 40)
BANK_AMIN, BANK_AMAX = 20, 40
BANK_PLANTS = [
    (85, 85, 85), (85, 85, 86), (85, 86, 86),                   # sums 255, 256, 257: MB_LH
    (5, 15, 16), (5, 16, 16), (5, 16, 17),                      # the part outside bank 0: 31, 32, 33: MB_L2
    (9, 3, 3), (10, 3, 3), (11, 3, 3),                          # bank 0: 9, 10, 11: the last column of the 2-D histogram
    (7, 6, 6), (7, 7, 6), (14, 13, 13), (14, 14, 13),           # sum: 19, 20, 40, 41
    (19, 30, 30), (20, 30, 30), (40, 45, 45), (41, 45, 45),     # min
    (19, 5, 5), (20, 5, 5), (40, 5, 5), (41, 5, 5),             # max
    (19, 0, 0), (20, 0, 0), (40, 0, 0), (41, 0, 0),             # one: a single bank
    (19, 20, 20), (20, 20, 20), (40, 40, 40), (41, 40, 40),     # all
    (19, 0, 20), (20, 0, 20), (20, 1, 20), (41, 0, 41),         # custom 0b101: banks 0 and 2 at amin or more, bank 1 empty
]
BANK_KINDS = [("min", 0), ("max", 0), ("one", 0), ("all", 0), ("custom", 0b101), ("sum", 0)]
_banks = {}


class CountOnce:
    """the oracle, with the count of every (stream, k) kept: _bank_reference counts its banks at every call"""
    def __init__(self, oracle):
        self.oracle, self.kept = oracle, {}

    def count(self, stream, k):
        if (id(stream), k) not in self.kept:
            self.kept[(id(stream), k)] = (stream, self.oracle.count(stream, k))
        return self.kept[(id(stream), k)][1]


def banks_of(oracle, k):
    """-> (streams of the three banks, per-bank oracle counts behind CountOnce, int64[planted, bank] counts in the reference)"""
    if k not in _banks:
        rng = np.random.default_rng(7)
        genome = rng.choice(ACGT, size=2_000 * RL // 20)
        streams = [reads_with_planted_kmers(rng, 2_000, RL, k, [(c[b], 100 + i) for i, c in enumerate(BANK_PLANTS)], genome=genome) for b in range(3)]
        once = CountOnce(oracle)
        counts = np.zeros((len(BANK_PLANTS), 3), dtype=np.int64)
        for i in range(len(BANK_PLANTS)):
            w = oracle.count(planted_kmer(100 + i, k), k).words()[0]      # the canonical value of the planted k-mer
            for b, s in enumerate(streams):
                r = once.count(s, k)
                counts[i, b] = r.ab[(r.words() == w[None, :]).all(1)].sum()
        _banks[k] = (streams, once, counts)
    return _banks[k]


def require_bank_edges(counts, kind, mask):
    """Preconditions on the reference's counts of the planted k-mers: they are the planted ones, and the constants of k_merge_banks
    and both edges of the window, for the deciding quantity of `kind`, each have a k-mer on them, below them and above them."""
    assert (counts == np.array(BANK_PLANTS)).all()
    tot = counts.sum(1)
    assert {255, 256, 257} <= set(tot) and {31, 32, 33} <= set(tot - counts[:, 0]) and {9, 10, 11} <= set(counts[:, 0])
    edges = {BANK_AMIN - 1, BANK_AMIN, BANK_AMAX, BANK_AMAX + 1}
    if kind == "sum": assert edges <= set(tot)
    if kind == "min": assert edges <= set(counts.min(1))
    if kind == "max": assert edges <= set(counts.max(1))
    if kind == "one": assert edges <= set(counts[(counts > 0).sum(1) == 1].max(1))          # k-mers of a single bank
    if kind == "all": assert edges <= set(counts[(counts[:, 1:] >= BANK_AMIN).all(1) & (counts[:, 1:] <= BANK_AMAX).all(1), 0])
    if kind == "custom":
        m = np.array([(mask >> b) & 1 for b in range(3)], dtype=bool)
        assert {BANK_AMIN - 1, BANK_AMIN, BANK_AMAX + 1} <= set(counts[(counts[:, ~m] == 0).all(1)][:, m].min(1))
        assert ((counts[:, ~m] > 0).any(1) & (counts[:, m] >= BANK_AMIN).all(1)).any()      # kept out by the other bank alone


@pytest.mark.parametrize("hmax", [10000, 256, 255, 32, 31])
@pytest.mark.parametrize("kind,mask", BANK_KINDS)
@pytest.mark.parametrize("k", [27, 41])
def test_merge_banks(oracle, dev, k, kind, mask, hmax):
    from dsk_amd import KmerCounter
    from tests.test_gpu_parity import _bank_reference
    streams, once, counts = banks_of(oracle, k)
    require_bank_edges(counts, kind, mask)
    want_k, want_a, want_h, want_h2, want_total = _bank_reference(once, streams, k, kind, BANK_AMIN, BANK_AMAX, mask, hmax)
    assert 0 < len(want_k) < int(want_h.sum())
    whole = device_bytes(f"banks{k}", np.concatenate(streams), dev)
    ends = [int(e) for e in np.cumsum([len(s) for s in streams])]
    with KmerCounter(kmer_size=k, abundance_min=BANK_AMIN, abundance_max=BANK_AMAX, histo_max=hmax, solidity_kind=kind, solidity_custom=mask,
                     histo2d=True) as kc:
        kc.set_reads_device(whole.data_ptr(), whole.numel())
        kc.set_banks(ends)
        kc.count()
        kmers, ab = kc.rows()
        st = kc.stats()
        hist, h2 = kc.histogram(), kc.histogram2d()
    assert hist.shape == (hmax + 1,) and h2.shape == (hmax + 1, 11)
    assert (hist == want_h).all()
    assert (h2 == want_h2).all()
    assert st["n_kmers"] == want_total and st["n_distinct"] == int(want_h.sum()) and st["n_solid"] == len(want_k)
    assert kmers.shape == (len(want_k), (k + 31) // 32)
    vals = kmers[:, 0] if k <= 32 else np.array([(int(h) << 64) | int(l) for l, h in zip(kmers[:, 0], kmers[:, 1])], dtype=object)
    assert (vals == want_k).all() and (ab == want_a).all()
