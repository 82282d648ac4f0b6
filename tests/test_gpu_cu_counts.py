"""The small exact tests of the suite at forced CU counts (DSKGPU_NUM_CU, read by Tuning::read and applied in dskgpu_create).

Every persistent or grid-capped launch sizes its grid from dskgpu_ctx::num_cu, and make_plan its level-1 bins.  At the MI355X's 256 CUs
the crafted inputs of the suite -- a few KB to a few MB -- give every block exactly one tile, one sub-partition, one chunk, so the loops
inside the kernels (grid stride, work counters, "next sub-partition on the same LDS table") run once on them, and the `large` branch of
make_plan is reached only by the full-size tests.  Here the same inputs, the same checkers and the same expectations run at

    SMALL = 1, 3      every block takes several units of work (asserted per case, see LAUNCH_COVER and two_level())
    REAL  = 32, 304   a CPX partition of the MI355X (where the `large` plan starts at 2048 sub-partitions) and an MI300X, whose count is
                      no power of two: other P1 roundings, chunk counts and "one block per CU" grids

No kernel waits for another block (no sleep, no spin on a flag), so a grid sized for more or fewer CUs than the device has runs in more or
fewer rounds.  Every comparison is exact and made by the checkers the suite already has; no expectation is computed by new code.  The
switch is set with monkeypatch.setenv BEFORE the context or group is created: it is read once, at creation.

Everything runs at SMALL; section a, the path-agreement cases and the multi-word prefix runs of section b also run at REAL.  The rest of
section b and section c are SMALL only, and the partition-order contract, whose body takes 25 s, runs at 3 CUs alone.

Sections: a. the count path against the CPU oracle, b. the row order, c. the entries that read the result or a stream (lookups, read
summaries and selection, correction, threading, variants, the dense-graph battery), d. the switch is read and changes nothing.  The
conditions that keep a case from passing vacuously are asserted in the case, from stats() and the input sizes (exceeds(), two_level());
those that need only the sizes or the CPU oracle also run without a GPU (test_inputs_exceed_what_one_launch_covers).  The one launch site
whose load no statistic reports, k_ovs_gather, is read off the library's own trace (DSKGPU_VERBOSE).
"""
import re

import numpy as np
import pytest

from tests import byte_streams as B
from tests import crafted_keys as ck
from tests import test_gpu_abundance_edges as AE
from tests import read_summary_model as RM
from tests import test_gpu_byte_values as BV
from tests import test_gpu_count_sweep as SW
from tests import test_gpu_crafted_keys as CK
from tests import test_gpu_parity as PA
from tests import test_gpu_partition_order_wide as PW
from tests.test_correct_restatement import planted_stream

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

SMALL = [1, 3]
REAL = [32, 304]
ALL = SMALL + REAL
HMAX = 10000

# What ONE launch covers at DSKGPU_NUM_CU = 1, from the launch sites (multiply by n for other counts); a case that names an entry must bring
# more than TWICE that, so that blocks go round their loop.  entry: (launch function the figure was read from, unit, units at n = 1)
LAUNCH_COVER = {
    "k_encode":         ("run_encode, dskgpu.hip: min(blocks, num_cu * 16) blocks x 256 words x 32 letters", "stream bytes", 16 * 256 * 32),
    "k_count_valid":    ("encode_current, dskgpu.hip: min(words / 256, num_cu * 8) blocks x 256 words", "packed words", 8 * 256),
    "level-1 chunks":   ("upload_descs1 -> build_descs1(..., num_cu * 8), dskgpu.hip: at most 8 n chunks of whole tiles; the histogram-free scatter walks them on "
                         "scatter_grid() = min(chunks, num_cu * per_cu) blocks, per_cu <= 2048 / SC_NT resident blocks, the exact passes on min(chunks, "
                         "num_cu): above 16 n tiles every chunk holds several tiles", "tiles", 8),
    "k_sk_count":       ("sk_sizes, dskgpu.hip: min(records / SKX_NT, num_cu * 16) chunks, one block each (also k_sk_expand)", "blocks of 256 records", 16),
    "sender":           ("sk_geometry, sender.hip: min(tiles / 8, num_cu * 8 or 9) chunks", "chunks of 8 tiles", 9),
    "query":            ("ensure_index, query.hip: k_query_build on min(rows / 256, num_cu * 32) blocks x 256 rows (the lookups, k_query_kmers and "
                         "k_query_reads, launch a block per 256 items whatever the CU count; their stream goes through k_encode)", "rows or items", 32 * 256),
    "read summaries":   ("record_grid, readsum.hip: min(blocks, num_cu * 32); k_rs_short takes 4 records per block", "blocks of 4 records", 32),
    "k_correct_rest":   ("launch_trials, correct.hip: min(candidates / 4, num_cu * 16) blocks x 4 candidates", "candidates", 16 * 4),
    "k_thread_maxsteps": ("thread.hip: min(walks / 256, num_cu * 8) blocks x 256 walks", "walks", 8 * 256),
    "k_variant_compare": ("compare, variants.hip: min(variants / 4, num_cu * 8) blocks x 4 waves", "variants", 8 * 4),
    "k_ovs_gather":     ("sort_oversize, rowsort.hip: min(listed, num_cu * 8) blocks", "listed sub-buckets", 8),
    "k_fix_runs_multi": ("sort_index_multiword, rowsort.hip: min(rows / 256, num_cu * 32) blocks x 256 rows", "rows", 32 * 256),
}
TILE_BYTES = {1: 16384, 2: 8192, 4: 4096}      # stream bytes per level-1 tile (Tile<W>::KEYS letters, kernels.h)


def exceeds(entry, units, n):
    """the condition: `units` of the entry's unit are more than twice what one launch covers at n CUs"""
    need = 2 * LAUNCH_COVER[entry][2] * n
    assert units > need, f"{entry}: {units} {LAUNCH_COVER[entry][1]}, one launch at {n} CUs covers {need // 2} ({LAUNCH_COVER[entry][0]})"


RECORD_WORDS = {31: 2, 63: 3}                  # 64-bit words of a super-k-mer record (k <= 45: 2)


def sender_chunks(nbytes):
    """sk_geometry, sender.hip: the encoded stream in groups of 16 window ends, tiles of SK_NT - SK_HALO = 508 groups, 8 tiles a chunk"""
    ngroups = (nbytes + 31) // 32 * 2
    return (ngroups + 507) // 508 // 8


def count_input_loops(nbytes, k, n):
    """a count of a stream of nbytes from the reads: the encode, the valid-window count and the level-1 chunks go round"""
    exceeds("k_encode", nbytes, n)
    exceeds("k_count_valid", nbytes // 32, n)
    exceeds("level-1 chunks", nbytes // TILE_BYTES[ck.key_words(k)], n)


def two_level(st, n):
    """a count labelled two-level: the count kernels launch min(F, 2 * num_cu) blocks, so every block counts more than one sub-partition"""
    assert st["n_levels"] == 2 and st["n_final_bins"] > 2 * n, (n, st)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


class Once:
    """the oracle with the count of every (stream bytes, k) kept across the CU counts (the bodies of tests/test_gpu_parity.py count their
    reference at every call); everything else is the oracle's"""
    kept = {}

    def __init__(self, oracle):
        self.oracle = oracle

    def count(self, stream, k):
        s = np.ascontiguousarray(stream, dtype=np.uint8)
        key = (len(s), hash(s.tobytes()), k)
        if key not in Once.kept:
            Once.kept[key] = self.oracle.count(stream, k)
        return Once.kept[key]

    def __getattr__(self, name):
        return getattr(self.oracle, name)


@pytest.fixture
def once(oracle):
    return Once(oracle)


def force(monkeypatch, n):
    monkeypatch.setenv("DSKGPU_NUM_CU", str(n))


# ------------------------------------------------------------------ the streams of section a (made once)
RANDOM_READS = {"all_distinct": 32_000, "mixed": 32_000, "cpx": 52_000}      # reads of SW.RL = 150 bases, one per line
_streams = {}


def stream_of(name):
    if name not in _streams:
        rng = np.random.default_rng(11)
        _streams[name] = (SW.genome_reads(rng, 32_000, 32_000 * SW.RL // 3, 0.01) if name == "mixed"
                          else SW.random_reads(rng, RANDOM_READS[name]))
    return _streams[name]


def stream_bytes(name):
    return RANDOM_READS[name] * (SW.RL + 1)


def counted(once, dev, name, k, amin):
    """one count of a random-read stream, exact against the oracle (AE.check_exact: rows in the oracle's order, abundances, the whole
    histogram, n_kmers, n_distinct, n_solid) -> what AE.run_count returns"""
    stream = stream_of(name)
    got = AE.run_count(AE.device_bytes("cu_counts_" + name, stream, dev), k, amin, AE.MAX, HMAX)
    AE.check_exact(once.count(stream, k), k, got, amin, AE.MAX, HMAX)
    return got


# ------------------------------------------------------------------ the conditions that need only the input sizes (no GPU)
def test_inputs_exceed_what_one_launch_covers(oracle):
    for n in SMALL:
        for name in RANDOM_READS:
            for k in (31, 63, 97):
                count_input_loops(stream_bytes(name), k, n)
        for name, (k, n_reads, _) in AE.STREAMS.items():
            if name.endswith("_two"):
                count_input_loops(n_reads * (AE.RL + 1), k, n)
        count_input_loops(AE.HEAVY_JUNK + AE.HEAVY_READS * (AE.RL + 1) + AE.HEAVY_TAIL, 63, n)
        for k in (31, 32, 64, 127):
            count_input_loops(ck.CROWD_READS[k] * (ck.READ_LEN + 1), k, n)
        for k in B.COUNT_KS:
            count_input_loops(len(byte_value_stream(k, n)), k, n)
        count_input_loops(60_000 * 151, 63, n)                                   # the reads of the row-sort and fallback bodies (synth.make_reads)
        count_input_loops(250_000 * 151, 31, n)                                  # the reads of the partition-order contract
        count_input_loops(ck.CROWD_READS[63] * (ck.READ_LEN + 1), 63, n)
        exceeds("k_fix_runs_multi", 60_000 - 100 + 1, n)                         # the multi-word rows of section b: >= the k-mers of the noise record
        exceeds("k_fix_runs_multi", merge_rows_sorted(oracle, 41), n)            # the union sort of the three banks
        exceeds("sender", sender_chunks(60_000 * 151 // 2), n)                   # the record path: two ranks, every second read each
        for k in (31, 63, 97):                                                   # section c
            exceeds("query", RANDOM_READS["all_distinct"] * (SW.RL - k + 1) * 9 // 10, n)      # rows: random 150-mers, all but a handful distinct
        exceeds("k_encode", 1_000_003, n)
        exceeds("query", 4 ** 8, n)
        exceeds("read summaries", 1200 // 4, n)
        exceeds("k_correct_rest", 3 * planted_stream(31)[2], n)                  # a candidate per planted substitution at the least
        exceeds("k_correct_rest", 3 * planted_stream(63)[2], n)
        exceeds("k_variant_compare", 240, n)
        exceeds("k_thread_maxsteps", 24_000 * 6 // 10, n)                        # (T.test_every_window_a_walk_head places more than 3072 of 5000 fragments)
    # the plans the two-level cases expect, from the restated planner (checked against stats() on the device)
    for n in ALL:
        for name, k in (("all_distinct", 31), ("all_distinct", 63), ("all_distinct", 97)):
            keys = RANDOM_READS[name] * (SW.RL - k + 1)
            levels, p1, p2 = ck.make_plan(keys + 1, 0, ck.key_words(k), n)
            assert levels == 2 and p1 * p2 > 2 * n and p1 >= 2
    levels, p1, p2 = ck.make_plan(RANDOM_READS["cpx"] * (SW.RL - 31 + 1) + 1, 0, 1, 32)
    assert levels == 2 and p1 * p2 >= 64 * 32 and p1 == 32 and p2 % 2 == 1      # the `large` branch: one segment per CU, odd P2


# ------------------------------------------------------------------ d. the switch is read, and it changes nothing
@gpu
def test_the_switch_is_read_and_changes_nothing(once, dev, monkeypatch):
    """k = 31, two levels: the count at the device's own CU count and at every forced one returns byte-identical rows, abundances and
    histogram; n_final_bins at 1 and 3 differs from the default run's and is a multiple of the forced count -- the variable reached make_plan."""
    monkeypatch.delenv("DSKGPU_NUM_CU", raising=False)
    rows0, ab0, hist0, st0, _ = counted(once, dev, "all_distinct", 31, 1)
    assert st0["n_levels"] == 2
    for n in ALL:
        force(monkeypatch, n)
        rows, ab, hist, st, _ = counted(once, dev, "all_distinct", 31, 1)
        assert rows.tobytes() == rows0.tobytes() and ab.tobytes() == ab0.tobytes() and hist.tobytes() == hist0.tobytes(), n
        two_level(st, n)
        keys = st["n_kmers"]
        assert st["n_final_bins"] == np.prod(ck.make_plan(keys + 1, 0, 1, n)[1:]), (n, st)      # the restated planner at this count
        if n in SMALL:
            assert st["n_final_bins"] != st0["n_final_bins"] and st["n_final_bins"] % n == 0, (n, st, st0)
    for bad in ("0", "1025", "-3", "x"):                                                        # out of range: the device's own count
        monkeypatch.setenv("DSKGPU_NUM_CU", bad)
        st = counted(once, dev, "all_distinct", 31, 1)[3]
        assert st["n_final_bins"] == st0["n_final_bins"], (bad, st)


# ------------------------------------------------------------------ a. the count path against the CPU oracle
@gpu
@pytest.mark.parametrize("n", ALL)
@pytest.mark.parametrize("name,amin", [("all_distinct", 1), ("mixed", 2)])
@pytest.mark.parametrize("k", [31, 63, 97])
def test_two_level_random_reads(once, dev, monkeypatch, k, name, amin, n):
    """k_count1v3, k_count2v3, k_count_mw<4, true> with several sub-partitions per block on one LDS table; the segment work counter of
    level 2 starting at min(P1, n)"""
    force(monkeypatch, n)
    st = counted(once, dev, name, k, amin)[3]
    two_level(st, n)


@gpu
@pytest.mark.parametrize("n", [3, 5, 12])
def test_level_one_holds_with_a_short_last_chunk(once, dev, monkeypatch, n):
    """With 8 n level-1 chunks and the last one short, the blocks that walk only full chunks take more of the input than chunks / grid
    says -- at 3 CUs this stream is 295 tiles in 23 chunks of 13, block 0 walks 104 / 295 = 35.25 % against 8 / 23 = 34.78 % -- and
    more than the 1 % of room of the level-1 slices: sized from chunks / grid, level 1 overflowed and the count went through the
    histogram passes of the exact path.  Sized from the chunk descriptors (busiest_share1, planning.h) it holds: no "hist1" / "hist2"
    stage, no retry.  (tests/host/test_planning.cpp has the same witness on the CPU.)"""
    force(monkeypatch, n)
    got = counted(once, dev, "all_distinct", 31, 1)
    st, stages = got[3], got[4]
    two_level(st, n)
    assert st["n_retries"] == 0 and "hist1" not in stages and "hist2" not in stages, (st, sorted(stages))


@gpu
def test_the_large_plan_of_a_cpx_partition(once, dev, monkeypatch):
    """32 CUs: the `large` branch of make_plan from 2048 sub-partitions on -- P1 = the CU count, a wide odd P2"""
    force(monkeypatch, 32)
    st = counted(once, dev, "cpx", 31, 2)[3]
    assert st["n_levels"] == 2 and st["n_final_bins"] >= 64 * 32 and st["n_final_bins"] % 32 == 0 and (st["n_final_bins"] // 32) % 2 == 1, st


# (k97_two has no w5 and no w9: a four-word region holds 1090 keys and has no chains, so AE plants 100, 200 and 300 there and nothing at 512 or
# 5120 -- AE.require_edges refuses those windows on it.  Its own windows are w1 and the planted 200, as in AE.W_K97_TWO.)
PLANTED = ([(s, w) for s in ("k31_two", "k63_two") for w in ("w1_1_max_h10000", "w5_2_512_h512", "w9_5120_5120_h5120")]
           + [("k97_two", "w1_1_max_h10000"), ("k97_two", "w200_200_200_h200")])


@gpu
@pytest.mark.parametrize("n", ALL)
@pytest.mark.parametrize("name,window", PLANTED, ids=AE.case_ids(PLANTED))
def test_planted_abundance_edges(once, dev, monkeypatch, name, window, n):
    """the ballot-counted singletons, the CNT_LH boundary and the k-mer the chained kernels count (tests/test_gpu_abundance_edges.py)"""
    force(monkeypatch, n)
    st, stages = AE.planted_case(once, dev, name, window)
    AE.histogram_free(st, stages, AE.STREAMS[name][0])
    two_level(st, n)


@gpu
@pytest.mark.parametrize("n", ALL)
@pytest.mark.parametrize("window", list(AE.HEAVY_WINDOWS))
@pytest.mark.parametrize("k", [31, 63])
def test_heavy_kmer_counted_apart(once, dev, monkeypatch, k, window, n):
    """the poly-A tail of AE.heavy_stream: one k-mer with a million occurrences, counted apart by the level-1 scatter at REAL (n_heavy 1,
    as in AE.test_heavy_rows).  At SMALL the plan has two or three level-1 bins, find_heavy's "1.2 x the median bin" has no median to
    stand on and the k-mer is not counted apart (measured: n_heavy 0 at one CU): it goes through the chain of extension regions
    instead -- a million keys through k_count_chained / k_count_chained_mw on two blocks -- with the same exact result."""
    force(monkeypatch, n)
    st = AE.heavy_case(once, dev, k, window)
    two_level(st, n)
    if n in REAL:
        assert st["n_heavy"] == 1, st
    else:
        assert st["n_heavy"] == 1 or st["n_ext_regions"] > 0, st


# Two-word keys at SMALL: the `large` branch gives F = ceil(keys / 2560) sub-partitions with nothing to spare, the crowd's 63-mers are all
# distinct, and k_count2v3's table holds 2688 of them: a few of the ~1070 sub-partitions exceed it, the pass is repeated with twice the
# sub-partitions (n_retries 1, exact rows), and the crafted family no longer sits where the restated plan puts it.  The balanced split
# of 256 CUs -- and of 32 and 304, whose `large` branch starts above these inputs -- leaves 2 % more room and stays below the limit.
# So the k = 63 cases run at REAL, and k = 64 (index table, 3584 keys) stands for the width at SMALL.
CROWD = [(k, n) for k in (31, 64, 127) for n in ALL] + [(63, n) for n in REAL]


@gpu
@pytest.mark.parametrize("hi32", [0xFFFFFFFF, 0])
@pytest.mark.parametrize("k,n", CROWD)
def test_crafted_family_in_a_crowd(once, dev, monkeypatch, k, hi32, n):
    """hundreds of k-mers with one home slot in the first / last sub-partition of a two-level count (tests/test_gpu_crafted_keys.py; the
    restated plan follows the forced count: crafted_keys.plan_num_cu)"""
    force(monkeypatch, n)
    CK.test_family_in_a_crowd(once, dev, k, hi32)
    assert np.prod(ck.make_plan(ck.crowd_kmers(k) + 1, 0, ck.key_words(k))[1:]) > 2 * n


@gpu
@pytest.mark.parametrize("k,n", [(32, n) for n in ALL] + [(63, n) for n in REAL])
def test_crafted_family_outgrows_its_region(once, dev, monkeypatch, k, n):
    force(monkeypatch, n)
    CK.test_family_outgrows_its_region(once, dev, k)


@gpu
@pytest.mark.parametrize("n", REAL)
def test_crafted_twins_in_the_crowd(once, dev, monkeypatch, n):
    """the twins are 63-mers in the same crowd: at SMALL the first plan is repeated for the crowd alone (above), and the body's "exactly
    one re-count" (n_retries == 1, the twins') no longer holds -- REAL only, like the other k = 63 bodies; at SMALL the case below"""
    force(monkeypatch, n)
    CK.test_twins_in_the_crowd(once, dev)


@gpu
@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("fam", ["last", "first", "twins"])
def test_crafted_63mers_with_the_retry_allowed(once, dev, monkeypatch, fam, n):
    """k = 63 at SMALL: the same crowd with the same crafted families spread through it (160 members on the last home slot of k_count2v3
    in the last / first sub-partition; the 300 twins), counted exactly -- rows, abundances, histogram and totals by CK.check against the
    oracle's rows of the crowd merged with the family's.  Where the family lands and how often the pass is repeated is left open: a
    `large` plan of 1 or 3 CUs has no spare sub-partitions (see above), so up to two repeats are allowed, and each is a finer plan."""
    from dsk_amd import KmerCounter
    force(monkeypatch, n)
    k = 63
    crowd, bw, bab, btotal = CK.crowd_of(once, k)
    members = ck.twin_family(k) if fam == "twins" else ck.crowd_family(k, 0xFFFFFFFF if fam == "last" else 0)[:160]
    fam_ab = ck.abundances(len(members))
    stream = ck.spread(crowd, ck.READ_LEN + 1, ck.records_of(members.text, fam_ab, np.random.default_rng(ck.seed_of("in crowd", k, len(members)))))
    count_input_loops(len(stream), k, n)
    words, ab = ck.merge_rows(bw, bab, members.words, fam_ab)
    assert len(ab) == len(bab) + len(members)
    for amin, po in ((1, False), (2, True)):
        with KmerCounter(kmer_size=k, abundance_min=amin, partition_order=po, timing=True) as kc:
            got = CK.count_on(kc, stream, dev, po)
        st = CK.check(got, words, ab, btotal + int(fam_ab.sum()), amin)
        print("k = 63 at", n, "CUs:", fam, "n_retries", st["n_retries"], "n_final_bins", st["n_final_bins"])
        two_level(st, n)
        assert st["n_retries"] <= 2, st


_reads60k = {}


def reads60k(dev):
    """the 60 000 reads of the fallback tests of tests/test_gpu_parity.py"""
    if "r" not in _reads60k:
        from dsk_amd import synth
        _reads60k["r"] = synth.make_reads(synth.make_genome(300_000, dev), 60_000, 150).cpu().numpy()
    return _reads60k["r"]


@gpu
@pytest.mark.parametrize("n", ALL)
@pytest.mark.parametrize("switch", ["DSKGPU_NO_OPT1", "DSKGPU_NO_OPT2", "DSKGPU_NO_ALIGNED"])
@pytest.mark.parametrize("k", [31, 63])
def test_exact_fallbacks(once, dev, monkeypatch, k, switch, n):
    """k_hist on a num_cu grid, k_plan, k_final_offsets and plain k_scatter"""
    force(monkeypatch, n)
    monkeypatch.setenv(switch, "1")
    if switch == "DSKGPU_NO_ALIGNED":
        monkeypatch.setenv("DSKGPU_NO_OPT2", "1")      # the key-array scatter of the exact level 2, with the plain write-out
    reads = reads60k(dev)
    if n in SMALL:
        count_input_loops(len(reads), k, n)
    st = PA.check_against_oracle(once, reads, k, dev)
    two_level(st, n)


@gpu
@pytest.mark.parametrize("n", ALL)
@pytest.mark.parametrize("k", [31, 63])
def test_finer_partition_retry(once, dev, monkeypatch, k, n):
    """DSKGPU_TABLE_MAXLOAD: the first plan overflows, the pass is repeated with a finer one (PA.test_table_overflow_retry_partitions_finer)"""
    force(monkeypatch, n)
    reads = reads60k(dev)
    if n in SMALL:
        count_input_loops(len(reads), k, n)
    st = PA.finer_partition_retry_case(once, reads, k, dev, monkeypatch)
    two_level(st, n)


@gpu
@pytest.mark.parametrize("n", ALL)
@pytest.mark.parametrize("level0", [True, False])
@pytest.mark.parametrize("k", [31, 63])
def test_multi_pass(once, dev, monkeypatch, k, level0, n):
    """several passes over the key space (max_pass_mkeys), with the level-0 sweep and with every pass generating its keys again"""
    force(monkeypatch, n)
    if not level0:
        monkeypatch.setenv("DSKGPU_NO_LEVEL0", "1")
    reads = reads60k(dev)
    if n in SMALL:
        count_input_loops(len(reads), k, n)
    st = PA.check_against_oracle(once, reads, k, dev, max_pass_mkeys=1)
    assert st["n_passes"] > 1
    assert n in REAL or st["n_final_bins"] > 2 * n, st      # (a pass of a million keys may plan one level: its count kernels still launch min(F, 2 n) blocks)


@gpu
@pytest.mark.parametrize("n", ALL)
@pytest.mark.parametrize("k", [31, 63])
def test_record_path_of_two_ranks(once, golden_dir, dev, monkeypatch, k, n):
    """the super-k-mer records: two contexts on one device with the exchange done by hand, then the in-process group of two ranks
    (contexts created by group.hip).  REAL: the golden reads of the two bodies.  SMALL: the 60 000 reads, so that every rank's sender
    walks more than two rounds of chunks and every receiver's k_sk_count blocks more than two rounds of 256 records (asserted from the
    shard's bytes and the words received)."""
    force(monkeypatch, n)
    if n in REAL:
        PA.test_multi_gpu_path_on_one_device(once, golden_dir, dev, 2, k, False)
        PA.test_group_count_in_one_process(once, golden_dir, dev, monkeypatch, 2, k, "copy", False)
        return
    reads = reads60k(dev)
    for shard_bytes, words_received in PA.multi_gpu_path_case(once, reads, dev, 2, k, False):
        exceeds("sender", sender_chunks(shard_bytes), n)
        exceeds("k_sk_count", words_received // RECORD_WORDS[k] // 256, n)
    PA.group_count_case(once, reads, monkeypatch, 2, k, "copy", False)      # (the same shards: every second read)


_bv = {}


def byte_value_stream(k, n):
    """the byte-value stream of tests/byte_streams.py, repeated (a newline between the copies) until the encode of n CUs goes round"""
    if (k, n) not in _bv:
        s = BV.all_stream(k)
        reps = 2 * LAUNCH_COVER["k_encode"][2] * min(n, 3) // len(s) + 2
        _bv[(k, n)] = np.concatenate([np.concatenate([s, np.array([B.NL], np.uint8)]) for _ in range(reps)]).astype(np.uint8)
    return _bv[(k, n)]


@gpu
@pytest.mark.parametrize("n", ALL)
@pytest.mark.parametrize("k", B.COUNT_KS)
def test_byte_values_through_the_count(once, dev, monkeypatch, k, n):
    """every byte value through k_encode on a looping grid: BV.test_count_matches_oracle on the repeated stream (its expectations are the
    oracle's on the same bytes)"""
    force(monkeypatch, n)
    s = byte_value_stream(k, n)
    if n in SMALL:
        count_input_loops(len(s), k, n)
    monkeypatch.setattr(BV, "all_stream", lambda kk: s)
    BV.test_count_matches_oracle(once, dev, k, False)


# ------------------------------------------------------------------ b. the row order
def watch(monkeypatch):
    """-> a list that receives (stream bytes, k, stats) of every count a body of tests/test_gpu_parity.py checks against the oracle"""
    seen, inner = [], PA.check_against_oracle

    def checked(oracle, stream, k, dev, *a, **kw):
        st = inner(oracle, stream, k, dev, *a, **kw)
        seen.append((len(stream), k, st))
        return st
    monkeypatch.setattr(PA, "check_against_oracle", checked)
    return seen


def sorts_loop(seen, n, least):
    """every count of the body: its input goes round the encode, the valid-window count and the level-1 chunks; the row sort's first
    step cuts the rows into a multiple of n chunks of at most 64 K rows (step_a_chunks), so rows above 2 x 65536 n are more than two rounds"""
    assert len(seen) >= least, len(seen)
    for nbytes, k, st in seen:
        count_input_loops(nbytes, k, n)
    assert max(st["n_solid"] for _, _, st in seen) > 2 * 65536 * n


@gpu
@pytest.mark.parametrize("n", ALL)
def test_row_sort_paths_agree(once, dev, monkeypatch, n):
    force(monkeypatch, n)
    seen = watch(monkeypatch)
    PA.test_row_sort_paths_agree(once, dev, monkeypatch)
    if n in SMALL:
        sorts_loop(seen, n, 15)


@gpu
@pytest.mark.parametrize("n", ALL)
def test_two_word_row_sort_paths_agree(once, dev, monkeypatch, n):
    force(monkeypatch, n)
    seen = watch(monkeypatch)
    PA.test_two_word_row_sort_paths_agree(once, dev, monkeypatch)
    if n in SMALL:
        sorts_loop(seen, n, 15)


@gpu
@pytest.mark.parametrize("n", SMALL)
def test_oversize_sub_buckets_go_round_again(once, dev, monkeypatch, capfd, n):
    """k_ovs_gather / k_ovs_scatter on min(listed, 8 n) blocks, with every sub-bucket above 64 rows listed (DSKGPU_RS_BLOCK_ROWS, as in
    PA.test_row_sort_paths_agree, which takes 512).  That body's skewed stream -- poly-A with sparse errors in front of 60 000 reads --
    lists 28 sub-buckets (47 in its second round at 64 rows), short of two launches at 3 CUs, so this is the same kind of input four
    times over: runs of A, C, AC and AG in front of the reads.  No statistic says how many were listed; the
    library's trace does (DSKGPU_VERBOSE: "row sort: N sub-bucket(s) above ..."), and the largest N must exceed two launches' worth."""
    force(monkeypatch, n)
    monkeypatch.setenv("DSKGPU_RS_BLOCK_ROWS", "64")
    monkeypatch.setenv("DSKGPU_VERBOSE", "1")
    skew = skewed(dev)
    capfd.readouterr()
    st = PA.check_against_oracle(once, skew, 31, dev, amin=1)
    listed = [int(m) for m in re.findall(r"row sort: (\d+) sub-bucket", capfd.readouterr().err)]
    print("sub-buckets listed at", n, "CUs:", listed)
    assert st["sort_fallback"] == 0 and listed, (st, listed)
    exceeds("k_ovs_gather", max(listed), n)


_skew = {}


def skewed(dev):
    """four records of 1.5 M letters, each a repeated unit with 2 % substitutions -> thousands of distinct k-mers under a few 20-bit
    prefixes -- and the 60 000 reads"""
    if "s" not in _skew:
        rng = np.random.default_rng(5)
        parts = []
        for unit in (b"A", b"C", b"AC", b"AG"):
            run = np.frombuffer(unit * (1_500_000 // len(unit)), dtype=np.uint8).copy()
            hit = rng.random(run.size) < 0.02
            run[hit] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(hit.sum()))
            parts += [run, np.array([10], np.uint8)]
        _skew["s"] = np.concatenate(parts + [reads60k(dev)]).astype(np.uint8)
    return _skew["s"]


@gpu
@pytest.mark.parametrize("n", ALL)
@pytest.mark.parametrize("k", [40, 100])
def test_multiword_prefix_runs(once, dev, monkeypatch, k, n):
    """k_fix_runs_multi on min(rows / 256, 32 n) blocks and k_fix_long_runs on exactly n blocks (the crafted prefix runs, and at k = 100
    the runs of 60 and 300 equal sort keys, on 1, 3, 32 and 304 blocks).  At SMALL every count of the body has more than two launches'
    worth of rows (its inputs are 60 000 random letters and a few hundred crafted records: the encode does not go round)"""
    force(monkeypatch, n)
    seen = watch(monkeypatch)
    PA.test_multiword_row_sort_prefix_runs_and_fallback(once, dev, k)
    assert len(seen) >= 3
    if n in SMALL:
        for _, _, st in seen:
            exceeds("k_fix_runs_multi", st["n_solid"], n)


@gpu
@pytest.mark.parametrize("n", [3])
def test_partition_order_contract(once, golden_dir, dev, monkeypatch, n):
    """(the body counts 250 000 reads of 150 bases some thirty times, the golden reads once, and the reads behind 300 000 skewed
    letters: about 25 s, so it runs at one forced count only -- 3, where the chunk counts are no power of two)"""
    force(monkeypatch, n)
    count_input_loops(250_000 * 151, 31, n)
    PA.test_partition_order_is_the_reference_contract(once, golden_dir, dev, monkeypatch)


@gpu
@pytest.mark.parametrize("n", SMALL)
def test_partition_order_of_four_word_rows(once, dev, monkeypatch, n):
    """k = 101 in partition order (the checkers of tests/test_gpu_partition_order_wide.py on the mixed reads)"""
    force(monkeypatch, n)
    stream = stream_of("mixed")
    count_input_loops(len(stream), 101, n)
    res = PW.run(stream, 101, 2, dev)
    PW.check_partitioned(res, once.count(stream, 101), 101, 2)
    two_level(res[4], n)


def merge_rows_sorted(oracle, k):
    """the rows the union sort of AE.test_merge_banks orders: every bank's distinct k-mers (CPU oracle alone)"""
    streams, counted_once, _ = AE.banks_of(oracle, k)
    return sum(counted_once.count(s, k).distinct for s in streams)


@gpu
@pytest.mark.parametrize("n", SMALL)
def test_three_bank_merge(once, dev, monkeypatch, n):
    """the union sort of three banks goes through sort_index_multiword with every k-mer present up to three times: more than two
    launches' worth of rows reach k_fix_runs_multi"""
    force(monkeypatch, n)
    exceeds("k_fix_runs_multi", merge_rows_sorted(once, 41), n)
    AE.test_merge_banks(once, dev, 41, "min", 0, 256)


# ------------------------------------------------------------------ c. the entries that read the result or a stream
MAX = 2147483647
_expected_reads = {}


@gpu
@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("k,partition_order", [(31, False), (31, True), (63, False), (97, True)])
def test_lookups_in_a_large_index(once, dev, monkeypatch, k, partition_order, n):
    """query_reads and query_kmers on the result of the all-distinct reads: k_query_build walks millions of rows on 32 n blocks, the
    queried stream goes round the encode.  Expectations as in tests/test_gpu_query.py: expected_reads() (the oracle's windows looked up
    in the oracle's rows by numpy) and lookup() for values that are rows and values that are none."""
    from dsk_amd import KmerCounter
    from tests import test_gpu_query as Q
    force(monkeypatch, n)
    stream = stream_of("all_distinct")
    ref = once.count(stream, k)
    t = AE.device_bytes("cu_counts_all_distinct", stream, dev)
    with KmerCounter(kmer_size=k, abundance_min=1, partition_order=partition_order) as kc:
        kc.set_reads_device(t.data_ptr(), t.numel())
        kc.count()
        st = kc.stats()
        assert st["n_solid"] == ref.distinct
        exceeds("query", st["n_solid"], n)
        part = stream[:1_000_003]
        exceeds("k_encode", len(part), n)
        if k not in _expected_reads:
            rng = np.random.default_rng(k)
            some = np.ascontiguousarray(ref.words()[:: 37])
            none = rng.integers(0, 1 << 62, size=(70_001, some.shape[1]), dtype=np.uint64)
            values = np.concatenate([some, none])
            _expected_reads[k] = (Q.expected_reads(once, ref, part, k, 1, MAX), values, Q.lookup(ref.words(), ref.ab, values))
        want_reads, values, want_values = _expected_reads[k]
        got = Q.query_reads(kc, part, dev, 3, 1)
        bad = np.nonzero(got != want_reads)[0]
        assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], want_reads[bad[:5]])
        assert int((got != 0).sum()) == int((want_reads != 0).sum()) > len(part) // 4      # (every valid window of the counted reads is a row)
        exceeds("query", len(values), n)
        got = Q.query_kmers(kc, values, dev)
        bad = np.nonzero(got != want_values)[0]
        assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], want_values[bad[:5]])
        assert int((want_values != 0).sum()) >= len(values) - 70_001


@gpu
@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("partition_order", [False, True])
def test_exhaustive_lookups(dev, monkeypatch, partition_order, n):
    """all 4^8 values, canonical or not, through query_kmers and graph_neighbors against the dense restatement (DN.check_lookups)"""
    from tests import test_gpu_dense as DN
    force(monkeypatch, n)
    exceeds("query", 4 ** 8, n)
    with DN.count(DN.dense_stream(8, 1), dev, 8, abundance_min=1, partition_order=partition_order) as kc:
        DN.check_lookups(kc, DN.restated(kc, 8, 1, partition_order), 8, 1, dev)


@gpu
@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k,seed", [(7, 1), (9, 2), (12, 1)])
def test_dense_graph_battery(dev, monkeypatch, k, seed, partition_order, n):
    """tests/test_gpu_dense.py: check_tables (lookups, unitigs, edges, components, one round of every rule, variants), then the sequence
    of test_reads_drop_and_a_new_count (threading, correction, drop_components, a new count).  The dense inputs stay as they are: a few
    thousand rows, which no grid of 8 n or more blocks goes round on -- what they bring is every degenerate structure by the hundred;
    the looping inputs of these entries are the other cases of this section."""
    from tests import test_gpu_dense as DN
    force(monkeypatch, n)
    with DN.count(DN.dense_stream(k, seed), dev, k, abundance_min=1, partition_order=partition_order) as kc:
        DN.check_tables(kc, DN.restated(kc, k, seed, partition_order), k, seed, dev)
    DN.test_reads_drop_and_a_new_count(dev, k, seed, partition_order)


_summaries = {}


@gpu
@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("k,partition_order", [(31, False), (65, True)])
def test_read_summaries_marks_and_selection(oracle, golden_dir, dev, monkeypatch, k, partition_order, n):
    """read_summaries, read_marks and select_reads on the first 1200 golden reads against tests/read_summary_model.py, with the helpers
    of tests/test_gpu_read_summaries.py (its parity case takes 600 records: k_rs_short's 4 records a block need more than 256 n)"""
    from tests import test_gpu_read_summaries as RS
    force(monkeypatch, n)
    whole = RS.golden_part(oracle, golden_dir)[0]
    ends = np.flatnonzero(whole == RM.NL)
    part = whole[: int(ends[1199]) + 1].copy()
    with RS.count(whole, dev, k, abundance_min=2, partition_order=partition_order) as kc:
        if k not in _summaries:
            table = RS.model_of(kc, k)
            _summaries[k] = {tmin: RM.summaries(part, table, k, tmin) for tmin in (0, 3)}
        for tmin in (0, 3):
            want, want_st = _summaries[k][tmin]
            got, st = RS.summarise(kc, dev, part, tmin)
            assert st == want_st and st["n_records"] == 1200
            exceeds("read summaries", st["n_records"] // 4, n)
            RS.same_table(got, want)
            RS.check_marks(kc, dev, want, RS.data_rules(want))
        third = (np.arange(len(want)) % 3 == 1).astype(np.uint8)
        for keep in (RM.marks(want, dict(min_valid=1, median_min=int(np.median(want["median"])))), third, 1 - third):
            sel = RS.device_select(kc, dev, part, keep, 3, 5)
            exp = RM.select(part, keep)
            assert len(sel) == len(exp) and (sel == exp).all()


_corrected = {}


@gpu
@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("k,partition_order", [(31, False), (63, True)])
def test_correct_reads(dev, monkeypatch, k, partition_order, staged, n):
    """correct_reads in its default form (one thread per candidate) and with DSKGPU_CORRECT_STAGED (k_correct_first, then k_correct_rest
    on min(candidates / 4, 16 n) blocks): three copies of the planted stream of tests/test_correct_restatement.py against the string
    restatement built from the rows, trust_min 3 -- bytes, states and stats (C.same); every copy comes out as the error-free stream"""
    from tests import test_gpu_correct as C
    force(monkeypatch, n)
    if staged:
        monkeypatch.setenv("DSKGPU_CORRECT_STAGED", "1")
    s, truth, plants = planted_stream(k)
    nl = np.array([10], np.uint8)
    stream = np.concatenate([s, nl, s, nl, s])
    with C.count(s, dev, k, abundance_min=1, partition_order=partition_order) as kc:
        if k not in _corrected:
            kk, ab = kc.rows()
            _corrected[k] = C.CorrectRestatement(C.row_values(kk), ab, k, 3).correct(stream)
        got = C.run(kc, dev, stream, 3)
        C.same(got, _corrected[k])
        st = got[2]
        exceeds("k_correct_rest", st["n_interior"] + st["n_head"] + st["n_tail"], n)
        assert (got[0] == np.concatenate([truth, nl, truth, nl, truth])).all() and st["n_corrected"] == st["n_gaps"] == 3 * plants


_walks = {}


@gpu
@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("partition_order", [False, True])
def test_thread_reads(oracle, golden_dir, dev, monkeypatch, partition_order, n):
    """thread_reads with every placed window a walk of its own, as in T.test_every_window_a_walk_head but 24 000 fragments instead of
    5000: k_thread_maxsteps and the walk tables on min(walks / 256, 8 n) blocks.  Expectation: the string restatement of the rows."""
    from tests import test_gpu_thread as T
    force(monkeypatch, n)
    k = 31
    golden = T.stream_of("golden", oracle, golden_dir)
    if "s" not in _walks:
        reads = [r for r in bytes(golden).split(b"\n") if len(r) >= 60]
        rng = np.random.default_rng(31)
        frags = [reads[int(r)][int(o): int(o) + k] for r, o in zip(rng.integers(0, len(reads), 24_000), rng.integers(0, 60 - k, 24_000))]
        _walks["s"] = np.frombuffer(b"\n".join(frags), dtype=np.uint8).copy()
    stream = _walks["s"]
    with T.count(golden, dev, k, abundance_min=2, partition_order=partition_order) as kc:
        exp = T.restated(kc, "golden", k, 2, partition_order)
        W = T.threaded(exp, ("cu_counts fragments", k, 2, partition_order), stream)
        assert W.stats["n_valid"] == 24_000 and W.stats["n_walks"] == W.stats["n_placed"] and W.stats["max_steps"] == 1
        st = T.check_against_restatement(kc, W, T.on_device(stream, dev))
        exceeds("k_thread_maxsteps", st["n_walks"], n)
        T.check_against_restatement(kc, W, T.on_device(stream, dev, odd=True))


_snps = {}


def snp_stream(k, n_sites, spacing):
    """two records: a random sequence and the same with a substitution every `spacing` letters -- n_sites bubbles of k rows a side"""
    if k not in _snps:
        rng = np.random.default_rng(700 + k)
        a = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(n_sites + 1) * spacing)
        b = a.copy()
        at = np.arange(1, n_sites + 1) * spacing
        b[at] = np.frombuffer(b"CGTA", dtype=np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), a[at])]
        _snps[k] = np.concatenate([a, np.array([10], np.uint8), b, np.array([10], np.uint8)])
    return _snps[k]


@gpu
@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("partition_order", [False, True])
def test_variants(dev, monkeypatch, partition_order, n):
    """variants on 250 isolated substitutions between two long records: k_variant_compare on min(variants / 4, 8 n) blocks of 4 waves.
    The golden reads of tests/test_gpu_variants.py give 134 variants at the most, short of two launches at 3 CUs; this is a longer
    input of the same kind, and its expectation is the same restatement (restate() of the rows, through V.check_variants)."""
    from tests import test_gpu_variants as V
    force(monkeypatch, n)
    k = 21
    with V.count(snp_stream(k, 250, 3 * k), dev, k, abundance_min=1, partition_order=partition_order) as kc:
        exp = V.restated(("cu_counts snps", k, partition_order), kc, k, 2 * k)
        st = V.check_variants(kc, exp, 2 * k)
        exceeds("k_variant_compare", st["n_variants"], n)
        assert st["n_snps"] == st["n_variants"] >= 240      # (a random repeat of k - 1 letters may merge a site or two)
