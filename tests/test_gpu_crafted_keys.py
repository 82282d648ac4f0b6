"""Crafted hash collisions through every count table and the lookup index (tests/crafted_keys.py builds the inputs,
tests/test_crafted_keys_restatement.py shows without a GPU that they are what they claim).

Random and natural reads leave probe runs of a dozen slots; here hundreds to thousands of DIFFERENT canonical k-mers share one
sub-partition and one home slot, so the insert and sweep loops of every count kernel and the probe loop of the lookup index walk runs
of that length, at the start of the table, at its end and across its end.  Every result is compared exactly with the CPU oracle
(totals, distinct, histogram, rows, abundances), every lookup exactly with a Python dictionary of the oracle's rows.  Abundances are
1..5 by member index.  Which kernel a case reaches is asserted from stats() and the stage names:

    one level (a family alone)            k_count1<false>, k_count_mw<2 / 4, false>          n_levels == 1
    two levels, k <= 32                   k_count1v3 (regions), k_count_chained (chains)     no "hist2" stage; n_ext_regions
    two levels, k = 63                    k_count2v3, then k_count_mw<2, true> on twins      no "hist2" stage; n_retries == 1 on twins
    two levels, k = 127                   k_count_mw<4, true>                                no "hist2" stage
    two levels, k = 64 / 128              the all-ones key is a k-mer there, so the sentinel-padded regions are off
                                          (dskgpu.hip: sentinel_ok): exact offsets, k_count_mw<2 / 4, false> -- "hist2" is a stage
"""
import numpy as np
import pytest

from tests import crafted_keys as ck

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E_OVERFLOW = -5
M32 = np.uint64(0xFFFFFFFF)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


# ------------------------------------------------------------------ helpers
def count_on(kc, stream, dev, po=True):
    """count a numpy stream on an open context -> (rows ascending, abundances, histogram, stats, stage names); po: the context's
    rows are in partition order"""
    t = torch.from_numpy(np.ascontiguousarray(stream)).to(dev)
    torch.cuda.synchronize()
    kc.set_reads_device(t.data_ptr(), t.numel())
    kc.count()
    rows, ab = kc.rows()
    order = np.lexsort(rows.T) if po else np.arange(len(ab))       # (partition order: ascending inside a partition only -- compared as a sorted multiset)
    return rows[order], ab[order], kc.histogram(), kc.stats(), [n for n, _ in kc.stage_times()]


def check(got, words, ab, total, amin):
    """words / ab: every distinct k-mer of the input, ascending, with its abundance (the oracle's)"""
    rows, rab, hist, st, _ = got
    keep = ab >= amin
    exp_hist = np.zeros(10001, np.uint64)
    np.add.at(exp_hist, np.minimum(ab, 10000), 1)
    assert st["n_kmers"] == total and st["n_distinct"] == len(ab) and st["n_solid"] == int(keep.sum()), (st, total, len(ab))
    assert (hist == exp_hist).all()
    assert rows.shape == (int(keep.sum()), words.shape[1])
    assert (rows == words[keep]).all() and (rab == ab[keep]).all()
    return st


def oracle_rows(oracle, stream, k):
    ref = oracle.count(stream, k)
    return ref.words(), ref.ab, ref.total


_crowd = {}


def crowd_of(oracle, k, extra=None):
    """(stream, oracle rows, abundances, total) of the random reads of this k, counted once"""
    key = (k, extra)
    if key not in _crowd:
        s = ck.crowd_stream(k) if extra is None else np.concatenate([ck.crowd_stream(k), ck.crowd_stream(extra)])
        _crowd[key] = (s,) + oracle_rows(oracle, s, k)
    return _crowd[key]


def sub_partition_load(k, words, ab, plan, h):
    """(distinct k-mers, keys) of the rows `words` that fall into the sub-partition of the mixed word h under plan (levels, P1, P2)"""
    _, p1, p2 = plan
    hi = ck.mixed_top_np(words, k) >> np.uint64(32)
    d1 = (hi * np.uint64(p1)) >> np.uint64(32)
    d2 = (((hi * np.uint64(p1)) & M32) * np.uint64(p2)) >> np.uint64(32)
    e1, e2 = ck.digits(h, p1, p2)
    m = (d1 == np.uint64(e1)) & (d2 == np.uint64(e2))
    return int(m.sum()), int(ab[m].sum())


def fit_into_crowd(k, base_words, base_ab, base_total, fam, ab_of, max_distinct, max_keys):
    """the longest prefix of fam (a multiple of 5 members) that keeps its sub-partition within max_distinct distinct k-mers and
    max_keys keys next to the crowd's own -- from the restated plan and the restated mixers -> (members, plan)"""
    W = ck.key_words(k)
    n = len(fam)
    while n > 0:
        plan = ck.make_plan(base_total + int(ab_of(n).sum()) + 1, 0, W)
        d, keys = sub_partition_load(k, base_words, base_ab, plan, fam.h[0])
        if d + n <= max_distinct and keys + int(ab_of(n).sum()) <= max_keys:
            return n, plan
        n -= 5
    raise AssertionError("the crowd alone fills the sub-partition")


def as_dict(words, ab, amin=1, only=None):
    """rows -> abundance as a dictionary; only: the questions (rows whose word 0 is no question's are left out: millions of rows)"""
    if only is not None:
        m = np.isin(words[:, 0], only[:, 0])
        words, ab = words[m], ab[m]
    return {tuple(int(x) for x in r): int(a) for r, a in zip(words, ab) if a >= amin}


def query_kmers(kc, words, dev):
    t = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint64).view(np.int64)).to(dev)
    return kc.query_kmers_tensor(t).cpu().numpy().view(np.uint32)


def query_reads(kc, stream, dev, out_off):
    """out_off: element offset of the output pointer from its allocation (aligned / unaligned stores)"""
    buf = torch.from_numpy(np.ascontiguousarray(stream)).to(dev)
    out = torch.full((out_off + len(stream) + 64,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    kc.query_reads(buf.data_ptr(), len(stream), out.data_ptr() + 4 * out_off)
    res = out.cpu().numpy()
    assert (res[:out_off] == -7).all() and (res[out_off + len(stream):] == -7).all(), "the query wrote outside its output"
    return res[out_off: out_off + len(stream)].view(np.uint32)


def random_canonical(k, n, rng):
    nw = ck.abi_words(k)
    out = []
    while len(out) < n:
        v = int.from_bytes(rng.bytes(32), "little") & ((1 << (2 * k)) - 1)
        out.append(min(v, ck.revcomp(v, k)))
    return np.array([ck.words_of(v, nw) for v in out], dtype=np.uint64).reshape(n, nw)


# ------------------------------------------------------------------ 1. a family alone
@pytest.mark.parametrize("hi32", ck.HI32S)
@pytest.mark.parametrize("k", ck.SLOT_KS)
def test_family_alone(oracle, dev, k, hi32):
    """One level (k_count1<false>, k_count_mw<W, false>): n members with one home slot and nothing else in the table -- a run of n
    slots at the start of the table, at its end and across its end; n = 1, 2, 64, 65 (one wave and one key more), 1000 (400 at k =
    27, which has ~523 members per slot); at k = 127 / 128 also 3000, where the representatives of the keys beyond the 1024 staged
    ones are read back from HBM.  Both row orders, abundance_min 1 and 2, the same four contexts for all inputs."""
    from dsk_amd import KmerCounter
    W = ck.key_words(k)
    ns = ck.alone_ns(k) + ((3000,) if k in (127, 128) and hi32 == ck.HI32S[2] else ())
    ctxs = [(amin, po, KmerCounter(kmer_size=k, abundance_min=amin, partition_order=po, timing=True)) for amin in (1, 2) for po in (False, True)]
    try:
        for n in ns:
            for low12 in ck.alone_low12s(n):
                fam = ck.alone_family(k, n, hi32, low12)
                stream = ck.reads_of(fam.text, ck.abundances(n), np.random.default_rng(ck.seed_of(k, n, low12)))
                words, ab, total = oracle_rows(oracle, stream, k)
                assert len(ab) == n and total == int(ck.abundances(n).sum())
                plan = ck.make_plan(total + 1, 0, W)
                for amin, po, kc in ctxs:
                    st = check(count_on(kc, stream, dev, po), words, ab, total, amin)
                    assert st["n_levels"] == 1 and st["n_retries"] == 0 and st["n_final_bins"] == plan[1], (k, n, low12, amin, po, st)
    finally:
        for _, _, kc in ctxs:
            kc.close()


# ------------------------------------------------------------------ 2. the load limit at its real value
@pytest.mark.parametrize("k", [32, 64, 128])
def test_load_limit_at_its_real_value(oracle, dev, k):
    """CNT_MAXLOAD / C2_MAXLOAD = 3584 distinct keys per table, with no environment switch: 3584 members of one sub-partition are
    counted (one run of 3584 slots across the end of the table); 3585 end with DSKGPU_E_OVERFLOW after exactly three retries, since
    no finer partition separates keys with one h[63:32].  The same context then counts another stream to the oracle's rows."""
    from dsk_amd import KmerCounter, DskGpuError
    fam = ck.alone_family(k, 3585, ck.HI32S[2], 4095)
    rng = np.random.default_rng(k)
    with KmerCounter(kmer_size=k, abundance_min=2, timing=True) as kc:
        stream = ck.reads_of(fam.text[:3584], ck.abundances(3584), rng)
        words, ab, total = oracle_rows(oracle, stream, k)
        assert len(ab) == 3584
        st = check(count_on(kc, stream, dev), words, ab, total, 2)
        assert st["n_levels"] == 1 and st["n_retries"] == 0
        stream = ck.reads_of(fam.text, ck.abundances(3585), rng)
        with pytest.raises(DskGpuError) as e:
            count_on(kc, stream, dev)
        # (a failed count leaves no stats to read: the three retries are in the message -- the only exit of run_one_pass that words it
        #  so is the one taken when the fourth attempt, at extra_bits = 3, overflows as well)
        assert e.value.code == E_OVERFLOW and "hash table overflow after 3 retries" in str(e.value), str(e.value)
        with pytest.raises(DskGpuError):
            kc.stats()
        small = ck.alone_family(k, 65, ck.HI32S[2], 4095)
        stream = ck.reads_of(small.text, ck.abundances(65), rng)
        words, ab, total = oracle_rows(oracle, stream, k)
        st = check(count_on(kc, stream, dev), words, ab, total, 2)
        assert st["n_retries"] == 0


# ------------------------------------------------------------------ 3. a family in a crowd
# (distinct keys a table holds, keys a region holds) of the kernel a two-level count of this k reaches
LIMITS = {31: (3584, 4360), 32: (3584, 4360), 63: (2688, 4092), 64: (3584, 1 << 30), 127: (3584, 1090)}


def run_in_crowd(oracle, dev, k, fam, fam_ab, cases, plan, expect_regions):
    """count the crowd with fam's records spread through it, under every (abundance_min, partition_order) of cases"""
    from dsk_amd import KmerCounter
    crowd, bw, bab, btotal = crowd_of(oracle, k)
    stream = ck.spread(crowd, ck.READ_LEN + 1, ck.records_of(fam.text, fam_ab, np.random.default_rng(ck.seed_of("in crowd", k, len(fam)))))
    words, ab = ck.merge_rows(bw, bab, fam.words, fam_ab)
    assert len(ab) == len(bab) + len(fam)                        # (no member is a k-mer of the random reads)
    total = btotal + int(fam_ab.sum())
    out = []
    for amin, po in cases:
        with KmerCounter(kmer_size=k, abundance_min=amin, partition_order=po, timing=True) as kc:
            got = count_on(kc, stream, dev, po)
        st = check(got, words, ab, total, amin)
        assert st["n_levels"] == 2 and st["n_final_bins"] == plan[1] * plan[2], (st, plan)
        assert ("hist2" not in got[4]) == expect_regions, got[4]
        out.append(st)
    return out


@pytest.mark.parametrize("hi32", [0xFFFFFFFF, 0])
@pytest.mark.parametrize("k", [31, 32, 63, 64, 127])
def test_family_in_a_crowd(oracle, dev, k, hi32):
    """Two levels: random reads sized just above 1024 sub-partitions of the width, the family's records spread evenly through them.
    hi32 = 0xFFFFFFFF is the last sub-partition, 0 the first (shared with poly-A, whose mixed key is 0: three poly-A records are
    added there).  family_slot at k = 31, 32 reaches k_count1v3 and at k = 127 k_count_mw<4, true>; family_v3 (home slot 3071, the
    last) at k = 63 reaches k_count2v3.  At k = 64 the all-ones key is a k-mer, the regions are off and the count takes exact
    offsets and k_count_mw<2, false> (asserted: "hist2" is a stage).  No retry anywhere.
    The issue asked for about 400 members; a sub-partition already holds the crowd's share (about 2840 one-word, 2410 two-word, 617
    four-word keys), so the members are as many of the 400 as the table's load limit (3584; 2688 in k_count2v3) and, for four-word
    keys, which have no extension regions, the region (1090 keys) leave room for: 400 at k <= 32 and 64, 160 and 185 at k = 63,
    135 and 155 at k = 127 -- computed by the test from the restated plan and mixers, and the plan is checked against stats()."""
    _, bw, bab, btotal = crowd_of(oracle, k)
    fam = ck.crowd_family(k, hi32)
    extra = 1 if hi32 == 0 else 0                                                 # poly-A
    n, plan = fit_into_crowd(k, bw, bab, btotal + 3 * extra, fam, ck.abundances, LIMITS[k][0] - 8 - extra, LIMITS[k][1] - 8 - 3 * extra)
    assert n >= 100, n
    members, ab = fam[:n], ck.abundances(n)
    if extra:
        members = ck.Family(k, members.values + [0])
        ab = np.concatenate([ab, np.array([3], np.uint32)])
        assert ck.digits(0, plan[1], plan[2]) == ck.digits(fam.h[0], plan[1], plan[2]) == (0, 0)
    for st in run_in_crowd(oracle, dev, k, members, ab, [(1, False), (2, True)], plan, expect_regions=(k != 64)):
        assert st["n_retries"] == 0 and st["n_ext_regions"] == 0, st


@pytest.mark.parametrize("k", [32, 63])
def test_family_outgrows_its_region(oracle, dev, k):
    """600 members x 8 occurrences in the last sub-partition: with the crowd's share the sub-partition holds more keys than its region
    (4360 one-word, 4092 two-word keys), the level-2 scatter chains extension regions and k_count_chained / k_count_chained_mw<2>
    count a table with a run of 600 slots at its end -- n_ext_regions >= 1, no retry.  (The first sizes tried, 600 x 8, need no
    change: the members are cut only where the table's 3584 distinct keys would not hold them next to the crowd's.)"""
    _, bw, bab, btotal = crowd_of(oracle, k)
    fam = ck.crowd_family(k, 0xFFFFFFFF, 600)
    eight = lambda n: np.full(n, 8, np.uint32)
    n, plan = fit_into_crowd(k, bw, bab, btotal, fam, eight, 3584 - 8, 1 << 30)
    assert n >= 300
    d, keys = sub_partition_load(k, bw, bab, plan, fam.h[0])
    assert keys + 8 * n > LIMITS[k][1]                            # the region cannot hold them
    for st in run_in_crowd(oracle, dev, k, fam[:n], eight(n), [(2, False)], plan, expect_regions=True):
        assert st["n_retries"] == 0 and st["n_ext_regions"] >= 1, st


# ------------------------------------------------------------------ 4. twins in bulk
def test_twins_in_the_crowd(oracle, dev):
    """300 different 63-mers with ONE mixed top word in the crowd: k_count2v3 sees one key, its verification finds the low words
    differ, and the pass is counted once more by k_count_mw<2, true> with 300 keys on one run: exactly one re-count."""
    k = 63
    _, bw, bab, btotal = crowd_of(oracle, k)
    fam = ck.twin_family(k)
    n, plan = fit_into_crowd(k, bw, bab, btotal, fam, ck.abundances, 3584 - 8, 4092 - 8)
    assert n == 300
    for st in run_in_crowd(oracle, dev, k, fam, ck.abundances(300), [(1, False), (2, True)], plan, expect_regions=True):
        assert st["n_retries"] == 1, st


@pytest.mark.parametrize("k", [64, 128])
def test_twins_alone(oracle, dev, k):
    from dsk_amd import KmerCounter
    fam = ck.twin_family(k)
    stream = ck.reads_of(fam.text, ck.abundances(300), np.random.default_rng(k))
    words, ab, total = oracle_rows(oracle, stream, k)
    assert len(ab) == 300
    for amin, po in [(1, False), (2, True)]:
        with KmerCounter(kmer_size=k, abundance_min=amin, partition_order=po, timing=True) as kc:
            st = check(count_on(kc, stream, dev, po), words, ab, total, amin)
            assert st["n_levels"] == 1 and st["n_retries"] == 0
            asked = np.concatenate([fam.words, ck.twins(k, 50, np.random.default_rng(1), fam.h[0]).words])
            have = as_dict(words, ab, amin)
            assert (query_kmers(kc, asked, dev) == np.array([have.get(tuple(int(x) for x in r), 0) for r in asked], np.uint32)).all()


# ------------------------------------------------------------------ 5. the sentinel k-mer
def neighbours(v, k):
    """the 8 de Bruijn neighbours and every single substitution of a k-mer value, canonical"""
    mask = (1 << (2 * k)) - 1
    out = [((v << 2) | c) & mask for c in range(4)] + [(v >> 2) | (c << (2 * k - 2)) for c in range(4)]
    out += [v ^ (c << (2 * p)) for p in range(k) for c in (1, 2, 3)]
    return [min(x, ck.revcomp(x, k)) for x in out]


@pytest.mark.parametrize("k,with_top_word", [(64, False), (64, True), (128, False)])
def test_sentinel_kmer(oracle, dev, k, with_top_word):
    """The k-mer whose mixed key is all ones in every word -- the pad and empty-slot value; a context of this k runs with
    sentinel_ok = false for its sake.  Alone (four records), in the crowd, and in a count of two passes; abundance_min 1 and 3, both
    row orders; at k = 64 also next to a k-mer whose mixed TOP word alone is all ones.  Then lookups of it and of its neighbours.
    (Found by this test: in a two-level count of k = 64 or 128 the key-array sources of level 2 took the all-ones key for a pad
    whatever the k and dropped the k-mer -- four occurrences and one distinct k-mer short; they now ask DigitSpec::ones_is_key.)"""
    from dsk_amd import KmerCounter
    sent = ck.sentinel_kmer(k)
    fams = [(sent, np.array([4], np.uint32))]
    if with_top_word:
        both = ck.Family(k, sent.values + ck.top_word_sentinel(k, np.random.default_rng(2)).values)
        fams = [(both, np.array([4, 3], np.uint32))]
    nw = ck.abi_words(k)
    asked = np.array([ck.words_of(x, nw) for x in [sent.values[0]] + neighbours(sent.values[0], k)], dtype=np.uint64).reshape(-1, nw)
    for fam, fab in fams:
        recs = ck.records_of(fam.text, fab, np.random.default_rng(3))
        alone = np.frombuffer(b"".join(r + b"\n" for r in recs), dtype=np.uint8).copy()
        crowd, bw, bab, btotal = crowd_of(oracle, k)
        big, gw, gab, gtotal = crowd_of(oracle, k, k - 1)
        inputs = [(alone, fam.words[np.lexsort(fam.words.T)], fab[np.lexsort(fam.words.T)], int(fab.sum()), {}, 1),
                  (ck.spread(crowd, ck.READ_LEN + 1, recs),) + ck.merge_rows(bw, bab, fam.words, fab) + (btotal + int(fab.sum()), {}, 2),
                  (ck.spread(big, ck.READ_LEN + 1, recs),) + ck.merge_rows(gw, gab, fam.words, fab) + (gtotal + int(fab.sum()), dict(max_pass_mkeys=1), 2)]
        for stream, words, ab, total, kw, levels in inputs:
            for amin, po in [(1, False), (3, False), (3, True)] if not kw else [(3, False)]:
                with KmerCounter(kmer_size=k, abundance_min=amin, partition_order=po, timing=True, **kw) as kc:
                    st = check(count_on(kc, stream, dev, po), words, ab, total, amin)
                    assert (kw or st["n_levels"] == levels) and st["n_retries"] == 0, st
                    assert st["n_passes"] >= 2 if kw else st["n_passes"] == 1, st
                    have = as_dict(words, ab, amin, only=asked)
                    exp = np.array([have.get(tuple(int(x) for x in r), 0) for r in asked], np.uint32)
                    assert exp[0] == 4
                    assert (query_kmers(kc, asked, dev) == exp).all()


# ------------------------------------------------------------------ 6. the lookup index
@pytest.mark.parametrize("n", [300, 513, 2049])
@pytest.mark.parametrize("k", [32, 64, 128])
def test_lookup_index_on_one_run(oracle, dev, k, n):
    """The index over rows that share fingerprint (h >> 32) and home slot (low12 = 0xFFF): its build claims a run of n slots and
    every lookup walks it, taking the branch "fingerprint equal, key different, go round again" up to n times per key -- on random
    rows that branch is taken with probability 2^-32 per probe.  n = 300 / 513 / 2049 rows (abundance_min 1; plus 40 twins for two-
    and four-word keys: one 64-bit hash) give capacities of 1024 / 2048 / 8192 slots: the run crosses the end of the table at the
    first two and lies in the middle of the third.  Asked for: every member; as many members that were NOT counted (same
    fingerprint, same home slot); random k-mers; a read stream of all three at output offsets 0 and 1; then the row-number form
    (colors_add: occurrences per row); then all of it again after filter_rows dropped every second row."""
    from dsk_amd import KmerCounter
    W = ck.key_words(k)
    fam2 = ck.lookup_family(k, n)
    counted, absent = fam2[:n], fam2[n:]
    rng = np.random.default_rng(ck.seed_of("lookup test", k, n))
    if W > 1:
        tw = ck.twins(k, 80, rng, (ck.HI32S[2] << 32) | (0x5A5A5 << 12) | 0xFFF)
        counted = ck.Family(k, counted.values + tw.values[:40])
        absent = ck.Family(k, absent.values + tw.values[40:])
    cab = ck.abundances(len(counted))
    stream = ck.reads_of(counted.text, cab, rng)
    words, ab, total = oracle_rows(oracle, stream, k)
    assert len(ab) == len(counted)
    rnd = random_canonical(k, 200, rng)
    asked = np.concatenate([counted.words, absent.words, rnd])
    # the queried stream: records of the counted, the absent and random k-mers, and a few longer random reads
    recs = ck.records_of(counted.text + absent.text + [ck.text(ck.value_of(r), k) for r in rnd], np.ones(len(asked), np.uint32), rng)
    longer = ["".join(rng.choice(list("ACGT"), 150)).encode() for _ in range(8)]
    qstream = np.frombuffer(b"".join(r + b"\n" for r in recs[: len(recs) // 2] + longer + recs[len(recs) // 2:]), dtype=np.uint8).copy()
    qwords, qvalid = oracle.enumerate_words(qstream, k)
    qkeys = [tuple(int(x) for x in r[: ck.abi_words(k)]) if v else None for r, v in zip(qwords, qvalid)]
    assert sum(1 for q in qkeys if q is not None) == len(recs) + 8 * (150 - k + 1)

    def check_lookups(kc, have):
        exp = np.array([have.get(tuple(int(x) for x in r), 0) for r in asked], np.uint32)
        got = query_kmers(kc, asked, dev)
        assert (got == exp).all(), (k, n, int((got != exp).sum()))
        assert int((exp != 0).sum()) == len(have) and (exp[len(counted):len(counted) + len(absent)] == 0).all()
        exp = np.array([have.get(q, 0) if q is not None else 0 for q in qkeys], np.uint32)
        for out_off in (0, 1):
            got = query_reads(kc, qstream, dev, out_off)
            assert (got == exp).all(), (k, n, out_off, int((got != exp).sum()))

    for amin in (1, 2):
        with KmerCounter(kmer_size=k, abundance_min=amin) as kc:
            rows, rab, _, st, _ = got = count_on(kc, stream, dev)
            check(got, words, ab, total, amin)
            assert st["n_levels"] == 1 and st["n_retries"] == 0
            have = as_dict(words, ab, amin)
            check_lookups(kc, have)
            # the row-number form: occurrences of every row in the queried stream (rows in the order the context holds them)
            held, _ = kc.rows()
            kc.colors_begin(1)
            cst = kc.colors_add_tensor(torch.from_numpy(qstream.copy()).to(dev), [len(qstream)])
            occ = {}
            for q in qkeys:
                if q is not None and q in have:
                    occ[q] = occ.get(q, 0) + 1
            counts = kc.colors_rows_tensor(1)[0].cpu().numpy().view(np.uint32).reshape(-1)
            assert (counts == np.array([occ.get(tuple(int(x) for x in r), 0) for r in held], np.uint32)).all()
            assert cst["n_placed"] == sum(occ.values()) and cst["n_valid"] == sum(1 for q in qkeys if q is not None)
            # every second row dropped: the dropped ones answer 0, the kept ones their abundance
            keep = np.arange(len(held)) % 2 == 0
            assert kc.filter_rows_tensor(torch.from_numpy(keep).to(dev)) == int(keep.sum())
            kept = {tuple(int(x) for x in r): have[tuple(int(x) for x in r)] for r in held[keep]}
            assert len(kept) == int(keep.sum())
            check_lookups(kc, kept)
