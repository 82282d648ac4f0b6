"""Saved rows loaded into a context on the device (include/dskgpu.h: dskgpu_load_rows; csrc/loadrows.h).

All comparisons are exact.  Part 1 compares the device -- rows, histogram, the count's record and the load's stats -- with the restatement of
tests/load_rows_model.py (which the CPU suite checks against the oracle first) on generated inputs.  Part 2 is runs of equal rows, which the
row order had never been fed before.  Part 3 is the oracle identity on the device: the load of two counts is the count of both.  Part 4: a
restored session answers every later call as the session it was saved from.  Part 5 is the contract.  Every input stands between guard bytes and
is checked unchanged after the call.

Every test here fails before the feature: KmerCounter has no load_rows and the library no dskgpu_load_rows.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import load_rows_model as M      # noqa: E402
from tests.test_gpu_unitigs import count      # noqa: E402
from tests.test_load_rows_restatement import joined, stream_of      # noqa: E402

E_ARG, E_STATE = -1, -4
GUARD, FILL = 64, 0xEE
AMAX = 2147483647
KS = (1, 2, 5, 16, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128)
NS = (1, 2, 63, 64, 65, 255, 256, 257, 4097, 70001)
ORDERS = ("shuffled", "ascending", "descending")
RULES = ("sum", "max", "min", "unique")
FILTERS = ((1, AMAX), (2, AMAX), (3, 7))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


# ------------------------------------------------------------------ one call, guard bytes round both inputs
def guarded_input(dev, arr):
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    t = torch.full((len(raw) + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    t[GUARD: GUARD + len(raw)] = torch.from_numpy(raw.copy()).to(dev)
    assert (t.data_ptr() + GUARD) % 8 == 0
    return t, raw


def unchanged(t, raw):
    b = t.cpu().numpy()
    assert (b[:GUARD] == FILL).all() and (b[GUARD + len(raw):] == FILL).all(), "guard bytes"
    assert (b[GUARD: GUARD + len(raw)] == raw).all(), "the input is left as it was"


def device_load(kc, dev, kmers, ab, combine="sum"):
    """kmers: uint64[n, words], ab: uint32[n] -> the load's stats; the inputs are checked unchanged, errors included"""
    kmers, ab = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1, kc.words), np.ascontiguousarray(ab, dtype=np.uint32)
    tk, rk = guarded_input(dev, kmers)
    ta, ra = guarded_input(dev, ab)
    torch.cuda.synchronize()
    try:
        return kc.load_rows(tk.data_ptr() + GUARD, ta.data_ptr() + GUARD, len(ab), combine)
    finally:
        torch.cuda.synchronize()
        unchanged(tk, rk)
        unchanged(ta, ra)


def same_as_model(kc, k, want, st=None, nb_partitions=4):
    rows, rab, hist, wst = want
    kk, ab = kc.rows()
    assert kk.shape == (len(rows), kc.words) and (kk == M.words_of(rows, k)).all(), "rows"
    assert (ab == rab).all(), "abundances"
    assert (kc.histogram() == hist).all(), "histogram"
    rec = kc.stats()
    fallback = rec.pop("sort_fallback")
    assert fallback in (0, 1)
    assert rec == {"n_bytes": 0, "n_kmers": wst["n_kmers"], "n_distinct": wst["n_distinct"], "n_solid": wst["n_rows"], "n_partitions": nb_partitions, "n_levels": 0,
                   "n_final_bins": 0, "n_retries": 0, "n_passes": 0, "n_ext_regions": 0, "n_heavy": 0, "n_read_sweeps": 0}
    n = len(rows)
    assert kc.partition_offsets().tolist() == [n * p // nb_partitions for p in range(nb_partitions + 1)]
    if st is not None:
        assert st == wst
    return fallback


def load_and_check(dev, k, values, ab, combine, amin=1, amax=AMAX, **kw):
    from dsk_amd import KmerCounter
    want = M.load(values, ab, k, combine, amin, amax)
    assert len(want) == 4, want
    with KmerCounter(kmer_size=k, abundance_min=amin, abundance_max=amax, **kw) as kc:
        st = device_load(kc, dev, M.words_of(values, k), ab, combine)
        return same_as_model(kc, k, want, st), st


# ------------------------------------------------------------------ generated inputs
def n_canonical(k):
    return (4 ** k + (4 ** (k // 2) if k % 2 == 0 else 0)) // 2


def palindromes(k, how_many, rng):
    """values of an even k that are their own reverse complement: a half followed by its reverse complement"""
    h = k // 2
    halves = range(4 ** h) if 4 ** h <= how_many else {int.from_bytes(rng.bytes(32), "little") % 4 ** h for _ in range(how_many)}
    return [(x << (2 * h)) | M.revcomp(x, h) for x in halves]


def pool(k, n, rng):
    """n distinct canonical values of k (all of them when there are no more), the palindromes of an even k among them"""
    if k <= 5:
        return sorted({M.canonical(v, k) for v in range(4 ** k)})[: max(n, n_canonical(k))]
    out = set(palindromes(k, max(1, n // 8), rng)[:n]) if k % 2 == 0 else set()
    while len(out) < n:
        out.add(M.canonical(int.from_bytes(rng.bytes(32), "little") % 4 ** k, k))
    return sorted(out)


def generated(k, n, order, combine, seed):
    rng = np.random.default_rng(seed)
    distinct_only = order != "shuffled" or combine == "unique"
    if distinct_only:
        values = pool(k, n, rng)[:n] if k > 5 else pool(k, n, rng)
        values = values[:n]
    else:
        base = pool(k, max(1, (n * 2) // 3), rng)
        values = [base[i] for i in rng.integers(0, len(base), n)]
        for v in base[: n]:                                      # every value of the pool at least once while it fits
            values[int(rng.integers(0, n))] = v
    if order == "ascending":
        values = sorted(values)
    elif order == "descending":
        values = sorted(values, reverse=True)
    else:
        values = [values[i] for i in rng.permutation(len(values))]
    ab = rng.integers(1, 13, len(values)).astype(np.uint32)
    if len(ab) > 3:
        ab[int(rng.integers(0, len(ab)))] = 0x7FFFFFF0               # one abundance near the top of the default filter
    return values, ab


# a sample of the product in which every value of every axis occurs, then the large shuffled inputs with repeats at every key width
CASES = [(KS[i % len(KS)], NS[(i * 3 + i // len(NS)) % len(NS)], ORDERS[i % 3], RULES[(i + i // 4) % 4], FILTERS[(i // 2) % 3]) for i in range(42)]
CASES += [(31, 70001, "shuffled", "sum", FILTERS[1]), (33, 70001, "shuffled", "sum", FILTERS[0]), (65, 70001, "shuffled", "max", FILTERS[2]),
          (96, 70001, "shuffled", "sum", FILTERS[1]), (128, 4097, "shuffled", "min", FILTERS[1]), (64, 4097, "shuffled", "sum", FILTERS[0]),
          (5, 70001, "shuffled", "sum", FILTERS[2]), (16, 70001, "shuffled", "unique", FILTERS[0])]


def test_the_sample_covers_every_value_of_every_axis():
    for axis, values in enumerate((KS, NS, ORDERS, RULES, FILTERS)):
        assert {c[axis] for c in CASES} == set(values), axis
    assert any(c[2] == "shuffled" and c[3] != "unique" and c[1] >= 4097 for c in CASES)
    for k in (2, 16, 32, 64, 96, 128):
        pal = palindromes(k, 8, np.random.default_rng(k))
        assert pal and all(M.revcomp(p, k) == p for p in pal)
    assert n_canonical(1) == 2 and n_canonical(2) == 10 and n_canonical(5) == 512
    for k in (1, 2, 5):
        assert len(pool(k, 1, np.random.default_rng(0))) == n_canonical(k)       # small k: ALL canonical k-mers


@pytest.mark.parametrize("k,n,order,combine,filt", CASES, ids=["k%d-n%d-%s-%s-%d_%d" % (c[0], c[1], c[2], c[3], c[4][0], min(c[4][1], 99)) for c in CASES])
def test_against_the_model(dev, k, n, order, combine, filt):
    values, ab = generated(k, n, order, combine, 1000 * k + n)
    if k <= 5 and (order != "shuffled" or combine == "unique"):
        assert len(values) == min(n, n_canonical(k))
    else:
        assert len(values) == n
    _, st = load_and_check(dev, k, values, ab, combine, *filt)
    if order == "ascending":
        assert st["sorted_input"] == 1
    if order == "descending" and len(values) > 1:
        assert st["sorted_input"] == 0


@pytest.mark.parametrize("k", (1, 2, 5))
def test_all_canonical_kmers_of_a_small_k(dev, k):
    values = pool(k, 1, np.random.default_rng(k))
    assert len(values) == n_canonical(k)
    rng = np.random.default_rng(7 + k)
    many = [values[i] for i in rng.integers(0, len(values), 4097)] + values
    load_and_check(dev, k, many, rng.integers(1, 5, len(many)).astype(np.uint32), "sum", 2)
    load_and_check(dev, k, values[::-1], np.arange(1, len(values) + 1, dtype=np.uint32), "unique", 1)


# ------------------------------------------------------------------ runs of equal rows
RUNS = (1, 2, 63, 64, 65, 256, 257, 1025, 70000)
_others = {}


def others(k):
    if k not in _others:
        _others[k] = pool(k, 5001, np.random.default_rng(50 + k))
    return _others[k]


@pytest.mark.parametrize("length", RUNS)
@pytest.mark.parametrize("k", (31, 63, 96))
def test_a_run_of_one_value_first_last_and_in_the_middle(dev, k, length, record_property):
    base = others(k)
    rng = np.random.default_rng(length + k)
    for place, at in (("first", 0), ("last", 5000), ("middle", 2500)):
        rest = base[:at] + base[at + 1:]                         # 5000 distinct others; the run's value is their first / last / middle neighbour
        values = [base[at]] * length + rest
        ab = rng.integers(1, 9, len(values)).astype(np.uint32)
        perm = rng.permutation(len(values))
        fb, st = load_and_check(dev, k, [values[i] for i in perm], ab[perm], "sum", 2)
        record_property("sort_fallback_%s" % place, fb)              # whatever it is: recorded, not asserted
        assert st["n_distinct"] == 5001 and st["n_in"] == 5000 + length


@pytest.mark.parametrize("k", (31, 63, 96))
def test_70000_copies_saturate_one_value(dev, k):
    base = others(k)[:300]
    values = [base[7]] * 70000 + base[:7] + base[8:]
    ab = np.array([1 << 20] * 70000 + [3] * 299, dtype=np.uint32)
    perm = np.random.default_rng(k).permutation(len(values))
    _, st = load_and_check(dev, k, [values[i] for i in perm], ab[perm], "sum", 1, 0xFFFFFFFF)
    assert st["n_saturated"] == 1 and st["n_kmers"] == 70000 * (1 << 20) + 3 * 299 and st["n_rows"] == 300
    from dsk_amd import KmerCounter
    with KmerCounter(kmer_size=k, abundance_min=1, abundance_max=0xFFFFFFFF) as kc:      # the stored abundance, read off the rows themselves
        device_load(kc, dev, M.words_of(values, k), ab, "sum")
        kk, rab = kc.rows()
        at = M.values_of(kk).index(base[7])
        assert rab[at] == 0xFFFFFFFF and kc.histogram()[10000] == 1 and kc.stats()["n_kmers"] == st["n_kmers"]


@pytest.mark.parametrize("k", (63, 64, 96, 127))
def test_values_that_differ_in_one_word_only(dev, k):
    """A...A is canonical whatever lies between (its reverse complement starts with T); one base changed in the bottom word, one in the top"""
    mid = int.from_bytes(np.random.default_rng(k).bytes(32), "little") % 4 ** (k - 2)
    x = mid << 2
    low, top = x ^ (1 << 8), x ^ (1 << (2 * k - 6))
    assert all(M.fault(v, 1, k) is None for v in (x, low, top)) and (x ^ low) >> 64 == 0 and (x ^ top) & ((1 << (64 * ((2 * k - 7) // 64))) - 1) == 0
    values = [x, low, top] * 700
    ab = np.arange(1, len(values) + 1, dtype=np.uint32)
    for rule in ("sum", "max", "min"):
        _, st = load_and_check(dev, k, values, ab, rule)
        assert st["n_distinct"] == 3


@pytest.mark.parametrize("k", (31, 63, 96))
def test_min_and_max_over_a_run_whose_extreme_sits_at_either_end(dev, k):
    base = others(k)[:40]
    for length in (2, 64, 300, 1500):
        for end in (0, length - 1):
            ab = np.full(length + 39, 50, dtype=np.uint32)
            for extreme, rule in ((1, "min"), (99, "max")):
                ab[end] = extreme
                values = [base[3]] * length + base[:3] + base[4:]
                load_and_check(dev, k, values, ab, rule)
                kept = M.load(values, ab, k, rule)
                assert kept[1][kept[0].index(base[3])] == extreme


# ------------------------------------------------------------------ the oracle identity on the device
def counted_rows(stream, dev, k, **kw):
    with count(stream, dev, k, **kw) as kc:
        kk, ab = kc.rows()
        return kk, ab, kc.histogram(), kc.stats()


def identity(dev, oracle, golden_dir, pair, k):
    from dsk_amd import KmerCounter
    sa, sb = (stream_of(n, oracle, golden_dir) for n in pair)
    ka, aa, _, _ = counted_rows(sa, dev, k, abundance_min=1)
    kb, ab_, _, _ = counted_rows(sb, dev, k, abundance_min=1)
    kmers, ab = np.concatenate([ka, kb]), np.concatenate([aa, ab_])
    for amin in (1, 2):
        wk, wa, whist, wst = counted_rows(joined(sa, sb), dev, k, abundance_min=amin)
        with KmerCounter(kmer_size=k, abundance_min=amin) as kc:
            st = device_load(kc, dev, kmers, ab, "sum")
            gk, ga = kc.rows()
            assert gk.shape == wk.shape and (gk == wk).all() and (ga == wa).all()
            assert (kc.histogram() == whist).all()
            got = kc.stats()
            assert (got["n_kmers"], got["n_distinct"], got["n_solid"]) == (wst["n_kmers"], wst["n_distinct"], wst["n_solid"])
            assert (st["n_kmers"], st["n_distinct"], st["n_rows"], st["n_in"]) == (wst["n_kmers"], wst["n_distinct"], wst["n_solid"], len(ab))


@pytest.mark.parametrize("k", (27, 31, 63, 96))
@pytest.mark.parametrize("pair", (("c1", "c2"), ("c3", "c4"), ("half0", "half1")), ids=("c1+c2", "c3+c4", "halves"))
def test_the_load_of_two_counts_is_the_count_of_both(dev, oracle, golden_dir, pair, k):
    identity(dev, oracle, golden_dir, pair, k)


@pytest.mark.parametrize("cus", ("1", "3"))
def test_the_identity_at_forced_cu_counts(dev, oracle, golden_dir, monkeypatch, cus):
    monkeypatch.setenv("DSKGPU_NUM_CU", cus)                         # (read at create)
    identity(dev, oracle, golden_dir, ("half0", "half1"), 31)


# ------------------------------------------------------------------ a restored session is the session
def snap(x):
    if isinstance(x, dict):
        return {k: snap(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return [snap(v) for v in x]
    if torch.is_tensor(x):
        x = x.cpu().numpy()
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    return x


def answers(kc, stream_t, ends):
    out = {}
    out["query_reads"] = snap(kc.query_reads_tensor(stream_t))
    out["adjacency"] = snap(kc.graph_adjacency_tensor())
    out["unitigs"] = snap(kc.unitigs())
    out["unitigs_stream"] = snap(kc.unitigs_stream_tensor())
    out["unitigs_table"] = snap(kc.unitigs_table_tensor())
    out["unitigs_rows"] = snap(kc.unitigs_rows_tensor())
    out["edges"] = snap(kc.unitig_edges())
    out["edges_table"] = snap(kc.unitig_edges_tensor())
    out["components"] = snap(kc.components())
    out["components_labels"] = snap(kc.components_labels_tensor())
    out["components_table"] = snap(kc.components_table_tensor())
    kc.colors_begin(len(ends))
    out["colors_add"] = snap(kc.colors_add_tensor(stream_t, ends))
    out["colors_rows"] = snap(kc.colors_rows_tensor(1))
    out["simplify_all"] = snap(kc.simplify_all())
    out["rows_left"] = snap(kc.rows())
    return out


def test_a_restored_session_answers_as_the_session(dev, oracle, golden_dir, tmp_path):
    from dsk_amd import KmerCounter
    k = 31
    stream = oracle.load_bank(os.path.join(golden_dir, "read50x_ref10K_e001.fasta.gz"))[0]
    t = torch.from_numpy(np.ascontiguousarray(stream)).to(dev)
    ends = [len(stream) // 3, 2 * len(stream) // 3, len(stream)]
    with count(stream, dev, k) as a, KmerCounter(kmer_size=k) as b, KmerCounter(kmer_size=k) as c, KmerCounter(kmer_size=k, partition_order=True, nb_partitions=7) as d:
        kk, ab = a.rows()
        st = device_load(b, dev, kk, ab, "unique")
        assert st["sorted_input"] == 1 and st["n_rows"] == len(ab) == st["n_distinct"] and st["n_below"] == 0
        # the round trip through a file, with a colour matrix
        a.colors_begin(3)
        a.colors_add_tensor(t, ends)
        saved = a.colors_rows_tensor(1)[0].cpu().numpy()
        path = str(tmp_path / "session.npz")
        a.save_rows(path)
        with np.load(path) as z:
            assert sorted(z.files) == ["abundance", "colors", "k", "kmers"] and int(z["k"]) == k and (z["kmers"] == kk).all() and (z["abundance"] == ab).all()
        assert c.load_saved(path)["n_rows"] == len(ab)
        assert (c.colors_rows_tensor(1)[0].cpu().numpy() == saved).all()
        with KmerCounter(kmer_size=27) as other:
            with pytest.raises(ValueError, match="k = 31"):
                other.load_saved(path)
        with KmerCounter(kmer_size=k, abundance_min=4) as strict:
            with pytest.raises(ValueError, match="not restored"):
                strict.load_saved(path)
        # a context created for the partition order: the loaded rows are in the global order all the same
        perm = np.random.default_rng(3).permutation(len(ab))
        device_load(d, dev, kk[perm], ab[perm], "unique")
        dk, da = d.rows()
        assert (dk == kk).all() and (da == ab).all()
        assert d.partition_offsets().tolist() == [len(ab) * p // 7 for p in range(8)]
        # every later call, byte for byte
        want, got = answers(a, t, ends), answers(b, t, ends)
        assert sorted(want) == sorted(got)
        for name in want:
            assert want[name] == got[name], name


def test_load_ascii_reads_the_text_of_the_rows(dev, oracle, golden_dir, tmp_path):
    from dsk_amd import KmerCounter
    k = 33
    res = oracle.count(stream_of("c1", oracle, golden_dir), k)
    lines = oracle.ascii_lines(res, amin=1)
    p = tmp_path / "rows.txt"
    p.write_text("\n".join(lines + lines[:100]) + "\n")
    with KmerCounter(kmer_size=k, abundance_min=2) as kc:
        st = kc.load_ascii(str(p))
        want_ab = res.ab.astype(np.int64)
        want_ab[:100] *= 2
        keep = want_ab >= 2
        kk, ab = kc.rows()
        assert (kk == res.words()[keep]).all() and (ab == want_ab[keep]).all() and st["n_in"] == len(lines) + 100 and st["n_distinct"] == res.distinct


# ------------------------------------------------------------------ the contract
def v(s):
    return sum("ACTG".index(c) << (2 * (len(s) - 1 - i)) for i, c in enumerate(s))


def refused(kc, dev, k, values, ab, combine, index, word):
    from dsk_amd import DskGpuError
    want = M.load(values, ab, k, combine)
    assert len(want) == 2 and want[0] == index, want
    with pytest.raises(DskGpuError) as e:
        device_load(kc, dev, M.words_of(values, k), np.asarray(ab, dtype=np.uint32), combine)
    assert e.value.code == E_ARG and "row %d " % index in str(e.value) and word in str(e.value), str(e.value)


@pytest.mark.parametrize("k", (31, 33, 97))
def test_an_invalid_row_names_the_lowest_index_and_leaves_the_result(dev, oracle, golden_dir, k):
    stream = stream_of("c1", oracle, golden_dir)
    rng = np.random.default_rng(k)
    good = pool(k, 600, rng)
    not_canonical = M.revcomp(next(x for x in good if M.revcomp(x, k) != x), k)
    too_big = good[5] | (1 << (2 * k))                             # bit 2k: >= 4^k
    if k == 97:
        too_big = good[5] | (1 << 255)                             # ... and the very top of the fourth word
    with count(stream, dev, k) as kc:
        rows0, hist0, stats0 = kc.rows(), kc.histogram(), kc.stats()
        t = torch.from_numpy(stream).to(dev)
        q0, u0 = snap(kc.query_reads_tensor(t)), snap(kc.unitigs_stream_tensor())
        ones = [1] * 600
        for combine in ("sum", "unique"):
            for bad_value, word in ((not_canonical, "canonical"), (too_big, "4^k")):
                values = list(good)
                values[77], values[401] = bad_value, bad_value
                refused(kc, dev, k, values, ones, combine, 77, word)
                values[77] = good[77]
                refused(kc, dev, k, values, ones, combine, 401, word)
            ab = list(ones)
            ab[300], ab[599] = 0, 0
            refused(kc, dev, k, good, ab, combine, 300, "abundance 0")
            mixed = list(good)
            mixed[10] = too_big
            refused(kc, dev, k, mixed, ab, combine, 10, "4^k")
        values = list(good)
        values[500], values[20], values[450] = good[3], good[400], good[3]         # repeats at 400 (of 20), 450 (of 3), 500 (of 3)
        refused(kc, dev, k, values, ones, "unique", 400, "repeats the value 0x%0*x" % (16 * kc.words, good[400]))
        values[0] = not_canonical
        refused(kc, dev, k, values, ones, "unique", 0, "canonical")
        # the previous result, its index and its unitigs still answer as before
        assert snap(kc.rows()) == snap(rows0) and (kc.histogram() == hist0).all() and kc.stats() == stats0
        assert snap(kc.query_reads_tensor(t)) == q0 and snap(kc.unitigs_stream_tensor()) == u0
        # ... and the same rows are taken when nothing is wrong with them
        assert device_load(kc, dev, M.words_of(good, k), np.asarray(ones, np.uint32), "unique")["n_rows"] == 0      # (abundance 1 < abundance_min 2)
        assert kc.stats()["n_distinct"] == 600 and kc.histogram()[1] == 600


def test_nothing_to_load_bad_arguments_and_a_rank(dev):
    from dsk_amd import DskGpuError, KmerCounter
    k = 31
    with KmerCounter(kmer_size=k, abundance_min=1) as kc:
        assert kc.load_rows(0, 0, 0) == dict.fromkeys(M.STATS, 0) | {"sorted_input": 1}
        assert kc.rows()[0].shape == (0, 1) and not kc.histogram().any() and kc.stats()["n_solid"] == 0 and kc.num_partitions() == 4
        values = pool(k, 10, np.random.default_rng(1))
        tk, _ = guarded_input(dev, M.words_of(values, k))
        ta, _ = guarded_input(dev, np.ones(10, np.uint32))
        torch.cuda.synchronize()
        pk, pa = tk.data_ptr() + GUARD, ta.data_ptr() + GUARD
        lib, h = kc._lib, kc._h
        for args, word in (((pk, pa, 10, 4), "combine"), ((0, pa, 10, 0), "null"), ((pk, 0, 10, 0), "null"), ((pk + 4, pa, 9, 0), "aligned"), ((pk, pa + 2, 9, 0), "aligned"),
                           ((pk, pa, (1 << 32) - 1, 0), "2^32 - 2")):
            rc = lib.dskgpu_load_rows(h, args[0] or None, args[1] or None, args[2], args[3], None)
            assert rc == E_ARG and word in lib.dskgpu_last_error(h).decode(), (args, lib.dskgpu_last_error(h).decode())
        with pytest.raises(ValueError):
            kc.load_rows(pk, pa, 10, "union")
        assert kc.stats()["n_solid"] == 0                              # the empty result is still there
        assert lib.dskgpu_load_rows(h, pk, pa, 10, 0, None) == 0 and kc.stats()["n_solid"] == 10      # (the stats may be left out)
        assert kc.load_rows(pk, pa, 10, "sum")["n_rows"] == 10
    with KmerCounter(kmer_size=k, world_size=2, rank=1) as rank:
        with pytest.raises(DskGpuError) as e:
            rank.load_rows(pk, pa, 10)
        assert e.value.code == E_STATE and "world_size" in str(e.value)


@pytest.mark.parametrize("histo_max", (12287, 12288, 20000))
def test_a_histogram_wider_than_a_block_keeps_in_lds(dev, histo_max):
    """LR_HIST_LDS = 12288 bins stay in LDS; the bins above go to the global histogram one by one (histo_max + 1 > 12288)"""
    from dsk_amd import KmerCounter
    k = 31
    rng = np.random.default_rng(histo_max)
    values = pool(k, 3000, rng)
    ab = rng.integers(1, 25000, 3000).astype(np.uint32)
    ab[:6] = (12287, 12288, 12289, 19999, 20000, 20001)
    many = values + values[:500]                                    # sums too: some cross the last bins
    ab = np.concatenate([ab, rng.integers(1, 9000, 500).astype(np.uint32)])
    want = M.load(many, ab, k, "sum", 2, AMAX, histo_max)
    assert want[2][histo_max] > 0 and want[2][12000:].sum() > 100
    with KmerCounter(kmer_size=k, abundance_min=2, histo_max=histo_max) as kc:
        st = device_load(kc, dev, M.words_of(many, k), ab, "sum")
        same_as_model(kc, k, want, st)


def test_the_stage_times_are_the_loads_and_survive_a_refused_one(dev):
    from dsk_amd import DskGpuError, KmerCounter
    k = 31
    values = pool(k, 500, np.random.default_rng(9))
    ones = np.ones(500, np.uint32)
    with KmerCounter(kmer_size=k, abundance_min=1, timing=True) as kc:
        device_load(kc, dev, M.words_of(values[::-1], k), ones)
        before = kc.stage_times()
        assert [name for name, _ in before] == ["load check", "load order", "load combine"]
        bad = ones.copy()
        bad[3] = 0
        with pytest.raises(DskGpuError):
            device_load(kc, dev, M.words_of(values, k), bad)
        assert kc.stage_times() == before
        device_load(kc, dev, M.words_of(values, k), ones)               # ascending: the order stage is there and empty
        assert [name for name, _ in kc.stage_times()] == ["load check", "load order", "load combine"]
    with KmerCounter(kmer_size=97) as wide:                            # four-word rows: the row order's own limit, refused before anything is read
        rc = wide._lib.dskgpu_load_rows(wide._h, 4096, 4096, 0xFFFF0000, 0, None)
        assert rc == E_ARG and "k > 64" in wide._lib.dskgpu_last_error(wide._h).decode()


def test_load_then_count_load_twice_and_filter_between(dev, oracle, golden_dir):
    from dsk_amd import KmerCounter
    k = 31
    stream = stream_of("c2", oracle, golden_dir)
    with count(stream, dev, k) as plain:
        want = snap(plain.rows()), snap(plain.histogram()), plain.stats()
    rng = np.random.default_rng(5)
    first, second = pool(k, 3000, rng), pool(k, 2000, rng)
    t = torch.from_numpy(stream).to(dev)
    torch.cuda.synchronize()
    with KmerCounter(kmer_size=k) as kc:
        kc.set_reads_device(t.data_ptr(), t.numel())
        ab1 = rng.integers(1, 6, 3000).astype(np.uint32)
        device_load(kc, dev, M.words_of(first, k), ab1, "sum")
        same_as_model(kc, k, M.load(first, ab1, k, "sum", 2))
        kc.count()                                                  # load, then count: the plain count
        assert (snap(kc.rows()), snap(kc.histogram()), kc.stats()) == want
        ab2 = rng.integers(2, 6, 2000).astype(np.uint32)
        device_load(kc, dev, M.words_of(second, k), ab2, "max")      # ... and a load over a count
        same_as_model(kc, k, M.load(second, ab2, k, "max", 2))
        device_load(kc, dev, M.words_of(first, k), ab1, "unique")    # load twice
        same_as_model(kc, k, M.load(first, ab1, k, "unique", 2))
        rows, rab, _, _ = M.load(first, ab1, k, "unique", 2)
        keep = (np.arange(len(rows)) % 3 != 0).astype(np.uint8)
        assert kc.filter_rows_tensor(torch.from_numpy(keep).to(dev)) == int(keep.sum())
        kk, ab = kc.rows()
        assert (kk == M.words_of(rows, k)[keep == 1]).all() and (ab == rab[keep == 1]).all()
        kc.query_prepare()
        device_load(kc, dev, M.words_of(second, k), ab2, "min")      # filter_rows after a load, then a second load
        same_as_model(kc, k, M.load(second, ab2, k, "min", 2))
        probe = torch.from_numpy(M.words_of(second[:50] + first[:50], k).view(np.int64)).to(dev)
        got = kc.query_kmers_tensor(probe).cpu().numpy().view(np.uint32)
        lookup = dict(zip(*M.load(second, ab2, k, "min", 2)[:2]))
        assert got.tolist() == [int(lookup.get(x, 0)) for x in second[:50] + first[:50]]
