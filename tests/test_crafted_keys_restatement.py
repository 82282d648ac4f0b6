"""The crafted inputs of tests/test_gpu_crafted_keys.py are what they claim -- checked without a GPU.

tests/crafted_keys.py restates the key mixers of dsk_amd/csrc/kmer_device.h in Python and inverts them to build canonical k-mers with
chosen bit fields of the mixed word.  Here: the restatement against the header itself (tests/host/mix_words.cpp is the header compiled
for the host), what every builder promises, the statement about the all-ones key for every k, the oracle's count of the crafted
streams, and a plain linear-probing model that says how long the probe runs are that the device tables see.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import crafted_keys as ck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mix_words():
    """keys (lists of words, least significant first) -> their mixed top words by the header's own code"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "host"), "mix_words"])
    exe = os.path.join(ROOT, "tests", "host", "mix_words")

    def run(keys):
        text = "".join("%d %s\n" % (len(w), " ".join("%x" % int(x) for x in w)) for w in keys)
        out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.split()
        assert len(out) == len(keys)
        return [int(x, 16) for x in out]
    return run


@pytest.fixture(scope="module")
def families():
    return ck.device_families()


def special_families():
    rng = np.random.default_rng(7)
    out = [("twins k=%d" % k, ck.twin_family(k)) for k in (63, 64, 128)] + [("twins k=127", ck.twins(127, 5, rng))]
    out += [("sentinel k=%d" % k, ck.sentinel_kmer(k)) for k in (64, 128)]
    out += [("top word sentinel k=%d" % k, ck.top_word_sentinel(k, rng)) for k in (63, 64)]
    out += [("v3 with low12 k=%d" % k, ck.family_v3(k, 200, 0xFFFFFFFF, 0xFFF, rng, low12=0xFFF)) for k in (63, 64)]
    return out


# ------------------------------------------------------------------ the restatement against the header
@pytest.mark.parametrize("W", [1, 2, 4])
def test_python_mixers_equal_the_header(mix_words, W):
    """10 000 random keys per width, and the keys whose carries are longest (all ones, single bits): the Python ints, the numpy form
    and kmer_device.h give the same mixed top word.  (Breaking MIX_C in tests/crafted_keys.py makes this fail.)"""
    rng = np.random.default_rng(100 + W)
    keys = rng.integers(0, 1 << 64, size=(10_000, W), dtype=np.uint64)
    keys[:64, :] = 0
    keys[np.arange(64), W - 1] = np.uint64(1) << np.arange(64, dtype=np.uint64)
    keys[64:128, 0] = ~keys[np.arange(64), W - 1]
    keys[128] = np.uint64(ck.M64)
    got = mix_words([list(r) for r in keys])
    py = [ck.kmixN([int(x) for x in r])[-1] if W > 1 else ck.kmix(int(r[0])) for r in keys]
    assert py == got
    k = {1: 32, 2: 64, 4: 128}[W]
    assert [int(x) for x in ck.mixed_top_np(keys, k)] == got
    for r in keys[:2000]:                                      # and the inverse is one
        w = [int(x) for x in r]
        assert (ck.kunmixN(ck.kmixN(w)) if W > 1 else [ck.kunmix(ck.kmix(w[0]))]) == w


def test_every_family_member_against_the_header(mix_words, families):
    for name, fam, _, _ in [(n, f, None, None) for n, f in special_families()] + families:
        W = ck.key_words(fam.k)
        assert mix_words([ck.words_of(v, W) for v in fam.values]) == fam.h, name


# ------------------------------------------------------------------ what the builders promise
def check_members(name, fam):
    k = fam.k
    assert len(set(fam.values)) == len(fam), name
    for v, s in zip(fam.values, fam.text):
        assert ck.is_canonical(v, k) and len(s) == k and ck.value_of_text(s) == v, name
    assert fam.words.shape == (len(fam), ck.abi_words(k))
    assert [ck.value_of(r) for r in fam.words] == fam.values


def test_builder_promises(families):
    """count, distinctness, canonicity, width; the fixed bit fields of h; pairwise different h; the slot formulas restated; one
    sub-partition under every plan the restated make_plan gives for the input at extra_bits 0..3"""
    for name, fam, fixed, crowd in families:
        check_members(name, fam)
        assert len(set(fam.h)) == len(fam), name
        for (hi, lo), val in fixed.items():
            assert {(h >> lo) & ((1 << (hi - lo + 1)) - 1) for h in fam.h} == {val}, (name, hi, lo)
        if (11, 0) in fixed:
            assert {ck.slot_4096(h) for h in fam.h} == {fixed[(11, 0)]}, name
            for cap in (1024, 2048, 4096):                     # the lookup index: home slot and fingerprint
                assert len({(h & (cap - 1), h >> 32) for h in fam.h}) == 1
        if (31, 20) in fixed:
            slots = {ck.slot_v3(h) for h in fam.h}
            assert slots == {3071}, (name, slots)                   # 0xFFF: the last slot of the 3072
        n_in = crowd + int(ck.abundances(len(fam)).sum()) + 1
        for n_upper in (n_in, crowd + 8 * len(fam) + 1):
            for eb in range(4):
                plan = ck.make_plan(n_upper, eb, ck.key_words(fam.k))
                if plan is not None:
                    assert len({ck.digits(h, plan[1], plan[2]) for h in fam.h}) == 1, (name, plan)


def test_restated_plan_sizes():
    """the crowds are two levels just above 1024 sub-partitions; a family alone is one level"""
    for k, n in ck.CROWD_READS.items():
        W = ck.key_words(k)
        levels, p1, p2 = ck.make_plan(ck.crowd_kmers(k) + 1, 0, W)
        assert levels == 2 and 1024 < -(-ck.crowd_kmers(k) // ck.TARGET_KEYS[W]) < 1100 and p1 * p2 > 1024, (k, p1, p2)
    for W in (1, 2, 4):
        assert ck.make_plan(5 * 3585, 0, W)[0] == 1 and ck.make_plan(5 * 3585, 3, W)[0] == 1


def test_family_v3_neighbouring_slots():
    """h[31:20] fixed: the home slot of k_count2v3 is the same or one of two neighbours, for any top12"""
    rng = np.random.default_rng(3)
    for top12 in (0, 1, 0x555, 0xABC, 0xFFF):
        fam = ck.family_v3(63, 300, 0x12345678, top12, rng)
        slots = {ck.slot_v3(h) for h in fam.h}
        assert max(slots) - min(slots) <= 1 and {(h >> 20) & 0xFFF for h in fam.h} == {top12}


def test_special_families():
    for name, fam in special_families():
        check_members(name, fam)
    for k in (63, 64, 127, 128):
        fam = ck.twin_family(k) if k != 127 else ck.twins(127, 5, np.random.default_rng(7))
        assert len(set(fam.h)) == 1 and len(fam) == (5 if k == 127 else 300)
    for k in (64, 128):
        v = ck.sentinel_kmer(k).values[0]
        assert ck.kmixN(ck.words_of(v, ck.key_words(k))) == [ck.M64] * ck.key_words(k)
    for k in (63, 64):
        fam = ck.top_word_sentinel(k, np.random.default_rng(9))
        assert fam.h == [ck.M64] and fam.words[0, 0] != np.uint64(ck.M64)
    for name, fam in special_families():
        if name.startswith("v3 with low12"):
            assert len(set(fam.h)) == 200 and {ck.slot_v3(h) for h in fam.h} == {3071} and {h & 4095 for h in fam.h} == {4095}


def test_moved_twin_helper_gives_the_same_strings():
    """the k-mers of the three parity tests that used this helper before it moved: same seed, same strings"""
    a, b, c = ck.top_word_twins(63, np.random.default_rng(5))
    assert a == "GAGTACCATTTGGTGTTTTGTGTAGTCCTTTAGAGTGCCCAGCCATCCAACCGAGATCTCGGC"
    assert b == "ATTCACTCTATGTTTTGGTGTCGAGACTTCTTAAGGTGACTAAAGGGCGTAAACTTTGCGAAT"
    assert c == "TCCGATAAATTAGAATACGTAAGTTGCCCTATAAAGCGACGCCGGTTAATCTGACATGGCTGC"
    va, vb, vc = (ck.value_of_text(s) for s in (a, b, c))
    assert va != vb and ck.mixed_top(va, 63) == ck.mixed_top(vb, 63) and ck.mixed_top(vc, 63) == ck.M64
    assert all(ck.is_canonical(v, 63) for v in (va, vb, vc))


# ------------------------------------------------------------------ the all-ones key
def test_the_all_ones_key_is_a_kmer_at_k_64_and_128_only():
    """The pad / empty-slot value of the tables is the mixed form of a canonical k-mer for k = 64 and k = 128 and for no other k in
    1..128 (never for k <= 32): what sentinel_is_a_kmer() in dskgpu.hip decides when a context is created."""
    is_kmer = []
    for k in range(1, 129):
        W = ck.key_words(k)
        v = ck.value_of(ck.kunmixN([ck.M64] * W)) if W > 1 else ck.kunmix(ck.M64)
        if ck.is_canonical(v, k):
            is_kmer.append(k)
    assert is_kmer == [64, 128]


# ------------------------------------------------------------------ the oracle on the crafted streams
@pytest.mark.parametrize("rc_prob", [0.0, 0.5])
@pytest.mark.parametrize("k", ck.SLOT_KS)
def test_oracle_counts_the_crafted_stream_to_the_given_kmers(oracle, k, rc_prob):
    fam = ck.alone_family(k, 65, ck.HI32S[2], 4095)
    ab = ck.abundances(len(fam))
    stream = ck.reads_of(fam.text, ab, np.random.default_rng(k), rc_prob)
    assert len(stream) == int(ab.sum()) * (k + 1)
    if rc_prob:
        fwd = set(fam.text)
        n_rc = sum(1 for line in stream.tobytes().decode().split() if line not in fwd)
        assert 0 < n_rc < int(ab.sum())                    # some records are written as their reverse complement
    ref = oracle.count(stream, k)
    order = np.lexsort(fam.words.T)
    assert ref.total == int(ab.sum()) and ref.distinct == len(fam)
    assert (ref.words() == fam.words[order]).all() and (ref.ab == ab[order]).all()


def test_spread_records_add_exactly_their_kmers(oracle):
    """records of k bases between the reads of a crowd add their own k-mers and no other: the expectation of the crowd tests is
    the crowd's count (computed once) merged with the family"""
    k = 63
    crowd = ck.crowd_stream(k)[: 151 * 500]
    fam = ck.crowd_family(k, 0)[:50]
    ab = ck.abundances(50)
    stream = ck.spread(crowd, 151, ck.records_of(fam.text, ab, np.random.default_rng(1)))
    assert len(stream) == len(crowd) + int(ab.sum()) * (k + 1)
    base, ref = oracle.count(crowd, k), oracle.count(stream, k)
    w, a = ck.merge_rows(base.words(), base.ab, fam.words, ab)
    assert ref.total == base.total + int(ab.sum()) and (ref.words() == w).all() and (ref.ab == a).all()
    lines = stream.tobytes().split(b"\n")
    at = [i for i, ln in enumerate(lines) if len(ln) == k]
    assert len(at) == int(ab.sum()) and at[0] == 0 and at[-1] > len(lines) * 0.9      # spread over the whole stream


# ------------------------------------------------------------------ how long the probe runs are
def test_probe_runs_of_crafted_and_random_inputs():
    """A plain linear-probing model of a 4096-slot table.  A crafted family of n members is ONE run of at least n slots, and the
    families placed at the table's end run across slot 4095 -> 0.  The same number of random k-mers (the suite's other inputs):
    longest run measured by this test for n = 64 / 1000 / 3000 / 3584 random 32-mers: 2 / 7 / 49 / 164 slots (printed below; only
    the last crosses the end of the table with these seeds), against 64 / 1000 / 3000 / 3584 for the crafted ones."""
    for k in (32, 64, 128):
        for n in (64, 1000) + ((3000,) if k == 128 else ()):
            for low12 in ck.alone_low12s(n):
                fam = ck.alone_family(k, n, ck.HI32S[2], low12)
                longest, wraps = ck.probe_model([ck.slot_4096(h) for h in fam.h])
                assert longest >= n
                assert wraps == (low12 + n > 4096), (k, n, low12)
        longest, wraps = ck.probe_model([ck.slot_4096(h) for h in ck.alone_family(k, 3585, ck.HI32S[2], 4095).h[:3584]])
        assert longest == 3584 and wraps
    measured = {}
    for n in (64, 1000, 3000, 3584):
        rng = np.random.default_rng(n)
        v = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
        h = ck.mixed_top_np(v.reshape(-1, 1), 32)
        measured[n] = ck.probe_model([int(x) & 4095 for x in h])
        print(f"random 32-mers, n = {n}: longest run {measured[n][0]} slots, crosses the end: {measured[n][1]}")
    assert measured[1000][0] < 100 and measured[64][0] < 16          # (orders of magnitude, not the figures: those are in the docstring)
