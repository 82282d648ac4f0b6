"""Canonical k-mers built to order for the hash structures of the count and lookup paths -- TEST INFRASTRUCTURE ONLY.

Every hash structure is keyed by a bijective mix of the k-mer (dsk_amd/csrc/kmer_device.h: kmix / kmixN), and the mixers are
invertible, so inputs can be made that random or natural reads never give: hundreds to thousands of DIFFERENT k-mers with one
sub-partition and one home slot, k-mers with one 64-bit hash, the k-mer whose mixed form is the empty-slot value.

    h                      the mixed (top) word of a key
    level-1 / level-2 digit  mulhi(h[63:32], P1), mulhi(lo32(h[63:32] * P1), P2): functions of h[63:32] alone
    home slot                h[11:0] in the 4096-slot LDS tables, (lo32(h) * 3072) >> 32 in k_count2v3,
                             h & (cap - 1) with fingerprint h >> 32 in the lookup index

Python ints and numpy only.  tests/test_crafted_keys_restatement.py pins the restatement of the mixers to the header (through
tests/host/mix_words.cpp) and checks what every builder promises.

Which widths can be crafted: the key of a k-mer has W = 1, 2 or 4 words (k <= 32, <= 64, <= 128) and h is a bijection of the TOP
word for fixed lower words.  h can be chosen freely only where the top word is (nearly) free: k = 32 / 64 / 128 (all 64 bits), 31 /
63 / 127 (62 bits), and by enumeration down to k = 27 (54 bits: 523 members per (hi32, low12)).  For k = 33..~60 and 65..~125 the
top word holds too few bits (for k <= 96 word 3 is zero: h is a hash of the low words) -- not crafted.
"""
import os

import numpy as np

M64 = (1 << 64) - 1
MIX_C = 0xff51afd7ed558ccd
MIX_CINV = 0x4f74430c22a54005
FOLD_MULT = (0x9e3779b97f4a7c15, 0xc2b2ae3d27d4eb4f, 0x165667b19e3779f9)
WIDE_KS = (63, 64, 127, 128)
SLOT_KS = (27, 31, 32) + WIDE_KS


# ------------------------------------------------------------------ the mixers, restated
def kmix(x):
    x ^= x >> 32
    x = (x * MIX_C) & M64
    return x ^ (x >> 32)


def kunmix(x):
    x ^= x >> 32
    x = (x * MIX_CINV) & M64
    return x ^ (x >> 32)


def kmum(a, c):
    p = a * c
    return (p & M64) ^ (p >> 64)


def kfold_low(words):
    """XOR of kmum over every word but the top one (words: least significant first)"""
    t = 0
    for i, w in enumerate(words[:-1]):
        t ^= kmum(w, FOLD_MULT[i])
    return t


def kmixN(words):
    return list(words[:-1]) + [kmix(words[-1] ^ kfold_low(words))]


def kunmixN(words):
    return list(words[:-1]) + [kunmix(words[-1]) ^ kfold_low(words)]


def _kunmix_np(h):
    h = h ^ (h >> np.uint64(32))
    h = h * np.uint64(MIX_CINV)
    return h ^ (h >> np.uint64(32))


# ------------------------------------------------------------------ k-mers as values
def key_words(k):
    """words of the device key: 1, 2 or 4"""
    return 1 if k <= 32 else 2 if k <= 64 else 4


def abi_words(k):
    """words of a row at the C-ABI"""
    return (k + 31) // 32


def words_of(v, nw):
    return [(v >> (64 * i)) & M64 for i in range(nw)]


def value_of(words):
    return sum(int(w) << (64 * i) for i, w in enumerate(words))


_REV4 = bytes(((b & 3) << 6) | ((b & 12) << 2) | ((b & 48) >> 2) | ((b & 192) >> 6) for b in range(256))
_COMP = int("10" * 128, 2)


def revcomp(v, k):
    """reverse complement of a k-mer value (A C T G = 0 1 2 3, first base most significant, complement = code ^ 2), k <= 128"""
    rev = int.from_bytes(v.to_bytes(32, "little").translate(_REV4), "big")       # all 128 pairs of 256 bits reversed
    return (rev >> (256 - 2 * k)) ^ (_COMP & ((1 << (2 * k)) - 1))


def is_canonical(v, k):
    return 0 <= v < (1 << (2 * k)) and v <= revcomp(v, k)


def text(v, k):
    return "".join("ACTG"[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))


def value_of_text(s):
    v = 0
    for ch in s:
        v = (v << 2) | "ACTG".index(ch)
    return v


_TEXT_RC = str.maketrans("ACGT", "TGCA")


def text_revcomp(s):
    return s.translate(_TEXT_RC)[::-1]


def mixed_top(v, k):
    """h of a k-mer value: what the device partitions, slots and fingerprints it by"""
    return kmixN(words_of(v, key_words(k)))[-1]


def _kmum_np(a, c):
    """numpy: low half ^ high half of the 128-bit products of the uint64 array a with the constant c"""
    m32 = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    a0, a1 = a & m32, a >> s32
    c0, c1 = np.uint64(c & 0xFFFFFFFF), np.uint64(c >> 32)
    p00, p01, p10, p11 = a0 * c0, a0 * c1, a1 * c0, a1 * c1
    mid = (p00 >> s32) + (p01 & m32) + (p10 & m32)
    hi = p11 + (p01 >> s32) + (p10 >> s32) + (mid >> s32)
    return (a * np.uint64(c)) ^ hi


def mixed_top_np(words, k):
    """numpy: h of every row of words (uint64[n, >= key words of k], least significant word first; missing words are zero)"""
    W = key_words(k)
    words = np.ascontiguousarray(words, dtype=np.uint64)
    if words.shape[1] < W:
        words = np.concatenate([words, np.zeros((len(words), W - words.shape[1]), np.uint64)], axis=1)
    x = words[:, W - 1].copy()
    for i in range(W - 1):
        x ^= _kmum_np(words[:, i], FOLD_MULT[i])
    x ^= x >> np.uint64(32)
    x *= np.uint64(MIX_C)
    return x ^ (x >> np.uint64(32))


def _revcomp_np(v, k):
    """numpy: reverse complement of one-word values"""
    r = np.zeros_like(v)
    x = v.copy()
    for _ in range(k):
        r = (r << np.uint64(2)) | ((x & np.uint64(3)) ^ np.uint64(2))
        x >>= np.uint64(2)
    return r


class Family:
    """distinct canonical k-mers: .values (ints), .text, .words (uint64[n, abi words]), .h (mixed top words, ints)"""

    def __init__(self, k, values):
        self.k = k
        self.values = [int(v) for v in values]
        self.h = [mixed_top(v, k) for v in self.values]
        self.text = [text(v, k) for v in self.values]
        nw = abi_words(k)
        self.words = np.array([words_of(v, nw) for v in self.values], dtype=np.uint64).reshape(len(self.values), nw)

    def __len__(self):
        return len(self.values)

    def __getitem__(self, sl):
        return Family(self.k, self.values[sl])


# ------------------------------------------------------------------ builders
def _one_word_members(k, h):
    """the canonical k-mers (k <= 32) among the pre-images of the mixed words h (numpy), in the order of h"""
    v = _kunmix_np(h)
    if k < 32:
        v = v[v < (np.uint64(1) << np.uint64(2 * k))]
    return v[v <= _revcomp_np(v, k)]


def _wide_member(k, h, rng, avoid=()):
    """a canonical k-mer of a two- / four-word k with mixed top word h: random lower words, the top word solved for"""
    W = key_words(k)
    top_bits = 2 * k - 64 * (W - 1)
    u = kunmix(h)
    for _ in range(4096):
        low = [int(x) for x in rng.integers(0, 1 << 64, size=W - 1, dtype=np.uint64)]
        top = u ^ kfold_low(low + [0])
        if top >> top_bits:
            continue
        v = value_of(low + [top])
        if v <= revcomp(v, k) and v not in avoid:
            return v
    raise ValueError(f"no canonical {k}-mer with mixed top word {h:#x} in 4096 tries")


def _family(k, n, h_of_free, n_free, rng):
    """n members with pairwise different h = h_of_free(f), f drawn without repetition from range(n_free)"""
    if k not in SLOT_KS:
        raise ValueError(f"k = {k}: the mixed word cannot be chosen")
    if k <= 32:
        free = np.arange(n_free, dtype=np.uint64)
        members = _one_word_members(k, h_of_free(free))
        if len(members) < n:
            raise ValueError(f"k = {k}: only {len(members)} members, {n} asked for")
        return Family(k, members[np.sort(rng.choice(len(members), size=n, replace=False))])
    if n > n_free:
        raise ValueError(f"{n} members asked for, {n_free} mixed words to choose from")
    return Family(k, [_wide_member(k, int(h_of_free(int(f))), rng) for f in rng.choice(n_free, size=n, replace=False)])


def family_slot(k, n, hi32, low12, rng):
    """n canonical k-mers with h[63:32] == hi32 and h[11:0] == low12, pairwise different h: one sub-partition under any plan and any
    retry, one home slot in every 4096-slot table (k_count1, k_count1v3, k_count_mw, k_count_chained) and in the lookup index up to
    4096 slots, one fingerprint."""
    fixed = (hi32 << 32) | low12
    if k <= 32:
        return _family(k, n, lambda f: np.uint64(fixed) | (f << np.uint64(12)), 1 << 20, rng)
    return _family(k, n, lambda f: fixed | (f << 12), 1 << 20, rng)


def family_v3(k, n, hi32, top12, rng, low12=None):
    """k in {63, 64}: h[63:32] == hi32 and h[31:20] == top12: home slot (lo32(h) * 3072) >> 32 of k_count2v3 equal or one of two
    neighbours (3071, the last, for 0xFFF).  h[19:0] is free; with low12 given h[11:0] is fixed as well (one slot in k_count_mw too)
    and only the 256 values of h[19:12] remain: n <= 200."""
    if k not in (63, 64):
        raise ValueError("family_v3 is for two-word keys whose top word can be chosen: k = 63, 64")
    fixed = (hi32 << 32) | (top12 << 20)
    if low12 is None:
        return _family(k, n, lambda f: fixed | f, 1 << 20, rng)
    if n > 200:
        raise ValueError("h[19:12] has 256 values: n <= 200")
    return _family(k, n, lambda f: fixed | (f << 12) | low12, 256, rng)


def twins(k, n, rng, h=None):
    """n different canonical k-mers with the SAME mixed top word: one sub-partition, slot, fingerprint and 64-bit hash"""
    if k not in WIDE_KS:
        raise ValueError("twins need lower words: k = 63, 64, 127, 128")
    if h is None:
        h = int(rng.integers(0, 1 << 64, dtype=np.uint64))
    seen = set()
    while len(seen) < n:
        seen.add(_wide_member(k, h, rng, seen))
    return Family(k, sorted(seen))


def sentinel_kmer(k):
    """k in {64, 128}: the k-mer whose mixed key is all ones in every word -- the pad / empty-slot value of the tables"""
    if k not in (64, 128):
        raise ValueError("the all-ones key is a canonical k-mer at k = 64 and k = 128 only")
    v = value_of(kunmixN([M64] * key_words(k)))
    assert is_canonical(v, k)
    return Family(k, [v])


def top_word_sentinel(k, rng):
    """k in {63, 64}: a k-mer whose mixed TOP word is all ones (the empty-slot value of k_count2v3's table), any low word"""
    if k not in (63, 64):
        raise ValueError("k = 63, 64")
    return Family(k, [_wide_member(k, M64, rng)])


def top_word_twins(k, rng):
    """Two different canonical k-mers (33 <= k <= 64) with the SAME mixed top word, and one whose mixed top word is the empty-slot
    value of the count tables -> three base strings.  (The draws are those of the helper the parity tests had before this module:
    the same seed gives the same strings.)"""
    def find(x, avoid=None):          # a canonical k-mer with top ^ kmum(low) == x
        while True:
            low = int(rng.integers(0, 1 << 62)) << 2 | int(rng.integers(0, 4))
            top = x ^ kmum(low, FOLD_MULT[0])
            v = (top << 64) | low
            if top >> (2 * k - 64) == 0 and v <= revcomp(v, k) and v != avoid:
                return v
    first = None
    while first is None:
        v = int(rng.integers(0, 1 << 62)) << (2 * k - 62) | int(rng.integers(0, 1 << 62))
        v &= (1 << (2 * k)) - 1
        if v <= revcomp(v, k):
            first = v
    x = (first >> 64) ^ kmum(first & M64, FOLD_MULT[0])
    return text(first, k), text(find(x, first), k), text(find(kunmix(M64), None), k)


# ------------------------------------------------------------------ streams
def records_of(kmers, counts, rng, rc_prob=0.5):
    """one record (bytes, no newline) per occurrence, shuffled; a record is written reverse-complemented with probability rc_prob"""
    recs = []
    for s, c in zip(kmers, counts):
        for _ in range(int(c)):
            recs.append((text_revcomp(s) if rng.random() < rc_prob else s).encode())
    order = rng.permutation(len(recs))
    return [recs[i] for i in order]


def reads_of(kmers, counts, rng, rc_prob=0.5):
    """uint8 stream: one k-base record per occurrence of every k-mer (text), shuffled, some reverse-complemented, '\\n' between"""
    recs = records_of(kmers, counts, rng, rc_prob)
    return np.frombuffer(b"".join(r + b"\n" for r in recs), dtype=np.uint8).copy()


def spread(crowd, record_bytes, records):
    """`records` put evenly between the records of `crowd` (a stream of records of record_bytes bytes each, newline included)"""
    assert len(crowd) % record_bytes == 0
    n = len(crowd) // record_bytes
    at = (np.arange(len(records)) * n) // max(1, len(records))
    parts, prev = [], 0
    for a, r in zip(at, records):
        parts.append(crowd[prev * record_bytes: int(a) * record_bytes])
        parts.append(np.frombuffer(r + b"\n", dtype=np.uint8))
        prev = int(a)
    parts.append(crowd[prev * record_bytes:])
    return np.concatenate(parts)


def merge_rows(words_a, ab_a, words_b, ab_b):
    """the rows of two counts as one, ascending by value, the abundances of rows in both added"""
    w = np.concatenate([words_a, words_b]); a = np.concatenate([ab_a, ab_b]).astype(np.uint64)
    order = np.lexsort(w.T)                              # last key = most significant word
    w, a = w[order], a[order]
    first = np.ones(len(w), bool)
    first[1:] = (w[1:] != w[:-1]).any(axis=1)
    return w[first], np.add.reduceat(a, np.nonzero(first)[0]).astype(np.uint32) if len(w) else a.astype(np.uint32)


def abundances(n):
    """1..5 by member index"""
    return (np.arange(n) % 5 + 1).astype(np.uint32)


# ------------------------------------------------------------------ restated slot and plan formulas
def slot_4096(h):
    return h & 4095


def slot_v3(h):
    return ((h & 0xFFFFFFFF) * 3072) >> 32


def digits(h, p1, p2):
    hi = h >> 32
    return (hi * p1) >> 32, (((hi * p1) & 0xFFFFFFFF) * p2) >> 32


SC_NT = 1024
TARGET_KEYS = {1: 2900, 2: 2560, 4: 640}


def ascatter_lds(W, P):
    key = 8 * W
    keys = SC_NT * (6 if W == 2 else 12 if W == 1 else 12 // W)
    G = 4 if W == 2 else 8 if W == 1 else 8 // W
    return keys * key + P * (G - 1) * key + (P + 1) * 4 + P * 4 + (P + 1) * 12 + P * 2 + 20 * 4 + 32 + 320 * 4 + 16 + 2 * 64 * 2 + 16


def plan_num_cu():
    """the CU count the library plans with: DSKGPU_NUM_CU where the environment forces one (1..1024, as Tuning::read takes it), else the
    MI355X's 256"""
    try:
        n = int(os.environ.get("DSKGPU_NUM_CU", "0"))
    except ValueError:
        n = 0
    return n if 1 <= n <= 1024 else 256


def make_plan(n_upper, extra_bits, W, num_cu=None):
    """planning.h: make_plan -> (levels, P1, P2), or None where it gives up"""
    if num_cu is None:
        num_cu = plan_num_cu()
    target = TARGET_KEYS[W]
    F = ((n_upper + target - 1) // target) << extra_bits
    F = max(F, 2)
    if F <= 1024:
        return 1, F, 1
    p2max = 2048
    while p2max > 64 and ascatter_lds(W, p2max) > 160 * 1024:
        p2max -= 1
    p1 = 1
    while p1 * p1 < F:
        p1 += 1
    if F >= num_cu * 64:
        p1 = max((F + p2max - 2) // (p2max - 1), num_cu, 2)
        p1 = (p1 + num_cu - 1) // num_cu * num_cu
        p1 = min(p1, 2048 - 8)
    p2 = (F + p1 - 1) // p1
    if p2 % 2 == 0 and p2 + 1 <= p2max:
        p2 += 1
    if p1 > 2048 or p2 > 2048:
        return None
    return 2, p1, p2


def probe_model(homes, slots=4096):
    """plain linear probing of distinct keys with the given home slots -> (longest run of occupied slots, counted round the end;
    does a run cross slot slots - 1 -> 0)"""
    occ = np.zeros(slots, bool)
    nxt = list(range(slots))                       # next slot that may be free, with path compression

    def free_from(s):
        path = []
        while nxt[s] != s:
            path.append(s)
            s = nxt[s]
        for p in path:
            nxt[p] = s
        return s
    assert len(homes) < slots
    for hm in homes:
        s = free_from(int(hm))
        occ[s] = True
        nxt[s] = (s + 1) % slots
    if occ.all():
        return slots, True
    start = int(np.nonzero(~occ)[0][0])
    rolled = np.roll(occ, -start)                  # begins with a free slot: runs no longer wrap
    longest = run = 0
    for o in rolled:
        run = run + 1 if o else 0
        longest = max(longest, run)
    return longest, bool(occ[slots - 1] and occ[0])


# ------------------------------------------------------------------ the inputs of tests/test_gpu_crafted_keys.py
# (built here so that tests/test_crafted_keys_restatement.py checks, without a GPU, exactly what the device tests feed)
import functools
import zlib

HI32S = (0, 0xFFFFFFFF, 0x9E3779B9)
READ_LEN = 150
CROWD_READS = {31: 26_000, 32: 26_000, 63: 31_000, 64: 31_000, 127: 28_000, 128: 30_000}      # just above 1024 sub-partitions of the width


def seed_of(*what):
    return zlib.crc32(repr(what).encode())


def alone_ns(k):
    return (1, 2, 64, 65, 400) if k == 27 else (1, 2, 64, 65, 1000)          # (k = 27: ~523 members per (hi32, low12))


def alone_low12s(n):
    """runs at the start of the table, at its end, and across its end"""
    return (0, 4095, (4096 - n // 2) % 4096)


@functools.lru_cache(maxsize=None)
def alone_family(k, n, hi32, low12):
    return family_slot(k, n, hi32, low12, np.random.default_rng(seed_of("alone", k, n, hi32, low12)))


@functools.lru_cache(maxsize=None)
def crowd_family(k, hi32, n=400):
    """the family put into the crowd: slots at the table's end (family_v3 for the top-word table of k = 63, 64)"""
    rng = np.random.default_rng(seed_of("crowd", k, hi32, n))
    if k in (63, 64):
        return family_v3(k, n, hi32, 0xFFF, rng)
    return family_slot(k, n, hi32, 4095 - 20, rng)


@functools.lru_cache(maxsize=None)
def twin_family(k, n=300, h=None):
    return twins(k, n, np.random.default_rng(seed_of("twins", k, n)), h)


@functools.lru_cache(maxsize=None)
def lookup_family(k, n, hi32=0x9E3779B9):
    """2 n members with low12 = 0xFFF: the first n are counted, the others asked for (same fingerprint, same home slot)"""
    return family_slot(k, 2 * n, hi32, 0xFFF, np.random.default_rng(seed_of("lookup", k, n)))


@functools.lru_cache(maxsize=None)
def crowd_stream(k):
    """random reads of READ_LEN bases, one per line"""
    rng = np.random.default_rng(seed_of("crowd reads", k))
    reads = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(CROWD_READS[k], READ_LEN))
    return np.concatenate([reads, np.full((len(reads), 1), 10, np.uint8)], axis=1).reshape(-1)


def crowd_kmers(k):
    return CROWD_READS[k] * (READ_LEN - k + 1)


def device_families():
    """(name, Family, fixed bit fields {(high bit, low bit): value} of h, k-mers of the input it is counted in) of every family the
    device tests use"""
    out = []
    for k in SLOT_KS:
        for hi32 in HI32S:
            for n in alone_ns(k) + ((3000,) if k in (127, 128) and hi32 == HI32S[2] else ()):
                for low12 in alone_low12s(n):
                    out.append((f"alone k={k} n={n} hi32={hi32:#x} low12={low12}", alone_family(k, n, hi32, low12), {(63, 32): hi32, (11, 0): low12}, 0))
    for k in (32, 64, 128):
        out.append((f"load limit k={k}", alone_family(k, 3585, HI32S[2], 4095), {(63, 32): HI32S[2], (11, 0): 4095}, 0))
        for n in (300, 513, 2049):
            out.append((f"lookup k={k} n={n}", lookup_family(k, n), {(63, 32): HI32S[2], (11, 0): 0xFFF}, 0))
    for k in (31, 32, 63, 64, 127):
        for hi32 in (0xFFFFFFFF, 0):
            fixed = {(63, 32): hi32, (31, 20): 0xFFF} if k in (63, 64) else {(63, 32): hi32, (11, 0): 4095 - 20}
            out.append((f"crowd k={k} hi32={hi32:#x}", crowd_family(k, hi32), fixed, crowd_kmers(k)))
    for k in (32, 63):
        fixed = {(63, 32): 0xFFFFFFFF, (31, 20): 0xFFF} if k == 63 else {(63, 32): 0xFFFFFFFF, (11, 0): 4095 - 20}
        out.append((f"chain k={k}", crowd_family(k, 0xFFFFFFFF, 600), fixed, crowd_kmers(k)))
    return out
