"""The restatement of dskgpu_load_rows (include/dskgpu.h) in Python ints and numpy -- TEST INFRASTRUCTURE ONLY.

A load is a count whose input is (k-mer, abundance) pairs: every pair must be valid by itself (value < 4^k, value <= its reverse complement in
the order A=0 C=1 T=2 G=3, abundance >= 1), equal values are combined (sum in unbounded ints, stored saturated at 2^32 - 1; max; min; or, with
"unique", refused), the histogram is taken over all distinct values, and the values with abundance_min <= combined <= abundance_max are the
rows, ascending.  tests/test_load_rows_restatement.py checks this model against the CPU oracle's count of two banks; tests/test_gpu_load_rows.py
checks the device against it."""
import numpy as np

STATS = ("n_in", "n_distinct", "n_rows", "n_below", "n_above", "n_kmers", "n_saturated", "sorted_input")
SAT = 0xFFFFFFFF
_RC = bytes(((b & 3) << 6 | (b >> 2 & 3) << 4 | (b >> 4 & 3) << 2 | (b >> 6 & 3)) ^ 0xAA for b in range(256))     # the four bases of a byte reversed and complemented


def revcomp(v: int, k: int) -> int:
    nb = (2 * k + 7) // 8
    return int.from_bytes(v.to_bytes(nb, "big").translate(_RC), "little") >> (8 * nb - 2 * k)


def canonical(v: int, k: int) -> int:
    return min(v, revcomp(v, k))


def words_of(values, k: int) -> np.ndarray:
    """Python ints -> uint64[n, ceil(k / 32)], least significant word first (the layout of the ABI)"""
    w = (k + 31) // 32
    return np.array([[(int(v) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(w)] for v in values], dtype=np.uint64).reshape(-1, w)


def values_of(words) -> list:
    words = np.asarray(words, dtype=np.uint64)
    if words.ndim == 1:
        return [int(v) for v in words]
    return [sum(int(x) << (64 * i) for i, x in enumerate(r)) for r in words]


def fault(v: int, a: int, k: int):
    """what is wrong with one pair by itself, or None; the order of the checks is the library's"""
    if v >> (2 * k):
        return "range"
    if revcomp(v, k) < v:
        return "canonical"
    if a < 1:
        return "abundance"
    return None


def load(kmers, abundance, k, combine="sum", abundance_min=1, abundance_max=2147483647, histo_max=10000):
    """kmers: Python ints, or the words array of the ABI; abundance: ints.
    -> (rows: ascending ints, abundance: uint32, histogram: uint64[histo_max + 1], stats) or (index, reason) of the lowest invalid row:
    reason is "range", "canonical" or "abundance"; under "unique", once every row is valid by itself, "repeat" at the lowest index whose
    value also stands at a lower index."""
    values = values_of(kmers) if isinstance(kmers, np.ndarray) else [int(v) for v in kmers]
    ab = [int(a) for a in abundance]
    assert len(values) == len(ab) and combine in ("sum", "max", "min", "unique")
    for i, (v, a) in enumerate(zip(values, ab)):
        why = fault(v, a, k)
        if why:
            return i, why
    acc = {}
    for i, (v, a) in enumerate(zip(values, ab)):
        if v not in acc:
            acc[v] = a
        elif combine == "unique":
            return i, "repeat"
        else:
            acc[v] = acc[v] + a if combine == "sum" else max(acc[v], a) if combine == "max" else min(acc[v], a)
    hist = np.zeros(histo_max + 1, dtype=np.uint64)
    rows, out_ab = [], []
    below = above = saturated = 0
    for v in sorted(acc):
        c = acc[v]
        if c > SAT:
            saturated += 1
            c = SAT
        hist[min(c, histo_max)] += 1
        if c < abundance_min:
            below += 1
        elif c > abundance_max:
            above += 1
        else:
            rows.append(v)
            out_ab.append(c)
    stats = {"n_in": len(values), "n_distinct": len(acc), "n_rows": len(rows), "n_below": below, "n_above": above, "n_kmers": sum(ab),
             "n_saturated": saturated, "sorted_input": int(all(x < y for x, y in zip(values, values[1:])))}
    return rows, np.array(out_ab, dtype=np.uint32), hist, stats
