"""The restatement of the row load (tests/load_rows_model.py) against the CPU oracle, and parse_ascii_rows against the oracle's text.  No GPU.

The oracle identity: count bank A and bank B with abundance_min 1, concatenate their rows, load them with SUM under abundance_min a -- that is
the count of A followed by B, in rows, abundances, histogram, total and distinct.  Banks: the golden c1..c4 pairwise and the 50x set split in
two halves at a record boundary; a in {1, 2, 3}; k = 27, 31, 33 and 65.  MAX, MIN and UNIQUE on hand-made inputs.

The tests of parse_ascii_rows fail before the feature (dsk_amd has none); the others need only the model and the oracle and check the
restatement the GPU tests rely on."""
import itertools
import os

import numpy as np
import pytest

from tests import load_rows_model as M

KS = (27, 31, 33, 65)
BANKS = ("c1", "c2", "c3", "c4")
PAIRS = list(itertools.combinations(BANKS, 2)) + [("half0", "half1")]
_streams, _counts = {}, {}


def stream_of(name, oracle, golden_dir):
    if name not in _streams:
        if name.startswith("half"):
            s = oracle.load_bank(os.path.join(golden_dir, "read50x_ref10K_e001.fasta.gz"))[0]
            ends = np.nonzero(s == 10)[0]
            cut = int(ends[len(ends) // 2]) + 1                  # behind the separator of the middle record
            _streams["half0"], _streams["half1"] = np.ascontiguousarray(s[:cut]), np.ascontiguousarray(s[cut:])
        else:
            _streams[name] = np.ascontiguousarray(oracle.load_bank(os.path.join(golden_dir, name + ".fasta.gz"))[0])
    return _streams[name]


def joined(a, b):
    """A followed by B with a '\\n' between the banks"""
    a = a if len(a) and a[-1] == 10 else np.concatenate([a, np.array([10], np.uint8)])
    return np.ascontiguousarray(np.concatenate([a, b]))


def counted(name, k, oracle, golden_dir):
    if (name, k) not in _counts:
        _counts[name, k] = oracle.count(stream_of(name, oracle, golden_dir), k)
    return _counts[name, k]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("pair", PAIRS, ids=["+".join(p) for p in PAIRS])
def test_the_load_of_two_counts_is_the_count_of_both(oracle, golden_dir, pair, k):
    A, B = (counted(n, k, oracle, golden_dir) for n in pair)
    both = oracle.count(joined(stream_of(pair[0], oracle, golden_dir), stream_of(pair[1], oracle, golden_dir)), k)
    assert A.total and B.total and both.total == A.total + B.total
    kmers = np.concatenate([A.words(), B.words()])              # the rows of A (abundance_min 1), then those of B
    ab = np.concatenate([A.ab, B.ab])
    want_values = both.values()
    for a in (1, 2, 3):
        rows, rab, hist, st = M.load(kmers, ab, k, "sum", abundance_min=a)
        keep = both.ab >= a
        assert rows == [int(v) for v in want_values[keep]]
        assert (rab == both.ab[keep]).all()
        assert (hist == both.histogram(10000)).all()
        assert st["n_kmers"] == both.total and st["n_distinct"] == both.distinct and st["n_rows"] == int(keep.sum())
        assert st["n_below"] == both.distinct - int(keep.sum()) and st["n_above"] == 0 and st["n_saturated"] == 0 and st["n_in"] == len(ab)


def test_the_halves_are_cut_at_a_record_boundary(oracle, golden_dir):
    h0, h1 = stream_of("half0", oracle, golden_dir), stream_of("half1", oracle, golden_dir)
    whole = oracle.load_bank(os.path.join(golden_dir, "read50x_ref10K_e001.fasta.gz"))[0]
    assert h0[-1] == 10 and len(h0) + len(h1) == len(whole) and (joined(h0, h1) == whole).all()
    assert abs(int((h0 == 10).sum()) - int((h1 == 10).sum())) <= 2        # (the separator of the middle record closes the first half: n / 2 + 1 records and n / 2 - 1)


# ---- the other rules, by hand: k = 3, values written as letters
def v(s):
    return sum("ACTG".index(c) << (2 * (len(s) - 1 - i)) for i, c in enumerate(s))


def test_max_min_and_unique_by_hand():
    k = 3
    kmers = [v("ACA"), v("AAA"), v("ACA"), v("CAG"), v("AAA"), v("ACA")]      # canonical: ACA < TGT, AAA < TTT, CAG < CTG
    ab = [5, 2, 9, 1, 7, 3]
    assert [M.fault(x, 1, k) for x in kmers] == [None] * 6
    order = sorted({*kmers})
    for rule, want in (("sum", {v("AAA"): 9, v("ACA"): 17, v("CAG"): 1}), ("max", {v("AAA"): 7, v("ACA"): 9, v("CAG"): 1}), ("min", {v("AAA"): 2, v("ACA"): 3, v("CAG"): 1})):
        rows, rab, hist, st = M.load(kmers, ab, k, rule, histo_max=8)
        assert rows == order and list(rab) == [want[x] for x in order], rule
        assert list(hist) == [sum(1 for c in want.values() if min(c, 8) == b) for b in range(9)], rule
        assert st == {"n_in": 6, "n_distinct": 3, "n_rows": 3, "n_below": 0, "n_above": 0, "n_kmers": 27, "n_saturated": 0, "sorted_input": 0}
    rows, rab, hist, st = M.load(kmers, ab, k, "sum", abundance_min=2, abundance_max=9, histo_max=8)
    assert rows == [v("AAA")] and list(rab) == [9] and (st["n_below"], st["n_above"], st["n_rows"]) == (1, 1, 1) and list(hist) == [0, 1, 0, 0, 0, 0, 0, 0, 2]
    assert M.load(kmers, ab, k, "unique") == (2, "repeat")                     # the second ACA, not the second AAA
    rows, rab, _, st = M.load(order, [4, 5, 6], k, "unique")
    assert rows == order and list(rab) == [4, 5, 6] and st["sorted_input"] == 1 and st["n_distinct"] == 3


def test_saturation_and_the_exact_total():
    rows, rab, hist, st = M.load([v("AAA")] * 5000 + [v("CAG")], [1 << 20] * 5000 + [7], 3, "sum", abundance_max=0xFFFFFFFF)
    assert rows == [v("AAA"), v("CAG")] and list(rab) == [0xFFFFFFFF, 7]
    assert st["n_saturated"] == 1 and st["n_kmers"] == 5000 * (1 << 20) + 7 and hist[10000] == 1 and hist[7] == 1
    assert M.load([v("AAA")] * 5000, [1 << 20] * 5000, 3, "max")[1][0] == 1 << 20


def test_the_lowest_invalid_row_and_its_reason():
    k = 3
    good = [v("AAA"), v("ACA")]
    assert M.load(good + [v("TTT")], [1, 1, 1], k) == (2, "canonical")
    assert M.load(good + [1 << 6], [1, 1, 1], k) == (2, "range")
    assert M.load(good + [v("CAG")], [1, 0, 1], k) == (1, "abundance")
    assert M.load([v("TGT"), v("AAA"), 1 << 7], [1, 0, 1], k) == (0, "canonical")
    assert M.load([v("AAA"), v("AAA"), v("TTT")], [1, 1, 1], k, "unique") == (2, "canonical")       # a row invalid by itself comes before a repeat
    # palindromes of an even k are their own reverse complement: valid
    assert M.revcomp(v("ACGT"), 4) == v("ACGT") and M.fault(v("ACGT"), 1, 4) is None
    for kk in (1, 2, 5, 31, 32, 33, 64, 65, 96, 97, 128):
        x = (0x1B2D3F4A5C6E7081 * 0x9E3779B97F4A7C15 ** 3) & ((1 << (2 * kk)) - 1)
        assert M.revcomp(M.revcomp(x, kk), kk) == x
        letters = "".join("ACTG"[(x >> (2 * (kk - 1 - i))) & 3] for i in range(kk))
        rc = "".join({"A": "T", "T": "A", "C": "G", "G": "C"}[c] for c in reversed(letters))
        assert M.revcomp(x, kk) == v(rc), kk


# ---- dsk2ascii's text
@pytest.mark.parametrize("k", (5, 31, 33, 70, 128))
def test_parse_ascii_rows_is_the_inverse_of_the_text(oracle, golden_dir, k):
    from dsk_amd import parse_ascii_rows
    from dsk_amd.engine import kmer_to_string
    res = oracle.count(stream_of("c1", oracle, golden_dir), k)
    lines = oracle.ascii_lines(res, amin=1)
    if k == 5:
        lines = lines[:]                                         # (every canonical 5-mer of the bank)
    else:
        lines = lines[:2000]
    kmers, ab = parse_ascii_rows(lines, k)
    n = len(lines)
    assert kmers.dtype == np.uint64 and kmers.shape == (n, (k + 31) // 32) and ab.dtype == np.uint32 and ab.shape == (n,)
    assert (kmers == res.words()[:n]).all() and (ab == res.ab[:n]).all()
    assert [kmer_to_string(x, k) + " %d" % a for x, a in zip(M.values_of(kmers), ab)] == lines


def test_parse_ascii_rows_reads_a_file_and_names_a_malformed_line(tmp_path):
    from dsk_amd import parse_ascii_rows
    p = tmp_path / "rows.txt"
    p.write_text("AAAAC 3\nACGTA 12\n")
    kmers, ab = parse_ascii_rows(str(p), 5)
    assert kmers.tolist() == [[1], [v("ACGTA")]] and ab.tolist() == [3, 12]
    kmers, ab = parse_ascii_rows([], 70)
    assert kmers.shape == (0, 3) and ab.shape == (0,)
    good = "AAAAC 3"
    for bad, what in (("AAAA 3", "4 letters"), ("AAAACC 3", "6 letters"), ("AANAC 3", "'N'"), ("aaaac 3", "'a'"), ("AAAAC 0", "abundance"), ("AAAAC -2", "abundance"),
                      ("AAAAC x", "abundance"), ("AAAAC 4294967296", "abundance"), ("AAAAC", "expected"), ("AAAAC 3 4", "expected")):
        with pytest.raises(ValueError) as e:
            parse_ascii_rows([good, good, bad, "AAAA 1"], 5)
        assert "line 3" in str(e.value) and what in str(e.value), (bad, str(e.value))
