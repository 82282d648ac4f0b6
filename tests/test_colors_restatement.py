"""The restatement of the sample colours (tests/color_model.py) checked on the CPU: three hand-made streams whose matrices are written out
below and were worked out by hand, and the identities that tests/test_gpu_colors.py asks of the device, asked here of the model alone on the
dense streams of tests/dense_streams.py split into 3 banks at record boundaries.  No GPU is needed: nothing of the engine is run.

The hand-made cases (rows as canonical strings; positions count from 0):

  "k4"   ACGT is its own reverse complement.  Bank 0 = "AAACGT\\n" (bytes 0..6): the windows end at 3 (AAAC, a row), 4 (AACG, no row) and
         5 (ACGT, the palindromic row: ONE count).  Bank 1 = "GTTTN\\n" (7..12): one window, GTTT at 10, the reverse complement of AAAC
         -- the same row as in bank 0, in the opposite orientation.  Bank 2 is empty (its end equals bank 1's).  Bank 3 = "ACGTACGT\\n"
         (13..21): windows at 16 .. 20, ACGT at 16 and 20; CGTA, GTAC and TACG are no rows.  "AACC\\n" (22..26) lies behind the last end:
         AACC is a row, and is not counted.  first_color = 1 of 5 colours: colour 0 stays empty.
  "k3"   no newline anywhere: "ACGTT" with the ends 2 and 4.  The window ACG ends at byte 2, which is the first byte of bank 1, so it is
         bank 1's although two of its letters lie in bank 0; CGT (= ACG reversed) ends at 3, bank 1 too; GTT (= AAC) ends at 4, behind the
         last end.
  "k2"   even k, every window a palindrome: "ATAT\\n" holds AT, TA, AT.
"""
from collections import Counter

import numpy as np
import pytest

from tests import color_model as M
from tests.dense_streams import DENSE_CASES, canon, dense_stream


def as_np(text):
    return np.frombuffer(text.encode(), dtype=np.uint8).copy()


# name -> k, the rows (a count of one line per row gives them), the stream, its bank ends, n_colors, first_color, and what was worked out by
#         hand: the matrix, the stats, masks {min_count: [mask of every row]}, and for a grouping unitig[r] chosen here: sums[u][c] and
#         all_any {min_count: (all[u], any[u])}
HAND = {
    "k4": dict(k=4, rows=["ACGT", "AAAC", "AACC"], stream=as_np("AAACGT\nGTTTN\nACGTACGT\nAACC\n"), ends=[7, 13, 13, 22], n_colors=5, first_color=1,
               matrix=[[0, 1, 0, 0, 2], [0, 1, 1, 0, 0], [0, 0, 0, 0, 0]], stats=dict(n_valid=9, n_placed=5, n_rows=3, n_colors=5),
               masks={1: [0b10010, 0b00110, 0], 2: [0b10000, 0, 0]}, unitig=[0, 0, 1],
               sums=[[0, 2, 1, 0, 2], [0, 0, 0, 0, 0]], all_any={1: ([0b00010, 0], [0b10110, 0]), 2: ([0, 0], [0b10000, 0])}),
    "k3": dict(k=3, rows=["ACG", "AAC"], stream=as_np("ACGTT"), ends=[2, 4], n_colors=2, first_color=0,
               matrix=[[0, 2], [0, 0]], stats=dict(n_valid=2, n_placed=2, n_rows=2, n_colors=2),
               masks={1: [0b10, 0], 2: [0b10, 0]}, unitig=[0, 1],
               sums=[[0, 2], [0, 0]], all_any={1: ([0b10, 0], [0b10, 0]), 2: ([0b10, 0], [0b10, 0])}),
    "k2": dict(k=2, rows=["AT", "TA"], stream=as_np("ATAT\n"), ends=[5], n_colors=1, first_color=0,
               matrix=[[2], [1]], stats=dict(n_valid=3, n_placed=3, n_rows=2, n_colors=1),
               masks={1: [1, 1], 2: [1, 0]}, unitig=[0, 0],
               sums=[[3]], all_any={1: ([1], [1]), 2: ([0], [1])}),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_the_matrices_written_out_by_hand(name):
    h = HAND[name]
    assert all(canon(s) == s for s in h["rows"])
    col = M.Colours(h["rows"], h["n_colors"], h["k"])
    assert col.add(h["stream"], h["ends"], h["first_color"]) == h["stats"]
    assert col.matrix() == h["matrix"]
    for mc, want in h["masks"].items():
        assert col.mask(mc) == want, mc
    nu = max(h["unitig"]) + 1
    for mc, (want_all, want_any) in h["all_any"].items():
        total, all_, any_ = col.unitigs(h["unitig"], nu, mc)
        assert total == h["sums"] and all_ == want_all and any_ == want_any, mc


def test_the_pieces_of_the_definition():
    assert [M.bank_of(p, [2, 2, 5]) for p in range(6)] == [0, 0, 2, 2, 2, None]          # an empty bank is stepped over
    assert M.bank_of(0, []) is None
    assert M.windows(as_np("acGTn\nAC"), 2) == [(1, "AC"), (2, "CG"), (3, "AC"), (7, "AC")]  # lower case counts, N and the newline end windows
    assert M.value_to_string(0b00011011, 4) == "ACTG"
    assert M.variant_colours([[1, 2], [3, 4], [5, 6]], [(0, 5), (3, 2)]) == [[[1, 2], [5, 6]], [[3, 4], [3, 4]]]
    s = as_np("AA\nCCC\nG\nTTTT\n")
    assert M.split_at_records(s, 1) == [len(s)] and M.split_at_records(s, 3) == [7, 14, 14]
    for n in (2, 3, 5):
        ends = M.split_at_records(s, n)
        assert len(ends) == n and ends == sorted(ends) and ends[-1] == len(s) and all(s[e - 1] == 10 for e in ends)


@pytest.mark.parametrize("k,seed", DENSE_CASES)
def test_identities_on_the_model_alone(k, seed):
    """what the device is asked in tests/test_gpu_colors.py part 2, with the counted stream coloured: here the count is a Counter"""
    stream = dense_stream(k, seed)
    wins = M.windows(stream, k)
    abundance = Counter(s for _, s in wins)
    rows = sorted(abundance)
    unitig = [r // 3 for r in range(len(rows))]                                # any grouping of the rows serves the reductions
    nu = unitig[-1] + 1
    ends = M.split_at_records(stream, 3)
    assert len(set(ends)) == 3 and all(stream[e - 1] == 10 for e in ends)

    one = M.Colours(rows, 3, k)
    st = one.add(stream, ends, 0, wins)
    C = np.array(one.matrix(), dtype=np.int64)
    assert (C.sum(1) == [abundance[s] for s in rows]).all()                   # (a)
    for c in range(3):                                                        # (b) a bank alone counts what its column holds
        lo = 0 if c == 0 else ends[c - 1]
        alone = Counter(s for _, s in M.windows(stream[lo: ends[c]], k))
        assert (C[:, c] == [alone[s] for s in rows]).all(), c
    assert st["n_placed"] == C.sum() == st["n_valid"] == len(wins)            # (c) every k-mer of the stream is a row here
    total, all_, any_ = one.unitigs(unitig, nu)
    total = np.array(total, dtype=np.int64)
    assert (total.sum(1) == np.bincount(unitig, weights=C.sum(1)).astype(np.int64)).all()      # (d)
    assert all(a & ~b == 0 for a, b in zip(all_, any_)) and all(b != 0 for b in any_)
    for mc in (1, 2, 3):
        m = one.mask(mc)
        assert m == [sum(1 << c for c in range(3) if C[r, c] >= mc) for r in range(len(rows))]

    three = M.Colours(rows, 3, k)                                             # (e) three calls with one bank each: the banks end with a newline
    for c in range(3):
        lo = 0 if c == 0 else ends[c - 1]
        three.add(stream[lo: ends[c]], [ends[c] - lo], c)
    assert three.matrix() == one.matrix()

    twice = M.Colours(rows, 3, k)                                             # (f)
    twice.add(stream, ends, 0, wins)
    twice.add(stream, ends, 0, wins)
    assert (np.array(twice.matrix(), dtype=np.int64) == 2 * C).all()
