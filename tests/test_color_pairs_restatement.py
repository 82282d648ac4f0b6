"""The restatement of the sample comparison (tests/color_pairs_model.py) on matrices written out by hand, its identities on random matrices,
and dsk_amd.sample_distances against the model's Fractions.  No GPU is needed.

The GPU suite (tests/test_gpu_color_pairs.py) compares the device with this model; here the model is compared with numbers a reader can check
with a pencil."""
import random
import warnings
from fractions import Fraction as F

import numpy as np
import pytest

from tests import color_pairs_model as M

# four rows, three colours; colour 2 is empty
EMPTY = [[3, 1, 0],
         [0, 2, 0],
         [5, 0, 0],
         [1, 1, 0]]
# five rows, three colours; min_count = 2 removes every 1
MIXED = [[3, 1, 2],
         [1, 1, 0],
         [0, 4, 4],
         [2, 0, 7],
         [0, 0, 0]]


def test_a_matrix_with_an_empty_colour():
    shared, cross, min_sum, st = M.pairs(EMPTY)
    assert shared == [[3, 2, 0], [2, 3, 0], [0, 0, 0]]
    assert cross == [[9, 4, 0], [2, 4, 0], [0, 0, 0]]                        # cross[0][1] = 3 + 1 (rows 0 and 3 hold colour 1)
    assert min_sum == [[9, 2, 0], [2, 4, 0], [0, 0, 0]]                      # min(3, 1) + min(1, 1)
    assert st == dict(n_rows=4, n_selected=4, n_present=4, n_colors=3)
    assert M.diagonal(EMPTY) == ([3, 3, 0], [9, 4, 0])


def test_min_count_two_changes_the_answer():
    s1, c1, m1, st1 = M.pairs(MIXED, 1)
    assert s1 == [[3, 2, 2], [2, 3, 2], [2, 2, 3]]
    assert c1 == [[6, 4, 5], [2, 6, 5], [9, 6, 13]]
    assert m1 == [[6, 2, 4], [2, 6, 5], [4, 5, 13]]
    assert st1 == dict(n_rows=5, n_selected=5, n_present=4, n_colors=3)
    s2, c2, m2, st2 = M.pairs(MIXED, 2)                                      # the cells left: row 0: 3 . 2; row 2: . 4 4; row 3: 2 . 7
    assert s2 == [[2, 0, 2], [0, 1, 1], [2, 1, 3]]
    assert c2 == [[5, 0, 5], [0, 4, 4], [9, 4, 13]]
    assert m2 == [[5, 0, 4], [0, 4, 4], [4, 4, 13]]
    assert st2 == dict(n_rows=5, n_selected=5, n_present=3, n_colors=3)     # row 1 has no cell left
    assert (s1, c1, m1) != (s2, c2, m2)


def test_a_select():
    select = [1, 0, 7, 0, 1]                                                 # rows 0, 2 and 4; any non-zero byte selects
    shared, cross, min_sum, st = M.pairs(MIXED, 1, select)
    assert shared == [[1, 1, 1], [1, 2, 2], [1, 2, 2]]
    assert cross == [[3, 3, 3], [1, 5, 5], [2, 6, 6]]
    assert min_sum == [[3, 1, 2], [1, 5, 5], [2, 5, 6]]
    assert st == dict(n_rows=5, n_selected=3, n_present=2, n_colors=3)
    assert M.pairs(MIXED, 1, [0] * 5)[:3] == tuple([[0] * 3 for _ in range(3)] for _ in range(3))
    assert M.pairs(MIXED, 1, [1] * 5) == M.pairs(MIXED, 1)


def test_cells_that_would_wrap_32_bits():
    big = 2 ** 32 - 1
    C = [[big, 1], [1, big], [big, big]]
    shared, cross, min_sum, _ = M.pairs(C)
    assert shared == [[3, 3], [3, 3]]
    assert cross == [[2 * big + 1, 2 * big + 1], [2 * big + 1, 2 * big + 1]]
    assert min_sum == [[2 * big + 1, big + 2], [big + 2, 2 * big + 1]]
    assert M.diagonal(C) == ([3, 3], [2 * big + 1, 2 * big + 1])


def test_marks_by_hand():
    keep = lambda **rule: M.marks(MIXED, 3, rule)[0]      # noqa: E731
    assert [M.mask(r, 1) for r in MIXED] == [7, 3, 6, 5, 0] and [M.mask(r, 2) for r in MIXED] == [5, 0, 6, 5, 0]
    assert keep() == [1, 1, 1, 1, 1]                                         # the empty rule keeps everything
    assert keep(need_all=1) == [1, 1, 0, 1, 0]
    assert keep(need_all=1, need_none=2) == [0, 0, 0, 1, 0]                  # private to colours 0 and 2
    assert keep(min_present=3) == [1, 0, 0, 0, 0]                            # the core
    assert keep(min_present=1, max_present=2) == [0, 1, 1, 1, 0]             # the accessory part
    assert keep(min_present=1, max_present=2, invert=True) == [1, 0, 0, 0, 1]
    assert keep(need_all=5, min_count=2) == [1, 0, 0, 1, 0]
    assert keep(max_present=1, min_count=2) == [0, 1, 0, 0, 1]
    assert M.marks(MIXED, 3, dict(need_all=1)) == ([1, 1, 0, 1, 0], dict(n_rows=5, n_kept=3))


def random_matrix(rng, n, nc, big=False):
    top = 2 ** 32 - 1 if big else 5
    return [[rng.choice((0, 0, 1, rng.randint(1, top))) for _ in range(nc)] for _ in range(n)]


@pytest.mark.parametrize("seed", range(6))
def test_identities(seed):
    rng = random.Random(seed)
    n, nc = rng.randint(1, 40), rng.randint(1, 7)
    C = random_matrix(rng, n, nc, big=seed % 2 == 1)
    select = None if seed < 2 else [rng.randint(0, 1) for _ in range(n)]
    for mc in (1, 2):
        shared, cross, min_sum, st = M.pairs(C, mc, select)
        N, T = M.diagonal(C, mc, select)
        for i in range(nc):
            assert shared[i][i] == N[i] and cross[i][i] == T[i] and min_sum[i][i] == cross[i][i]
            for j in range(nc):
                assert shared[i][j] == shared[j][i] and min_sum[i][j] == min_sum[j][i]
                assert shared[i][j] <= min(N[i], N[j])
                assert min_sum[i][j] <= min(cross[i][j], cross[j][i])
        assert st["n_present"] <= st["n_selected"] <= st["n_rows"] == n
        keep, mst = M.marks(C, nc, dict(min_count=mc, min_present=1))
        assert mst["n_kept"] == M.pairs(C, mc)[3]["n_present"]                # a row is present exactly when its mask is not empty
        assert M.pairs(C, mc, keep)[:3] == M.pairs(C, mc)[:3]                 # and only those rows carry anything


def check_distances(shared, cross, min_sum):
    from dsk_amd import sample_distances
    want = M.distances(shared, cross, min_sum)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                       # there are no warnings
        got = sample_distances(np.array(shared, dtype=np.uint64), np.array(cross, dtype=np.uint64), np.array(min_sum, dtype=np.uint64))
    assert sorted(got) == sorted(M.DISTANCES)
    nc = len(shared)
    for name in M.DISTANCES:
        g = got[name]
        assert g.dtype == np.float64 and g.shape == (nc, nc)
        for i in range(nc):
            for j in range(nc):
                w = want[name][i][j]
                if w is None:
                    assert np.isnan(g[i][j]), (name, i, j)
                else:
                    assert abs(g[i][j] - float(w)) <= 1e-12, (name, i, j, g[i][j], w)      # values in [0, 2], a handful of float64 operations
                    assert -1e-12 <= g[i][j] <= 2
    return got, want


def test_distances_by_hand():
    shared, cross, min_sum, _ = M.pairs(MIXED, 2)
    got, want = check_distances(shared, cross, min_sum)
    # N = 2, 1, 3; T = 5, 4, 13
    assert want["jaccard"][0][2] == 1 - F(2, 2 + 3 - 2) and want["jaccard"][0][1] == 1
    assert want["sorensen"][1][2] == 1 - F(2, 4)
    assert want["kulczynski"][0][2] == 1 - (F(2, 2) + F(2, 3)) / 2
    assert want["bray_curtis"][0][2] == 1 - F(8, 18) and want["ruzicka"][0][2] == 1 - F(4, 14)
    U, V = F(5, 5), F(9, 13)
    assert want["ab_jaccard"][0][2] == 1 - U * V / (U + V - U * V) and want["ab_sorensen"][0][2] == 1 - 2 * U * V / (U + V)
    for name in M.DISTANCES:
        assert all(want[name][i][i] == 0 for i in range(3)), name             # a zero diagonal
        assert (np.diag(got[name]) == 0).all(), name


def test_distances_with_an_empty_sample_are_nan_where_the_denominator_is_zero():
    shared, cross, min_sum, _ = M.pairs(EMPTY)
    got, want = check_distances(shared, cross, min_sum)
    for name in M.DISTANCES:
        assert want[name][2][2] is None and np.isnan(got[name][2][2]), name  # the empty sample against itself: 0 / 0 everywhere
    assert want["jaccard"][0][2] == 1 and want["sorensen"][2][1] == 1        # a denominator that is not zero: the samples share nothing
    for name in ("ochiai", "kulczynski", "ab_jaccard", "ab_ochiai", "ab_sorensen"):
        assert want[name][0][2] is None and want[name][2][0] is None, name
    assert (np.diag(got["jaccard"])[:2] == 0).all()


@pytest.mark.parametrize("seed", range(4))
def test_distances_on_random_matrices_are_symmetric(seed):
    rng = random.Random(100 + seed)
    C = random_matrix(rng, rng.randint(5, 60), rng.randint(2, 6), big=seed == 3)
    shared, cross, min_sum, _ = M.pairs(C, 1 + seed % 2)
    got, _ = check_distances(shared, cross, min_sum)
    for name in M.DISTANCES:
        g = got[name]
        assert ((g == g.T) | (np.isnan(g) & np.isnan(g.T))).all(), name


def test_distances_take_tensors_and_refuse_other_shapes():
    torch = pytest.importorskip("torch")
    from dsk_amd import sample_distances
    shared, cross, min_sum, _ = M.pairs(MIXED)
    as_t = lambda m: torch.tensor(m, dtype=torch.int64)      # noqa: E731
    a, b = sample_distances(as_t(shared), as_t(cross), as_t(min_sum)), sample_distances(shared, cross, min_sum)
    assert all((a[name] == b[name]).all() for name in M.DISTANCES)
    with pytest.raises(ValueError):
        sample_distances(shared, cross, [[1, 2]])
