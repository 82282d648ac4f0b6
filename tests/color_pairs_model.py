"""The restatement of dskgpu_colors_pairs / dskgpu_colors_marks (include/dskgpu.h: THRESHOLDED CELL, PAIR MATRICES, RULE) and of the sample
distances, in plain Python over a list-of-lists matrix.  Not a test module; it shares no code with the engine.

Every sum is a Python int, so nothing can wrap; every distance that is rational is a fractions.Fraction, the two with a square root are floats
computed from Fractions.  A distance whose denominator is zero is None.
"""
import math
from fractions import Fraction

INVERT = 1
DISTANCES = ("jaccard", "sorensen", "ochiai", "kulczynski", "bray_curtis", "ruzicka", "ab_jaccard", "ab_ochiai", "ab_sorensen")


def thresholded(C, min_count):
    assert min_count >= 1
    return [[v if v >= min_count else 0 for v in row] for row in C]


def pairs(C, min_count=1, select=None, n_colors=None):
    """-> (shared, cross, min_sum: lists of lists of int, stats) over the rows r with select is None or select[r] != 0"""
    nc = n_colors if n_colors is not None else len(C[0])
    shared = [[0] * nc for _ in range(nc)]
    cross = [[0] * nc for _ in range(nc)]
    min_sum = [[0] * nc for _ in range(nc)]
    n_selected = n_present = 0
    for r, row in enumerate(thresholded(C, min_count)):
        assert len(row) == nc
        if select is not None and not select[r]:
            continue
        n_selected += 1
        there = [c for c in range(nc) if row[c] > 0]
        n_present += 1 if there else 0
        for i in there:
            for j in there:
                shared[i][j] += 1
                cross[i][j] += row[i]
                min_sum[i][j] += min(row[i], row[j])
    return shared, cross, min_sum, dict(n_rows=len(C), n_selected=n_selected, n_present=n_present, n_colors=nc)


def diagonal(C, min_count=1, select=None):
    """the hand-computable part: -> (N[c] = the selected rows with C'[r][c] > 0, T[c] = the sum of C'[r][c] over them), column by column"""
    nc = len(C[0])
    rows = [row for r, row in enumerate(C) if select is None or select[r]]
    N = [sum(1 for row in rows if row[c] >= min_count) for c in range(nc)]
    T = [sum(row[c] for row in rows if row[c] >= min_count) for c in range(nc)]
    return N, T


def mask(row, min_count):
    return sum(1 << c for c, v in enumerate(row) if v >= min_count)


def marks(C, n_colors, rule):
    """rule: dict with need_all, need_none, min_count, min_present, max_present, invert (all optional) -> (the list of 0 / 1, the stats)"""
    need_all, need_none = rule.get("need_all", 0), rule.get("need_none", 0)
    min_count, min_present, max_present = rule.get("min_count", 1), rule.get("min_present", 0), rule.get("max_present", 0)
    flip = 1 if rule.get("invert", False) else 0
    assert min_count >= 1 and (need_all | need_none) >> n_colors == 0
    keep = []
    for row in C:
        assert len(row) == n_colors
        m = mask(row, min_count)
        present = bin(m).count("1")
        keep0 = (m & need_all) == need_all and (m & need_none) == 0 and present >= min_present and (max_present == 0 or present <= max_present)
        keep.append((1 if keep0 else 0) ^ flip)
    return keep, dict(n_rows=len(C), n_kept=sum(keep))


def _ratio(num, den):
    return None if den == 0 else Fraction(num, den)


def distances(shared, cross, min_sum):
    """-> {name: [[Fraction, float or None]]}; None where the denominator is zero"""
    nc = len(shared)
    N, T = [shared[i][i] for i in range(nc)], [cross[i][i] for i in range(nc)]
    out = {name: [[None] * nc for _ in range(nc)] for name in DISTANCES}

    def one_minus(x):
        return None if x is None else 1 - x

    for i in range(nc):
        for j in range(nc):
            a, s = shared[i][j], min_sum[i][j]
            out["jaccard"][i][j] = one_minus(_ratio(a, N[i] + N[j] - a))
            out["sorensen"][i][j] = one_minus(_ratio(2 * a, N[i] + N[j]))
            out["ochiai"][i][j] = None if N[i] * N[j] == 0 else 1.0 - a / math.sqrt(N[i] * N[j])
            x, y = _ratio(a, N[i]), _ratio(a, N[j])
            out["kulczynski"][i][j] = None if x is None or y is None else 1 - (x + y) / 2
            out["bray_curtis"][i][j] = one_minus(_ratio(2 * s, T[i] + T[j]))
            out["ruzicka"][i][j] = one_minus(_ratio(s, T[i] + T[j] - s))
            U, V = _ratio(cross[i][j], T[i]), _ratio(cross[j][i], T[j])
            if U is None or V is None:
                continue
            UV = U * V
            out["ab_jaccard"][i][j] = None if U + V - UV == 0 else 1 - UV / (U + V - UV)
            out["ab_ochiai"][i][j] = 1.0 - math.sqrt(UV)
            out["ab_sorensen"][i][j] = None if U + V == 0 else 1 - 2 * UV / (U + V)
    return out
