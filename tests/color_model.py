"""The sample colours (include/dskgpu.h: "sample colours for rows, unitigs and variants"): CELL, MASK, UNITIG COLOURS and VARIANT COLOURS
restated on strings in plain Python.  Not a test module: tests/test_colors_restatement.py checks it on the CPU before
tests/test_gpu_colors.py trusts it on the device.  It shares no code with the engine: k-mers are STRINGS in the lexicographic canonical form
of tests/dense_streams.py (canon), cells are counted in a Counter, masks are Python ints.  Its inputs are the rows (canonical strings in
result order), unitig[r] of every row and the stream with its bank ends."""
from collections import Counter

from tests.byte_streams import upper_bases
from tests.dense_streams import canon

_BASES = frozenset(b"ACGTacgt")


def value_to_string(value, k):
    """the k letters of a k-mer value: two bits per base, A C T G = 0 1 2 3, the first base in the highest bits"""
    return "".join("ACTG"[(value >> (2 * (k - 1 - i))) & 3] for i in range(k))


def rows_of(values, k):
    """the rows' values (Python ints, result order) -> their canonical strings"""
    return [canon(value_to_string(int(v), k)) for v in values]


def windows(stream, k):
    """-> [(p, canonical k-mer)] of the valid windows of the stream, p = the byte the window ends at"""
    raw = bytes(stream)
    text = upper_bases(raw)
    out, run = [], 0
    for p in range(len(raw)):
        run = run + 1 if raw[p] in _BASES else 0
        if run >= k:
            out.append((p, canon(text[p - k + 1: p + 1])))
    return out


def bank_of(p, ends):
    """the least b with p < ends[b]; None behind the last end"""
    for b, e in enumerate(ends):
        if p < e:
            return b
    return None


class Colours:
    """the matrix of `rows` (canonical strings, result order) with n_colors columns"""

    def __init__(self, rows, n_colors, k):
        assert 1 <= n_colors <= 64
        self.k, self.n_colors, self.n_rows = k, n_colors, len(rows)
        self.index = {s: r for r, s in enumerate(rows)}
        assert len(self.index) == len(rows)
        self.cells = Counter()                                                # (r, c) -> count

    def add(self, stream, ends, first_color=0, wins=None):
        """one dskgpu_colors_add -> its stats.  wins: windows(stream, k), when the caller has them already"""
        ends = [int(e) for e in ends]
        assert all(a <= b for a, b in zip(ends, ends[1:])) and (not ends or ends[-1] <= len(stream)) and first_color + len(ends) <= self.n_colors
        n_valid = n_placed = 0
        for p, s in (windows(stream, self.k) if wins is None else wins):
            b = bank_of(p, ends)
            if b is None:
                continue
            n_valid += 1
            r = self.index.get(s)
            if r is not None:
                n_placed += 1
                self.cells[(r, first_color + b)] += 1
        return dict(n_valid=n_valid, n_placed=n_placed, n_rows=self.n_rows, n_colors=self.n_colors)

    def matrix(self):
        """-> [[C[r][c] for c] for r], modulo 2^32"""
        C = [[0] * self.n_colors for _ in range(self.n_rows)]
        for (r, c), v in self.cells.items():
            C[r][c] = v & 0xFFFFFFFF
        return C

    def mask(self, min_count=1):
        assert min_count >= 1
        m = [0] * self.n_rows
        for (r, c), v in self.cells.items():
            if (v & 0xFFFFFFFF) >= min_count:
                m[r] |= 1 << c
        return m

    def unitigs(self, unitig, n_unitigs, min_count=1):
        """unitig[r] of every row -> (sum[u][c], all[u], any[u])"""
        total = [[0] * self.n_colors for _ in range(n_unitigs)]
        for (r, c), v in self.cells.items():
            total[int(unitig[r])][c] += v & 0xFFFFFFFF
        all_, any_ = [(1 << self.n_colors) - 1] * n_unitigs, [0] * n_unitigs
        for r, m in enumerate(self.mask(min_count)):
            u = int(unitig[r])
            all_[u] &= m
            any_[u] |= m
        return total, all_, any_


def variant_colours(total, alleles):
    """alleles: [(A, B)] oriented unitigs of the variants -> vsum[v][0 / 1][c]"""
    return [[list(total[int(a) >> 1]), list(total[int(b) >> 1])] for a, b in alleles]


def split_at_records(stream, n_banks):
    """bank ends that cut the stream behind newlines into n_banks banks of about equal size (the last ends at the stream's end)"""
    raw = bytes(stream)
    ends = []
    for i in range(1, n_banks):
        at = raw.find(b"\n", len(raw) * i // n_banks)
        ends.append(len(raw) if at < 0 else at + 1)
    return ends + [len(raw)]
