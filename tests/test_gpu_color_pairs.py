"""The samples compared with each other on the device (include/dskgpu.h: dskgpu_colors_pairs / _colors_load / _colors_marks; csrc/colors.h).

All comparisons are exact integers.  Part 1 compares the device with the restatement of tests/color_pairs_model.py (which the CPU suite
checks first), fed with dskgpu_colors_rows' copy of real colours.  Part 2 loads matrices of every shape at which the two pair kernels can go
wrong -- this is where a cell of 2^32 - 1 meets a partial sum.  Part 3 is identities on the device alone.  Part 4 is the contract.  Every
output has guard bytes around it and every input is checked unchanged.

Every test here fails before the feature: KmerCounter has no colors_pairs and the library no dskgpu_colors_pairs.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import color_model as CM      # noqa: E402
from tests import color_pairs_model as M      # noqa: E402
from tests.dense_streams import dense_stream      # noqa: E402
from tests.test_correct_restatement import handmade_correct      # noqa: E402
from tests.test_gpu_colors import add, read_rows      # noqa: E402
from tests.test_gpu_read_summaries import GUARD, as_np, guarded, inside, put      # noqa: E402
from tests.test_gpu_unitigs import code_of, count, stream_of      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_STATE = -1, -4
BIG = 2 ** 32 - 1
_colors_h = open(os.path.join(ROOT, "dsk_amd", "csrc", "colors.h")).read()
# n_colors up to REG_SWITCH take k_color_pairs_reg, above it k_color_pairs_tile, which stages TILE_ROWS rows at a time
REG_SWITCH, REG_MAX, TILE_ROWS, BLOCK = (int(re.search(r"^#define %s (\d+)" % name, _colors_h, flags=re.M).group(1))
                                         for name in ("CP_REG_SWITCH", "CP_REG_MAX", "CP_TILE_ROWS", "CP_BLOCK"))
N_COLORS = sorted({1, 2, 3, 4, 5, 8, 31, 32, 33, 63, 64} | {max(REG_SWITCH, 1), REG_SWITCH + 1})      # both sides of the switch, whatever it is
assert REG_SWITCH == 8 and 8 in N_COLORS and 9 in N_COLORS and REG_SWITCH <= REG_MAX
# 1, 2, a wave, a block and a tile +- 1, and five tiles plus one row
N_ROWS = sorted({1, 2, 63, 64, 65, 255, 256, 257, TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, BLOCK - 1, BLOCK, BLOCK + 1, 5 * TILE_ROWS + 1}, reverse=True)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


# ------------------------------------------------------------------ one call each, guard bytes round every output
def device_pairs(kc, dev, nc, min_count=1, select=None, singles=False):
    """-> (shared, cross, min_sum as lists of lists of int, the stats); select: None or one byte per row, handed over at an odd address"""
    bufs = [guarded(dev, 8 * nc * nc) for _ in range(3)]
    sel = None if select is None else put(dev, np.asarray(select, dtype=np.uint8), 1)
    torch.cuda.synchronize()
    sp = 0 if select is None or len(select) == 0 else sel.data_ptr() + 1
    st = kc.colors_pairs(min_count, *(b.data_ptr() + GUARD for b in bufs), sp)
    torch.cuda.synchronize()
    out = [inside(b, 8 * nc * nc).view(np.uint64).reshape(nc, nc) for b in bufs]
    if singles:                                                               # one by one, the other two NULL
        for x in range(3):
            one = guarded(dev, 8 * nc * nc)
            torch.cuda.synchronize()
            assert kc.colors_pairs(min_count, *(one.data_ptr() + GUARD if y == x else 0 for y in range(3)), sp) == st
            torch.cuda.synchronize()
            assert (inside(one, 8 * nc * nc).view(np.uint64).reshape(nc, nc) == out[x]).all(), x
    if sel is not None:
        back = sel.cpu().numpy()
        assert (back[1: 1 + len(select)] == np.asarray(select, dtype=np.uint8)).all() and back[0] == 10 and (back[1 + len(select):] == 10).all(), "the input is left as it was"
    return [[[int(v) for v in row] for row in m] for m in out] + [st]


def device_marks(kc, dev, n, **rule):
    """-> (u8[n] written at an odd address, the stats)"""
    buf = guarded(dev, n, 1)
    torch.cuda.synchronize()
    st = kc.colors_marks(buf.data_ptr() + GUARD + 1, **rule)
    torch.cuda.synchronize()
    return inside(buf, n, 1), st


def load(kc, dev, mat, off=0):
    """dskgpu_colors_load of mat (uint32[n, nc]) from an address 4 * off bytes behind a 16-byte boundary; the input is checked unchanged"""
    n, nc = mat.shape
    raw = np.ascontiguousarray(mat, dtype=np.uint32).view(np.uint8).reshape(-1)
    src = put(dev, raw, 4 * off)
    torch.cuda.synchronize()
    kc.colors_load(src.data_ptr() + 4 * off if n else 0, nc)
    back = src.cpu().numpy()
    assert (back[4 * off: 4 * off + len(raw)] == raw).all() and (back[: 4 * off] == 10).all() and (back[4 * off + len(raw):] == 10).all(), "the input is left as it was"


def check_pairs(kc, dev, mat, min_count=1, select=None, singles=False, want=None):
    got = device_pairs(kc, dev, mat.shape[1], min_count, select, singles)
    if want is None:
        want = M.pairs(mat.tolist(), min_count, select)
    for name, g, w in zip(("shared", "cross", "min_sum", "stats"), got, want):
        assert g == w, (name, mat.shape, min_count, select is not None)
    return got


def some_select(n, seed=0):
    return (np.random.default_rng(1000 + seed).integers(0, 3, n) % 2 * 255).astype(np.uint8)      # 0 or 255, about one row in three


def rules_for(nc):
    top = 1 << (nc - 1)
    return [dict(), dict(need_all=1), dict(need_all=top, need_none=1 if nc > 1 else 0), dict(min_present=nc), dict(min_present=1, max_present=max(nc - 1, 1)),
            dict(min_present=2, invert=True), dict(need_all=1, min_count=2), dict(max_present=1, min_count=2, invert=True)]


def check_marks(kc, dev, mat, rules):
    n, nc = mat.shape
    for rule in rules:
        keep, st = device_marks(kc, dev, n, **rule)
        want, want_st = M.marks(mat.tolist(), nc, rule)
        assert keep.tolist() == want and st == want_st, rule


def trim(kc, dev, n):
    """the first n rows of the result are the result"""
    have = kc.result_device()[2]
    assert have >= n
    if have > n:
        keep = torch.zeros(have, dtype=torch.uint8, device=dev)
        keep[:n] = 1
        assert kc.filter_rows_tensor(keep) == n


# ------------------------------------------------------------------ 1. the model on real colours
_parts = {}


def golden_part(oracle, golden_dir):
    if "g" not in _parts:
        whole = stream_of("golden", oracle, golden_dir)
        ends = np.flatnonzero(whole == 10)
        _parts["g"] = (whole[int(ends[99]) + 1: int(ends[399]) + 1].copy(), whole[: int(ends[299]) + 1].copy())      # records 100 .. 399 counted, 0 .. 299 coloured
    return _parts["g"]


def streams(kind, k, oracle, golden_dir):
    """-> (the stream to count, the stream to colour)"""
    if kind == "golden":
        return golden_part(oracle, golden_dir)
    if kind == "hand":
        counted, s, _ = handmade_correct(k)
        return counted, np.concatenate([s, as_np("\n"), counted])
    s = dense_stream(k, int(kind.split(":")[1]))
    return s, s


@pytest.mark.parametrize("kind,k", [("golden", k) for k in (12, 31, 33, 65)] + [("hand", k) for k in (12, 31, 33, 65)] + [("dense:1", 12), ("dense:2", 9)])
def test_device_equals_the_model_on_real_colours(oracle, golden_dir, dev, kind, k):
    """3 and 5 banks, both row orders: pairs at min_count 1 and 2, with and without a select, and the marks of a few rules, against the model
    fed with the matrix that dskgpu_colors_rows copies out"""
    counted, stream = streams(kind, k, oracle, golden_dir)
    placed = 0
    for order in (False, True):
        with count(counted, dev, k, abundance_min=1, partition_order=order) as kc:
            n = kc.result_device()[2]
            for nb in (3, 5):
                kc.colors_begin(nb)
                placed += add(kc, dev, stream, CM.split_at_records(stream, nb))["n_placed"]
                mat = read_rows(kc, dev, n, nb)[0]
                for mc in (1, 2):
                    got = check_pairs(kc, dev, mat, mc, singles=mc == 1)
                    check_pairs(kc, dev, mat, mc, some_select(n, nb).tolist())
                    assert got[3]["n_rows"] == n and got[3]["n_colors"] == nb
                check_marks(kc, dev, mat, rules_for(nb))
                assert (read_rows(kc, dev, n, nb)[0] == mat).all()              # pairs and marks leave the matrix alone
    assert placed > 0


# ------------------------------------------------------------------ 2. loaded matrices
def matrices(n, nc, seed):
    """-> [(name, uint32[n, nc], closed form or None)]; closed form: the value v of a matrix whose every cell is v"""
    rng = np.random.default_rng(seed)
    sparse = np.where(rng.random((n, nc)) < 0.25, rng.choice(np.array([1, 1, 2, 3, 1000, BIG], dtype=np.uint32), (n, nc)), 0).astype(np.uint32)
    column = np.zeros((n, nc), dtype=np.uint32)
    column[:, nc // 2] = 5
    alternating = np.zeros((n, nc), dtype=np.uint32)
    alternating[:, nc - 1] = np.where(np.arange(n) % 2 == 0, BIG, 1)
    return [("sparse", sparse, None), ("zero", np.zeros((n, nc), dtype=np.uint32), 0), ("equal", np.full((n, nc), 7, dtype=np.uint32), 7), ("column", column, None),
            ("big", np.full((n, nc), BIG, dtype=np.uint32), BIG), ("alternating", alternating, None)]


def closed_form(n, nc, v, min_count, select):
    """every cell is v: every entry of shared is the number of selected rows (when v counts), every entry of cross and min_sum v times that"""
    n_sel = n if select is None else int(np.count_nonzero(select))
    there = n_sel if v >= min_count else 0
    full = lambda x: [[x] * nc for _ in range(nc)]      # noqa: E731
    return full(there), full(there * v), full(there * v), dict(n_rows=n, n_selected=n_sel, n_present=there, n_colors=nc)


def loaded_case(kc, dev, n, nc):
    for x, (name, mat, v) in enumerate(matrices(n, nc, 7 * n + nc)):
        load(kc, dev, mat, off=x % 2)                                         # (every other one from a 4-byte-only aligned address)
        back = read_rows(kc, dev, n, nc)[0]
        assert (back == mat).all(), name                                      # a load followed by colors_rows returns the loaded matrix
        select = some_select(n, x).tolist() if name in ("sparse", "big", "alternating") else None
        for mc, sel in ((1, None), (2, select)):
            want = closed_form(n, nc, v, mc, sel) if v is not None else None
            got = check_pairs(kc, dev, mat, mc, sel, singles=name == "sparse" and mc == 1, want=want)
            N, T = M.diagonal(mat.tolist(), mc, sel)                          # the hand-computable part, whatever the model says
            assert [got[0][c][c] for c in range(nc)] == N and [got[1][c][c] for c in range(nc)] == T == [got[2][c][c] for c in range(nc)], (name, mc)
            if v is not None and nc <= 8:
                assert M.pairs(mat.tolist(), mc, sel) == tuple(want)          # (the closed form is the model's answer)
        if name in ("sparse", "alternating"):
            check_marks(kc, dev, mat, rules_for(nc)[:5] + rules_for(nc)[6:7])


@pytest.mark.parametrize("nc", N_COLORS)
def test_loaded_matrices_of_every_shape(dev, nc):
    """one dense result trimmed by filter_rows to every row count of N_ROWS in turn; six matrices each.  n_colors <= REG_SWITCH: one thread
    per row; above it: tiles of TILE_ROWS rows in LDS"""
    s = dense_stream(12, 1)
    with count(s, dev, 12, abundance_min=1) as kc:
        for n in N_ROWS:
            trim(kc, dev, n)
            assert code_of(lambda: kc.colors_pairs(1, 0, 0, 0)) == E_ARG
            loaded_case(kc, dev, n, nc)


@pytest.mark.parametrize("reg_max,grid", [(REG_MAX, 0), (0, 0), (REG_MAX, 2), (0, 2), (0, 1)])
def test_both_kernels_at_every_small_width_and_blocks_that_walk(dev, monkeypatch, reg_max, grid):
    """DSKGPU_PAIRS_REG_MAX (read when a context is created) hands every n_colors up to REG_MAX to the one kernel or to the other;
    DSKGPU_PAIRS_GRID = 2 or 1 makes every block walk several stretches of the rows; DSKGPU_PAIRS_NO_SKIP takes the same sums"""
    monkeypatch.setenv("DSKGPU_PAIRS_REG_MAX", str(reg_max))
    if grid:
        monkeypatch.setenv("DSKGPU_PAIRS_GRID", str(grid))
    if grid == 1:
        monkeypatch.setenv("DSKGPU_PAIRS_NO_SKIP", "1")
    s = dense_stream(12, 1)
    with count(s, dev, 12, abundance_min=1) as kc:
        n = 4 * BLOCK + 3 if grid else TILE_ROWS + 1
        trim(kc, dev, n)
        for nc in list(range(1, REG_MAX + 1)) + ([33, 64] if grid else []):
            for name, mat, v in matrices(n, nc, 11 * nc + grid):
                if name in ("sparse", "big", "alternating"):
                    load(kc, dev, mat)
                    sel = some_select(n, nc).tolist()
                    want = closed_form(n, nc, v, 1, sel) if v is not None else None
                    check_pairs(kc, dev, mat, 1, sel, want=want)
                    check_pairs(kc, dev, mat, 2, None, want=closed_form(n, nc, v, 2, None) if v is not None else None)


# ------------------------------------------------------------------ 3. identities on the device alone
def test_identities_with_the_counted_stream_coloured(oracle, golden_dir, dev):
    stream = golden_part(oracle, golden_dir)[1]
    with count(stream, dev, 31, abundance_min=1) as kc:
        n, total = kc.result_device()[2], kc.stats()["n_kmers"]
        kc.colors_begin(1)                                                    # the counted stream as one bank
        add(kc, dev, stream, [len(stream)])
        shared, cross, min_sum, st = device_pairs(kc, dev, 1)
        assert shared == [[n]] and cross == [[total]] and min_sum == [[total]] and st == dict(n_rows=n, n_selected=n, n_present=n, n_colors=1)
        kc.colors_begin(2)                                                    # the same stream as banks 0 and 1
        add(kc, dev, stream, [len(stream)], 0)
        add(kc, dev, stream, [len(stream)], 1)
        shared, cross, min_sum, _ = device_pairs(kc, dev, 2)
        assert shared == [[n, n], [n, n]] and cross == [[total, total], [total, total]] and min_sum == cross
        for nb in (2, 3, 5, 33):                                              # splitting into banks never changes the sum of the diagonal of cross
            kc.colors_begin(nb)
            add(kc, dev, stream, CM.split_at_records(stream, nb))
            shared, cross, min_sum, st = device_pairs(kc, dev, nb)
            assert sum(cross[c][c] for c in range(nb)) == total and st["n_present"] == n
            assert all(min_sum[i][i] == cross[i][i] and shared[i][j] == shared[j][i] and min_sum[i][j] == min_sum[j][i] <= min(cross[i][j], cross[j][i])
                       for i in range(nb) for j in range(nb))


@pytest.mark.parametrize("nb", [3, 9])
def test_save_mark_filter_load_round_trip(oracle, golden_dir, dev, nb):
    """save the matrix, mark by colour, filter the rows, load the saved matrix gathered to the kept rows: the pairs are those of before the
    filter with select = the keep bytes"""
    stream = golden_part(oracle, golden_dir)[1]
    with count(stream, dev, 31, abundance_min=1) as kc:
        kc.colors_begin(nb)
        add(kc, dev, stream, CM.split_at_records(stream, nb))
        saved, _ = kc.colors_rows_tensor()
        keep, st = kc.colors_marks_tensor(min_present=2, min_count=1)
        assert 0 < st["n_kept"] < st["n_rows"] == saved.shape[0] and int(keep.sum().item()) == st["n_kept"]
        before = device_pairs(kc, dev, nb, 1, keep.cpu().numpy().tolist())
        t_before = kc.colors_pairs_tensor(1, keep)
        assert [t.cpu().numpy().tolist() for t in t_before[:3]] == before[:3] and t_before[3] == before[3]
        assert kc.filter_rows_tensor(keep) == st["n_kept"]
        assert code_of(lambda: kc.colors_pairs_tensor()) == E_STATE           # the filter dropped the matrix
        kc.colors_load_tensor(saved[keep.bool()].contiguous())
        after = device_pairs(kc, dev, nb)
        assert after[:3] == before[:3]
        assert after[3] == dict(n_rows=st["n_kept"], n_selected=st["n_kept"], n_present=before[3]["n_present"], n_colors=nb)
        assert (kc.colors_rows_tensor()[0] == saved[keep.bool()]).all()


# ------------------------------------------------------------------ 4. the contract
def test_bad_arguments_and_state(dev):
    s = dense_stream(9, 2)
    out = guarded(dev, 1 << 16)
    torch.cuda.synchronize()
    o = out.data_ptr() + GUARD
    with count(s, dev, 9, abundance_min=1) as kc:
        lib, h = kc._lib, kc._h
        n = kc.result_device()[2]
        mat = torch.ones((n, 3), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        for call in (lambda: kc.colors_pairs(1, o, 0, 0), lambda: kc.colors_marks(o), kc.colors_pairs_tensor, kc.colors_marks_tensor):
            assert code_of(call) == E_STATE                                   # no matrix yet
        for nc in (0, 65, 1 << 31):
            assert code_of(lambda: kc.colors_load(mat.data_ptr(), nc)) == E_ARG
        assert code_of(lambda: kc.colors_load(0, 3)) == E_ARG                 # null d_counts while there are rows
        assert code_of(lambda: kc.colors_pairs(1, o, 0, 0)) == E_STATE        # a refused load keeps nothing
        kc.colors_load_tensor(mat)
        bad = [lambda: kc.colors_pairs(1, 0, 0, 0),                           # all three outputs null
               lambda: kc.colors_pairs(0, o, 0, 0),                           # min_count == 0
               lambda: kc.colors_marks(o, min_count=0),
               lambda: kc.colors_marks(o, need_all=8), lambda: kc.colors_marks(o, need_none=1 << 63),      # bits at or above n_colors
               lambda: kc.colors_marks(0)]                                    # null d_keep while there are rows
        for i, call in enumerate(bad):
            assert code_of(call) == E_ARG, i
        from dsk_amd.engine import _ColorRule
        assert lib.dskgpu_colors_marks(h, None, C.c_void_p(o), None) == E_ARG                                # a null rule
        assert lib.dskgpu_colors_marks(h, C.byref(_ColorRule(min_count=1, flags=2)), C.c_void_p(o), None) == E_ARG      # unknown flags
        assert lib.dskgpu_colors_pairs(None, 1, None, C.c_void_p(o), None, None, None) == E_ARG and lib.dskgpu_colors_load(None, C.c_void_p(o), 1) == E_ARG
        assert lib.dskgpu_colors_marks(None, C.byref(_ColorRule(min_count=1)), C.c_void_p(o), None) == E_ARG
        assert (out.cpu().numpy() == 0xEE).all()                              # no refused call wrote anything
        assert lib.dskgpu_colors_pairs(h, 1, None, C.c_void_p(o), None, None, None) == 0                     # stats may be NULL
        assert lib.dskgpu_colors_marks(h, C.byref(_ColorRule(min_count=1)), C.c_void_p(o + 4096), None) == 0
        torch.cuda.synchronize()
        assert inside(out, 1 << 16)[:72].view(np.uint64).tolist() == [n] * 9 and (inside(out, 1 << 16)[4096: 4096 + n] == 1).all()
        kc.colors_load_tensor(mat[:, :2].contiguous())                       # a second load replaces the matrix
        assert device_pairs(kc, dev, 2)[0] == [[n, n], [n, n]]
        kc.colors_begin(4)                                                    # and so does a begin
        assert device_pairs(kc, dev, 4)[3] == dict(n_rows=n, n_selected=n, n_present=0, n_colors=4)
        kc.colors_load_tensor(mat)
        kc.count()                                                           # a new count drops the matrix
        for call in (lambda: kc.colors_pairs(1, o, 0, 0), lambda: kc.colors_marks(o)):
            assert code_of(call) == E_STATE


def test_before_any_count_is_a_state_error(dev):
    from dsk_amd import KmerCounter
    buf = torch.zeros(1024, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p = buf.data_ptr()
    with KmerCounter(kmer_size=31) as kc:
        for call in (lambda: kc.colors_load(p, 2), lambda: kc.colors_pairs(1, p, 0, 0), lambda: kc.colors_marks(p)):
            assert code_of(call) == E_STATE


def test_a_result_without_rows(oracle, golden_dir, dev):
    stream = golden_part(oracle, golden_dir)[1]
    with count(stream, dev, 31, abundance_min=10 ** 6) as kc:
        assert kc.stats()["n_solid"] == 0
        assert code_of(lambda: kc.colors_pairs(1, 1, 0, 0)) == E_STATE
        kc.colors_load(0, 3)                                                  # zero rows: a null d_counts is taken
        shared, cross, min_sum, st = device_pairs(kc, dev, 3, singles=True)
        zero = [[0] * 3 for _ in range(3)]
        assert shared == zero and cross == zero and min_sum == zero           # the outputs are zeroed
        assert st == dict(n_rows=0, n_selected=0, n_present=0, n_colors=0)
        out = guarded(dev, 64)
        torch.cuda.synchronize()
        assert kc.colors_marks(out.data_ptr() + GUARD) == dict(n_rows=0, n_kept=0) and kc.colors_marks(0) == dict(n_rows=0, n_kept=0)
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == 0xEE).all()
        t = kc.colors_pairs_tensor()
        assert all(x.shape == (3, 3) and not x.any() for x in t[:3]) and kc.colors_marks_tensor()[0].shape == (0,)


def test_the_context_is_left_alone(oracle, golden_dir, dev):
    """rows, stats and histogram, a kept compaction and the matrix, before and after pairs and marks"""
    stream = golden_part(oracle, golden_dir)[1]
    with count(stream, dev, 31, abundance_min=2) as kc:
        k1, a1 = kc.rows(); h1 = kc.histogram(); s1 = kc.stats()
        u1 = kc.unitigs()
        ur1 = [x.clone() for x in kc.unitigs_rows_tensor()]
        kc.colors_begin(5)
        kc.colors_add_tensor(torch.from_numpy(stream).to(dev), CM.split_at_records(stream, 5))
        m1 = kc.colors_rows_tensor()[0].clone()
        sums1 = [x.clone() for x in kc.colors_unitigs_tensor()]
        kc.colors_pairs_tensor(); kc.colors_pairs_tensor(2, kc.colors_marks_tensor(min_present=2)[0]); kc.colors_marks_tensor(need_all=3, invert=True)
        k2, a2 = kc.rows()
        assert (k1 == k2).all() and (a1 == a2).all() and (kc.histogram() == h1).all() and kc.stats() == s1
        assert kc.unitigs() == u1 and all((x == y).all() for x, y in zip(ur1, kc.unitigs_rows_tensor()))
        assert (kc.colors_rows_tensor()[0] == m1).all() and all((x == y).all() for x, y in zip(sums1, kc.colors_unitigs_tensor()))
        kc.colors_load_tensor(m1)                                            # a load of the matrix itself changes nothing else either
        assert kc.unitigs() == u1 and all((x == y).all() for x, y in zip(sums1, kc.colors_unitigs_tensor())) and kc.stats() == s1


def test_a_rank_of_a_group_adds_up_to_one_context(oracle, golden_dir, dev):
    """world_size = 2: the ranks partition the k-mers, so their pair matrices add up to those of one context"""
    from dsk_amd import KmerGroup
    whole = stream_of("golden", oracle, golden_dir)
    part = golden_part(oracle, golden_dir)[1]
    recs = bytes(whole).split(b"\n")[:400]
    ends = CM.split_at_records(part, 3)
    total = None
    with KmerGroup([0, 0], kmer_size=31, abundance_min=2) as g:
        for r in range(2):
            g.rank(r).push_reads(b"\n".join(recs[r::2]) + b"\n")
        g.count()
        for r in range(2):
            kc = g.rank(r)
            n = kc.result_device()[2]
            kc.colors_begin(3)
            add(kc, dev, part, ends)
            mat = read_rows(kc, dev, n, 3)[0]
            got = check_pairs(kc, dev, mat, 1)                                # the rank's rows against the model
            check_marks(kc, dev, mat, rules_for(3)[:3])
            arr = [np.array(m, dtype=object) for m in got[:3]] + [got[3]["n_present"]]
            total = arr if total is None else [x + y for x, y in zip(total, arr)]
    with count(as_np(b"\n".join(recs) + b"\n"), dev, 31, abundance_min=2) as one:
        one.colors_begin(3)
        add(one, dev, part, ends)
        shared, cross, min_sum, st = device_pairs(one, dev, 3)
        assert [m.tolist() for m in total[:3]] == [shared, cross, min_sum] and total[3] == st["n_present"] > 0


def test_stage_times_name_the_stages(oracle, golden_dir, dev):
    stream = golden_part(oracle, golden_dir)[1]
    with count(stream, dev, 31, abundance_min=2, timing=True) as kc:
        assert not any(n in dict(kc.stage_times()) for n in ("color pairs", "color marks", "color load"))
        kc.colors_begin(2)
        kc.colors_add_tensor(torch.from_numpy(stream).to(dev), CM.split_at_records(stream, 2))
        saved = kc.colors_rows_tensor()[0]
        kc.colors_pairs_tensor()
        assert dict(kc.stage_times())["color pairs"] > 0 and "color marks" not in dict(kc.stage_times())
        kc.colors_marks_tensor(min_present=1)
        assert dict(kc.stage_times())["color marks"] > 0 and "color load" not in dict(kc.stage_times())
        kc.colors_load_tensor(saved)
        assert dict(kc.stage_times())["color load"] > 0
