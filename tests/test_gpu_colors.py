"""Sample colours for rows, unitigs and variants on the device (include/dskgpu.h: dskgpu_colors_begin / _colors_add / _colors_rows /
_colors_unitigs; csrc/colors.h).

All comparisons are exact integers.  Part 1 compares the device -- matrix, masks, unitig sums / all / any, variant colours and stats -- with
the restatement of tests/color_model.py (which the CPU suite checks first) built from kc.rows() and the device's own unitig[r], and with the
matrices written out in tests/test_colors_restatement.py.  Part 2 is identities on the device alone, with the counted stream coloured.
Part 3 is geometry: the smallest shapes at which the bank walk, the frame, the run merge, the atomics and the copy kernel can go wrong.
Part 4 is the contract.  Every output has guard bytes around it and every input is checked unchanged.

Every test here fails before the feature: KmerCounter has no colors_begin and the library no dskgpu_colors_begin.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import color_model as M      # noqa: E402
from tests.dense_streams import DENSE_CASES, dense_stream      # noqa: E402
from tests.test_colors_restatement import HAND      # noqa: E402
from tests.test_correct_restatement import KS, handmade_correct      # noqa: E402
from tests.test_gpu_read_summaries import GUARD, as_np, guarded, inside, put      # noqa: E402
from tests.test_gpu_unitigs import code_of, count, row_values, stream_of      # noqa: E402

E_ARG, E_STATE = -1, -4
assert all(k in KS for k in (31, 32, 33, 64, 65))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


# ------------------------------------------------------------------ one call each, guard bytes round every output
def add(kc, dev, stream, ends, first_color=0, off=0):
    """one dskgpu_colors_add of the stream at offset `off` of an aligned allocation -> the stats; the input is checked unchanged"""
    n = len(stream)
    src = put(dev, stream, off)
    torch.cuda.synchronize()
    st = kc.colors_add(src.data_ptr() + off if n else 0, n, ends, first_color)
    back = src.cpu().numpy()
    assert (back[off: off + n] == stream).all() and (back[:off] == 10).all() and (back[off + n:] == 10).all(), "the input is left as it was"
    return st


def read_rows(kc, dev, n, nc, min_count=1, off=0):
    """-> (uint32[n, nc] the matrix, uint64[n] the masks); off: the counts 4 * off bytes and the masks 8 * off bytes off a 16-byte boundary"""
    cb, mb = guarded(dev, 4 * n * nc, 4 * off), guarded(dev, 8 * n, 8 * off)
    torch.cuda.synchronize()
    kc.colors_rows(min_count, cb.data_ptr() + GUARD + 4 * off, mb.data_ptr() + GUARD + 8 * off)
    torch.cuda.synchronize()
    counts, mask = inside(cb, 4 * n * nc, 4 * off).view(np.uint32).reshape(n, nc), inside(mb, 8 * n, 8 * off).view(np.uint64)
    only = guarded(dev, 8 * n)                                                # the masks alone, and the counts alone
    torch.cuda.synchronize()
    kc.colors_rows(min_count, 0, only.data_ptr() + GUARD)
    torch.cuda.synchronize()
    assert (inside(only, 8 * n).view(np.uint64) == mask).all()
    return counts, mask


def read_unitigs(kc, dev, nu, nc, min_count=1):
    """-> (uint64[nu, nc] sum, uint64[nu] all, uint64[nu] any)"""
    sb, ab, yb = guarded(dev, 8 * nu * nc), guarded(dev, 8 * nu), guarded(dev, 8 * nu)
    torch.cuda.synchronize()
    kc.colors_unitigs(min_count, sb.data_ptr() + GUARD, ab.data_ptr() + GUARD, yb.data_ptr() + GUARD)
    torch.cuda.synchronize()
    return inside(sb, 8 * nu * nc).view(np.uint64).reshape(nu, nc), inside(ab, 8 * nu).view(np.uint64), inside(yb, 8 * nu).view(np.uint64)


def u64s(values):
    return np.array([int(v) for v in values], dtype=np.uint64)


def check_against(kc, dev, model, unitig=None, nu=0, alleles=None, min_counts=(1, 2)):
    """the kept matrix and everything derived from it against the model"""
    n, nc = model.n_rows, model.n_colors
    want = np.array(model.matrix(), dtype=np.uint32).reshape(n, nc)
    for mc in min_counts:
        counts, mask = read_rows(kc, dev, n, nc, mc)
        bad = np.argwhere(counts != want)
        assert len(bad) == 0, (len(bad), bad[:5], counts[counts != want][:5], want[counts != want][:5])
        assert (mask == u64s(model.mask(mc))).all(), mc
        if unitig is not None:
            total, all_, any_ = read_unitigs(kc, dev, nu, nc, mc)
            w_total, w_all, w_any = model.unitigs(unitig, nu, mc)
            assert (total == np.array(w_total, dtype=np.uint64).reshape(nu, nc)).all(), mc
            assert (all_ == u64s(w_all)).all() and (any_ == u64s(w_any)).all(), mc
    t_counts, t_mask = kc.colors_rows_tensor(min_counts[0])
    assert t_counts.shape == (n, nc) and (t_counts.cpu().numpy().view(np.uint32) == want).all()
    assert (t_mask.cpu().numpy().view(np.uint64) == u64s(model.mask(min_counts[0]))).all()
    if unitig is not None:
        w_total = model.unitigs(unitig, nu, 1)[0]
        t_total, t_all, t_any = kc.colors_unitigs_tensor(1)
        assert t_total.shape == (nu, nc) and (t_total.cpu().numpy() == np.array(w_total, dtype=np.int64).reshape(nu, nc)).all()
        if alleles is not None:
            v = kc.variants_colors_tensor().cpu().numpy()
            assert v.shape == (len(alleles), 2, nc)
            assert (v == np.array(M.variant_colours(w_total, alleles), dtype=np.int64).reshape(len(alleles), 2, nc)).all()


def graph_of(kc):
    """-> (unitig[r] of every row, n_unitigs, the (A, B) of the kept variants), all from the device"""
    nu = kc.unitigs()["n_unitigs"]
    unitig = kc.unitigs_rows_tensor()[0].cpu().numpy()
    kc.variants()
    return unitig, nu, kc.variants_tensor().cpu().numpy()[:, :2]


# ------------------------------------------------------------------ 1. the restatement, every key width, both row orders
_parts, _wins = {}, {}


def golden_part(oracle, golden_dir):
    if "g" not in _parts:
        whole = stream_of("golden", oracle, golden_dir)
        ends = np.flatnonzero(whole == 10)
        _parts["g"] = (whole, whole[: int(ends[599]) + 1].copy(), whole[int(ends[299]) + 1: int(ends[899]) + 1].copy())
    return _parts["g"]


def streams(kind, k, oracle, golden_dir):
    """-> (the stream to count, the stream to colour)"""
    if kind == "golden":                                                   # records 300 .. 899 counted, records 0 .. 599 coloured: half of them overlap
        return golden_part(oracle, golden_dir)[2], golden_part(oracle, golden_dir)[1]
    if kind == "hand":
        counted, s, _ = handmade_correct(k)
        return counted, np.concatenate([s, as_np("\n"), counted])          # (every separator, lower case, N; then reads that are rows)
    s = dense_stream(k, int(kind.split(":")[1]))
    return s, s


def windows_of(kind, k, stream):
    if (kind, k) not in _wins:
        _wins[(kind, k)] = M.windows(stream, k)
    return _wins[(kind, k)]


def parity_case(dev, kind, k, oracle, golden_dir):
    counted, stream = streams(kind, k, oracle, golden_dir)
    wins = windows_of(kind, k, stream)
    seen = set()
    for order in (False, True):
        for amin in (1, 3):
            with count(counted, dev, k, abundance_min=amin, partition_order=order) as kc:
                rows = M.rows_of(row_values(kc.rows()[0]), k)
                unitig, nu, alleles = graph_of(kc)
                for nb in (1, 2, 3, 5):
                    ends = M.split_at_records(stream, nb)
                    first = 1 if nb == 2 else 0                               # (two banks: colours 1 and 2 of 3)
                    model = M.Colours(rows, nb + first, k)
                    want_st = model.add(stream, ends, first, wins)
                    kc.colors_begin(nb + first)
                    st = add(kc, dev, stream, ends, first)
                    print("colours", kind, k, order, amin, nb, st, "unitigs", nu, "variants", len(alleles))
                    assert st == want_st
                    check_against(kc, dev, model, unitig, nu, alleles)
                    seen.add((st["n_placed"] > 0, len(alleles) > 0))
    return seen


@pytest.mark.parametrize("kind,k", [("golden", k) for k in KS] + [("hand", k) for k in KS] + [("dense:%d" % s, k) for k, s in DENSE_CASES])
def test_device_equals_the_model(oracle, golden_dir, dev, kind, k):
    """matrix, masks (min_count 1 and 2), unitig sum / all / any, variant colours and stats; 1, 2, 3 and 5 banks; both row orders;
    abundance_min 1 and 3"""
    seen = parity_case(dev, kind, k, oracle, golden_dir)
    assert any(placed for placed, _ in seen) or (kind == "golden" and k > 100)      # (the golden reads have 100 letters)
    if kind == "golden" and k <= 33:
        assert (True, True) in seen                                          # (the golden reads' errors make bubbles at abundance_min 1)


@pytest.mark.parametrize("name", sorted(HAND))
def test_the_matrices_written_out_by_hand(dev, name):
    """a count crafted to the hand-made rows (one line per row) -> the matrix written out in the restatement's test, row by row"""
    h = HAND[name]
    k, nc = h["k"], h["n_colors"]
    with count(as_np("".join(s + "\n" for s in h["rows"])), dev, k, abundance_min=1) as kc:
        rows = M.rows_of(row_values(kc.rows()[0]), k)
        assert sorted(rows) == sorted(h["rows"])
        perm = [h["rows"].index(s) for s in rows]                             # device row -> hand row
        kc.colors_begin(nc)
        assert add(kc, dev, h["stream"], h["ends"], h["first_color"]) == h["stats"]
        for mc, masks in h["masks"].items():
            counts, mask = read_rows(kc, dev, len(rows), nc, mc)
            assert counts.tolist() == [h["matrix"][i] for i in perm]
            assert mask.tolist() == [masks[i] for i in perm]
        model = M.Colours(rows, nc, k)
        model.add(h["stream"], h["ends"], h["first_color"])
        unitig, nu, alleles = graph_of(kc)
        check_against(kc, dev, model, unitig, nu, alleles)


# ------------------------------------------------------------------ 2. identities on the device alone
@pytest.mark.parametrize("k,amin", [(31, 1), (31, 2), (65, 2), (12, 1)])
def test_identities_with_the_counted_stream_coloured(oracle, golden_dir, dev, k, amin):
    from dsk_amd import KmerCounter
    stream = dense_stream(12, 1) if k == 12 else golden_part(oracle, golden_dir)[1]
    ends = M.split_at_records(stream, 3)
    assert len(set(ends)) == 3
    t = torch.from_numpy(stream).to(dev)
    with count(stream, dev, k, abundance_min=amin) as kc:
        kk, ab = kc.rows()
        n = len(ab)
        kc.colors_begin(3)
        st = add(kc, dev, stream, ends)
        C1, _ = read_rows(kc, dev, n, 3)
        C1 = C1.astype(np.int64)
        assert (C1.sum(1) == ab.astype(np.int64)).all()                                    # (a)
        keys = torch.from_numpy(kk.view(np.int64)).to(dev)
        for c in range(3):                                                                  # (b) a second context that counted bank c alone
            lo = 0 if c == 0 else ends[c - 1]
            with KmerCounter(kmer_size=k, abundance_min=1) as other:
                bank = t[lo: ends[c]].clone()
                torch.cuda.synchronize()
                other.set_reads_device(bank.data_ptr(), bank.numel())
                other.count()
                got = other.query_kmers_tensor(keys if kc.words > 1 else keys.reshape(-1)).cpu().numpy().view(np.uint32)
            assert (C1[:, c] == got).all(), c
        kmers = torch.zeros((len(stream), kc.words), dtype=torch.int64, device=dev)        # (c)
        valid = torch.zeros(len(stream), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        kc.k_enumerate(t.data_ptr(), len(stream), kmers.data_ptr(), valid.data_ptr())
        torch.cuda.synchronize()
        assert st["n_placed"] == C1.sum() and st["n_valid"] == int((valid != 0).sum().item()) and st["n_rows"] == n and st["n_colors"] == 3
        nu = kc.unitigs()["n_unitigs"]                                                      # (d)
        total, all_, any_ = read_unitigs(kc, dev, nu, 3)
        ab_sum = kc.unitigs_table_tensor()[1].cpu().numpy()
        assert (total.astype(np.int64).sum(1) == ab_sum).all()
        assert ((all_ & ~any_) == 0).all() and (any_ != 0).all()
        kc.colors_begin(3)                                                                  # (e) three calls with one bank each
        for c in range(3):
            lo = 0 if c == 0 else ends[c - 1]
            add(kc, dev, stream[lo: ends[c]], [ends[c] - lo], c)
        assert (read_rows(kc, dev, n, 3)[0] == C1).all()
        add(kc, dev, stream, ends)                                                          # (f) the same stream once more: every cell doubles
        assert (read_rows(kc, dev, n, 3)[0] == 2 * C1).all()


# ------------------------------------------------------------------ 3. geometry
_geo = {}


def boundary_stream():
    """about 200 bytes, two records and an N: short enough to move a boundary through every offset, long enough for windows of 65"""
    if "s" not in _geo:
        rng = np.random.default_rng(5)
        s = "".join("ACGT"[i] for i in rng.integers(0, 4, 203))
        _geo["s"] = as_np(s[:150] + "\n" + s[150:170] + "N" + s[170:] + "\n")
    return _geo["s"]


@pytest.mark.parametrize("k", [5, 33, 65])
def test_a_bank_boundary_at_every_residue(dev, k):
    """two banks, the boundary at 64 consecutive offsets: every residue modulo 32 and so modulo N = 16 / 8 / 4; the windows that cross the
    boundary belong to the bank they end in"""
    s = boundary_stream()
    wins = M.windows(s, k)
    with count(s, dev, k, abundance_min=1) as kc:
        rows = M.rows_of(row_values(kc.rows()[0]), k)
        src = put(dev, s)
        torch.cuda.synchronize()
        for b in range(40, 104):
            model = M.Colours(rows, 2, k)
            want = model.add(s, [b, len(s)], 0, wins)
            kc.colors_begin(2)
            assert kc.colors_add(src.data_ptr(), len(s), [b, len(s)]) == want, b
            counts, _ = read_rows(kc, dev, len(rows), 2)
            assert (counts == np.array(model.matrix(), dtype=np.uint32)).all(), b
            assert counts[:, 0].sum() == sum(1 for p, _ in wins if p < b)
        assert (src.cpu().numpy()[: len(s)] == s).all()


@pytest.mark.parametrize("off", [1, 3, 15])
def test_streams_at_odd_addresses(dev, off):
    s = boundary_stream()
    with count(s, dev, 5, abundance_min=1) as kc:
        rows = M.rows_of(row_values(kc.rows()[0]), 5)
        model = M.Colours(rows, 3, 5)
        ends = [77, 77, len(s)]                                               # (an empty bank in the middle)
        want = model.add(s, ends)
        kc.colors_begin(3)
        assert add(kc, dev, s, ends, 0, off) == want
        check_against(kc, dev, model)


def test_small_shapes(dev):
    """a stream shorter than k, one bank, two empty banks in a row, ends that stop before nbytes, colour 63 of 64"""
    s = boundary_stream()
    k = 5
    with count(s, dev, k, abundance_min=1) as kc:
        rows = M.rows_of(row_values(kc.rows()[0]), k)
        n = len(rows)
        unitig, nu, alleles = graph_of(kc)
        kc.colors_begin(1)
        assert add(kc, dev, as_np("ACGT"), [4]) == dict(n_valid=0, n_placed=0, n_rows=n, n_colors=1)      # shorter than k
        assert not read_rows(kc, dev, n, 1)[0].any()
        for nc, ends, first in ((1, [len(s)], 0), (4, [50, 50, 50, 120], 0), (2, [60, 100], 0), (64, [len(s)], 63), (64, [10, 90], 62)):
            model = M.Colours(rows, nc, k)
            want = model.add(s, ends, first)
            kc.colors_begin(nc)
            assert add(kc, dev, s, ends, first) == want, (nc, ends)
            assert want["n_valid"] < len(M.windows(s, k)) or ends[-1] == len(s)
            check_against(kc, dev, model, unitig, nu, alleles)
        counts, mask = read_rows(kc, dev, n, 64)
        assert not counts[:, :62].any() and counts[:, 63].any() and (mask >> np.uint64(63)).any()


@pytest.mark.parametrize("nc", [1, 3, 4, 5, 8])
def test_the_copy_at_every_vector_width(dev, nc):
    """n_colors 1, 3, 4, 5 and 8, the counts 16-byte aligned and 4 bytes off: both forms of the copy kernel where n_colors % 4 == 0"""
    s = boundary_stream()
    k = 5
    with count(s, dev, k, abundance_min=1) as kc:
        rows = M.rows_of(row_values(kc.rows()[0]), k)
        ends = [33, 97, 131, 151, 180, 190, 200][: nc - 1] + [len(s)]
        model = M.Colours(rows, nc, k)
        want = model.add(s, ends)
        kc.colors_begin(nc)
        assert add(kc, dev, s, ends) == want
        for off in (0, 1):
            for mc in (1, 2):
                counts, mask = read_rows(kc, dev, len(rows), nc, mc, off)
                assert (counts == np.array(model.matrix(), dtype=np.uint32)).all() and (mask == u64s(model.mask(mc))).all(), (off, mc)


@pytest.mark.parametrize("k", [21, 32])
def test_one_row_takes_every_add(dev, k):
    """5000 A and (AC) x 2500: one row, or two, take every add of many waves -- the run merge and the atomics -- whole and with a boundary in
    the middle of either read"""
    s = as_np("A" * 5000 + "\n" + "AC" * 2500 + "\n")
    with count(s, dev, k, abundance_min=1) as kc:
        kk, ab = kc.rows()
        rows = M.rows_of(row_values(kk), k)
        assert sorted(ab.tolist()) == [2500 - k // 2, 2500 - (k - 1) // 2, 5000 - k + 1] and len(rows) == 3
        wins = M.windows(s, k)
        for ends in ([len(s)], [2503, 7777, len(s)], [5001, len(s)]):
            model = M.Colours(rows, len(ends), k)
            want = model.add(s, ends, 0, wins)
            kc.colors_begin(len(ends))
            assert add(kc, dev, s, ends) == want
            check_against(kc, dev, model)
            assert (read_rows(kc, dev, 3, len(ends))[0].astype(np.int64).sum(1) == ab).all()


# ------------------------------------------------------------------ 4. the contract
def test_bad_arguments(dev):
    s = boundary_stream()
    src = put(dev, s)
    out = guarded(dev, 1 << 16)
    torch.cuda.synchronize()
    p, o, n = src.data_ptr(), out.data_ptr() + GUARD, len(s)
    with count(s, dev, 5, abundance_min=1) as kc:
        lib, h = kc._lib, kc._h
        for nc in (0, 65, 1 << 31):
            assert code_of(lambda: kc.colors_begin(nc)) == E_ARG
        for call in (lambda: kc.colors_add(p, n, [n]), lambda: kc.colors_rows(1, o, 0), lambda: kc.colors_unitigs(1, o, 0, 0)):
            assert code_of(call) == E_STATE                                   # no begin yet
        kc.colors_begin(3)
        bad = [lambda: kc.colors_add(p, n, [10, 20, 30, n]),                  # first_color + n_banks > n_colors
               lambda: kc.colors_add(p, n, [10, n], 2),
               lambda: kc.colors_add(p, n, [n], 3),
               lambda: kc.colors_add(p, n, []),                               # no bank for a stream
               lambda: kc.colors_add(p, n, [20, 10, n]),                      # decreasing ends
               lambda: kc.colors_add(p, n, [10, n + 1]),                      # an end above nbytes
               lambda: kc.colors_add(0, n, [n]),                              # null d_bytes
               lambda: kc.colors_add(p, n, list(range(65))),                  # more banks than a mask has bits
               lambda: kc.colors_rows(1, 0, 0), lambda: kc.colors_unitigs(1, 0, 0, 0),
               lambda: kc.colors_rows(0, o, 0), lambda: kc.colors_unitigs(0, o, 0, 0)]
        for i, call in enumerate(bad):
            assert code_of(call) == E_ARG, i
        assert lib.dskgpu_colors_add(h, C.c_void_p(p), n, None, 1, 0, None) == E_ARG         # null end_offsets
        assert lib.dskgpu_colors_begin(None, 1) == E_ARG and lib.dskgpu_colors_rows(None, 1, C.c_void_p(o), None) == E_ARG
        assert kc.colors_add(0, 0, []) == dict(n_valid=0, n_placed=0, n_rows=0, n_colors=0)                      # nbytes == 0: all-zero stats
        assert kc.colors_add(p, 0, [0, 0]) == kc.colors_add(0, 0, [])
        ends = (C.c_uint64 * 1)(n)
        assert lib.dskgpu_colors_add(h, C.c_void_p(p), n, ends, 1, 0, None) == 0             # stats may be NULL
        assert not read_rows(kc, dev, len(kc.rows()[1]), 3)[0][:, 1:].any()                  # nothing of all that reached the matrix but the last call
        assert (out.cpu().numpy() == 0xEE).all()                                             # and no refused call wrote anything


def test_before_any_count_is_a_state_error(dev):
    from dsk_amd import KmerCounter
    buf = torch.zeros(1024, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p = buf.data_ptr()
    with KmerCounter(kmer_size=31) as kc:
        for call in (lambda: kc.colors_begin(2), lambda: kc.colors_add(p, 64, [64]), lambda: kc.colors_rows(1, p, 0), lambda: kc.colors_unitigs(1, p, 0, 0),
                     kc.colors_rows_tensor, kc.colors_unitigs_tensor):
            assert code_of(call) == E_STATE


def test_a_result_without_rows(oracle, golden_dir, dev):
    whole, part = golden_part(oracle, golden_dir)[:2]
    with count(whole, dev, 31, abundance_min=10 ** 6) as kc:
        assert kc.stats()["n_solid"] == 0
        kc.colors_begin(2)
        assert add(kc, dev, part, M.split_at_records(part, 2)) == dict(n_valid=600 * 70, n_placed=0, n_rows=0, n_colors=2)
        out = guarded(dev, 64)
        torch.cuda.synchronize()
        kc.colors_rows(1, out.data_ptr() + GUARD, out.data_ptr() + GUARD)
        kc.colors_unitigs(1, out.data_ptr() + GUARD, out.data_ptr() + GUARD, out.data_ptr() + GUARD)
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == 0xEE).all()                             # nothing is written by the copy calls
        assert kc.colors_rows_tensor()[0].shape == (0, 2) and kc.colors_unitigs_tensor()[0].shape == (0, 2)


def test_what_drops_the_matrix_and_what_a_second_begin_does(oracle, golden_dir, dev):
    """a new count, filter_rows and simplify_all each drop it (E_STATE until a new begin); a second begin zeroes it"""
    whole, part = golden_part(oracle, golden_dir)[:2]
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    src = put(dev, part)
    torch.cuda.synchronize()
    p, o, n = src.data_ptr(), buf.data_ptr(), len(part)

    def gone(kc):
        for call in (lambda: kc.colors_add(p, n, [n]), lambda: kc.colors_rows(1, o, 0), lambda: kc.colors_unitigs(1, 0, o, 0), kc.colors_rows_tensor):
            assert code_of(call) == E_STATE

    with count(part, dev, 31, abundance_min=1) as kc:
        n_rows = len(kc.rows()[1])
        kc.colors_begin(2)
        st = kc.colors_add(p, n, [n])
        assert st["n_placed"] == st["n_valid"] > 0
        kc.colors_begin(2)                                                    # a second begin: all zero again
        assert not read_rows(kc, dev, n_rows, 2)[0].any()
        kc.colors_add(p, n, [n], 1)
        C1, _ = read_rows(kc, dev, n_rows, 2)
        assert not C1[:, 0].any() and C1[:, 1].sum() == st["n_placed"]
        kc.count()                                                           # a new count
        gone(kc)
        kc.colors_begin(2)
        kc.colors_add(p, n, [n], 1)
        assert (read_rows(kc, dev, n_rows, 2)[0] == C1).all()
        keep = torch.from_numpy((kc.rows()[1] >= 2).astype(np.uint8)).to(dev)
        left = kc.filter_rows_tensor(keep)                                   # filter_rows
        assert 0 < left < n_rows
        gone(kc)
        kc.colors_begin(1)
        st2 = kc.colors_add(p, n, [n])
        assert st2["n_rows"] == left and st2["n_valid"] == st["n_valid"] and 0 < st2["n_placed"] < st["n_placed"]
        model = M.Colours(M.rows_of(row_values(kc.rows()[0]), 31), 1, 31)     # the next matrix is that of the rows left
        model.add(part, [n])
        check_against(kc, dev, model, min_counts=(1,))
    with count(part, dev, 31, abundance_min=1) as kc:
        n_rows = len(kc.rows()[1])
        kc.colors_begin(1)
        kc.colors_add(p, n, [n])
        kc.simplify_all()                                                    # the simplifications filter rows
        assert len(kc.rows()[1]) < n_rows
        gone(kc)
    assert (src.cpu().numpy()[:n] == part).all()


def test_the_context_is_left_alone(oracle, golden_dir, dev):
    """rows, stats and histogram before and after; a kept encoding and a kept threading stay as they are"""
    from dsk_amd import KmerCounter
    whole, part = golden_part(oracle, golden_dir)[:2]
    reads = torch.from_numpy(whole).to(dev)
    other = torch.from_numpy(part).to(dev)
    buf = reads.clone()
    torch.cuda.synchronize()
    with KmerCounter(kmer_size=31, abundance_min=2) as kc:
        kc.set_reads_device(buf.data_ptr(), buf.numel())
        kc.encode_reads()
        buf.zero_(); torch.cuda.synchronize()                                # the bytes are gone: the 2-bit form is the only copy of the reads
        kc.count()
        k1, a1 = kc.rows(); h1 = kc.histogram(); s1 = kc.stats()
        ts = kc.thread_reads_tensor(other)
        w1 = [x.clone() for x in kc.thread_walks_tensor()]
        kc.colors_begin(4)
        st = kc.colors_add_tensor(other, M.split_at_records(part, 4))
        assert st["n_placed"] > 0
        kc.colors_rows_tensor(); kc.colors_unitigs_tensor(2)
        k2, a2 = kc.rows()
        assert (k1 == k2).all() and (a1 == a2).all() and (kc.histogram() == h1).all() and kc.stats() == s1
        w2 = kc.thread_walks_tensor()                                        # the kept threading
        assert all((x == y).all() for x, y in zip(w1, w2)) and ts["n_walks"] > 0
        kc.count()                                                           # from the kept encoding: identical rows
        k3, a3 = kc.rows()
        assert (k1 == k3).all() and (a1 == a3).all() and kc.stats() == s1
    assert (other.cpu().numpy() == part).all()


def test_a_rank_of_a_group_serves_rows_and_refuses_unitigs(oracle, golden_dir, dev):
    """world_size > 1: begin / add / rows work on the rank's rows; dskgpu_colors_unitigs is DSKGPU_E_STATE and the text names world_size"""
    from dsk_amd import KmerGroup
    whole, part = golden_part(oracle, golden_dir)[:2]
    recs = bytes(whole).split(b"\n")
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with KmerGroup([0, 0], kmer_size=31, abundance_min=2) as g:
        for r in range(2):
            g.rank(r).push_reads(b"\n".join(recs[r::2]) + b"\n")
        g.count()
        placed = 0
        for r in range(2):
            kc = g.rank(r)
            rows = M.rows_of(row_values(kc.rows()[0]), 31)
            model = M.Colours(rows, 2, 31)
            ends = M.split_at_records(part, 2)
            want = model.add(part, ends, 0, windows_of("golden", 31, part))
            kc.colors_begin(2)
            assert add(kc, dev, part, ends) == want
            check_against(kc, dev, model, min_counts=(1,))
            placed += want["n_placed"]
            assert code_of(lambda: kc.colors_unitigs(1, buf.data_ptr(), 0, 0)) == E_STATE
            assert "world_size" in kc._lib.dskgpu_last_error(kc._h).decode()
        with count(whole, dev, 31, abundance_min=2) as one:                   # the ranks' rows are the rows of one context, shared out
            one.colors_begin(2)
            assert add(one, dev, part, ends)["n_placed"] == placed


def test_stage_times_name_the_stages(oracle, golden_dir, dev):
    whole, part = golden_part(oracle, golden_dir)[:2]
    with count(whole, dev, 31, abundance_min=2, timing=True) as kc:
        before = dict(kc.stage_times())
        assert not any(n in before for n in ("colors", "color unitigs", "query index"))
        kc.colors_begin(2)
        add(kc, dev, part, M.split_at_records(part, 2))
        after = dict(kc.stage_times())
        assert after["colors"] > 0 and after["query index"] > 0 and "color unitigs" not in after
        kc.colors_unitigs_tensor()
        assert dict(kc.stage_times())["color unitigs"] > 0
