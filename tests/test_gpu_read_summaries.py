"""Per-read abundance summaries and read selection on the device (include/dskgpu.h: dskgpu_read_summaries / _read_summaries_table /
_read_marks / dskgpu_select_reads; csrc/readsum.h).

All comparisons are exact.  Part 1 compares the device -- table, stats and marks -- with the restatement of tests/read_summary_model.py
(which the CPU suite checks first) built from kc.rows(), and with the tables written out in tests/test_read_summary_restatement.py.
Part 2 is a second path to the same table: numpy reductions over dskgpu_query_reads and dskgpu_k_enumerate.  Part 3 is geometry: the
smallest shapes at which the frame, the valid bits, the record ranking, the two summary paths and their boundary can go wrong.  Part 4 is
the median's corner cases, part 5 the selection, part 6 the contract.

Every test here fails before the feature: KmerCounter has no read_summaries and the library no dskgpu_read_summaries.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import read_summary_model as M      # noqa: E402
from tests.test_correct_restatement import KS, handmade_correct      # noqa: E402
from tests.test_gpu_unitigs import code_of, count, row_values, stream_of      # noqa: E402
from tests.test_read_summary_restatement import HAND, RULES, S21, W21, expected_array      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_STATE = -1, -4
GUARD, FILL = 64, 0xEE
RS_WAVE_CAP = int(re.search(r"^#define RS_WAVE_CAP (\d+)", open(os.path.join(ROOT, "dsk_amd", "csrc", "readsum.h")).read(), flags=re.M).group(1))
ZERO = dict.fromkeys(M.STATS, 0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


# ------------------------------------------------------------------ one call each, guard bytes round every output
def as_np(text):
    return np.frombuffer(text if isinstance(text, bytes) else text.encode(), dtype=np.uint8).copy()


def put(dev, stream, off=0):
    """the stream at offset `off` of a 16-byte aligned allocation, separators around it"""
    t = torch.full((len(stream) + off + GUARD,), 10, dtype=torch.uint8, device=dev)
    t[off: off + len(stream)] = torch.from_numpy(np.ascontiguousarray(stream)).to(dev)
    assert t.data_ptr() % 16 == 0
    return t


def guarded(dev, nbytes, off=0):
    return torch.full((nbytes + off + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)


def inside(buf, nbytes, off=0):
    b = buf.cpu().numpy()
    assert (b[: GUARD + off] == FILL).all() and (b[GUARD + off + nbytes:] == FILL).all(), "guard bytes"
    return b[GUARD + off: GUARD + off + nbytes].copy()


def summarise(kc, dev, stream, trust_min=0, off=0):
    """-> (the table as numpy, the stats)"""
    from dsk_amd.engine import READ_SUMMARY_DTYPE
    n = len(stream)
    src = put(dev, stream, off)
    torch.cuda.synchronize()
    st = kc.read_summaries(src.data_ptr() + off if n else 0, n, trust_min)
    nr = st["n_records"]
    buf = guarded(dev, 32 * nr)
    torch.cuda.synchronize()
    kc.read_summaries_table(buf.data_ptr() + GUARD)
    torch.cuda.synchronize()
    T = inside(buf, 32 * nr).view(READ_SUMMARY_DTYPE)
    back = src.cpu().numpy()
    assert (back[off: off + n] == stream).all() and (back[:off] == 10).all() and (back[off + n:] == 10).all(), "the input is left as it was"
    return T, st


def device_marks(kc, dev, n_records, off=1, **rule):
    """-> (u8[n_records] at an odd address, the stats)"""
    buf = guarded(dev, n_records, off)
    torch.cuda.synchronize()
    st = kc.read_marks(buf.data_ptr() + GUARD + off, **rule)
    torch.cuda.synchronize()
    return inside(buf, n_records, off), st


def device_select(kc, dev, stream, keep, off_in=0, off_out=0):
    """the sizing run, then the real one -> the selected bytes"""
    n, nr = len(stream), len(keep)
    src, kp = put(dev, stream, off_in), put(dev, np.asarray(keep, dtype=np.uint8), 3)
    torch.cuda.synchronize()
    args = (src.data_ptr() + off_in, n, kp.data_ptr() + 3, nr)
    need, nrec = kc.select_reads(*args)
    assert nrec == int(np.count_nonzero(keep))
    out = guarded(dev, need, off_out)
    torch.cuda.synchronize()
    assert kc.select_reads(*args, out.data_ptr() + GUARD + off_out, need) == (need, nrec)
    torch.cuda.synchronize()
    assert (src.cpu().numpy()[off_in: off_in + n] == stream).all()
    return inside(out, need, off_out)


def same_table(got, want):
    assert got.dtype.itemsize == 32 and len(got) == len(want), (len(got), len(want))
    for f in M.FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, (f, len(bad), bad[:5], got[f][bad[:5]], want[f][bad[:5]], want["len"][bad[:5]])


def model_of(kc, k):
    kk, ab = kc.rows()
    return M.table_of(row_values(kk), ab, k)


def check_marks(kc, dev, T, rules):
    for rule in rules:
        want = M.marks(T, rule)
        keep, st = device_marks(kc, dev, len(T), **(rule or {}))
        assert (keep == want).all(), (rule, np.nonzero(keep != want)[0][:5])
        assert st == M.mark_stats(T, want), rule
        assert kc.read_marks(0, **(rule or {})) == st                         # the stats alone


def data_rules(T):
    """the rules of the restatement's test + every condition at a threshold that splits THIS table (read off the model's table)"""
    nz = T[T["n_valid"] > 0]
    med, nv = (int(np.median(nz["median"])), int(np.median(nz["n_valid"]))) if len(nz) else (1, 1)
    return RULES + [dict(median_min=med), dict(median_max=max(med, 1)), dict(min_valid=nv), dict(solid_num=9, solid_den=10),
                    dict(min_valid=nv, median_min=max(med - 1, 0), median_max=med + 1, solid_num=1, solid_den=3),
                    dict(min_valid=nv, median_min=max(med - 1, 0), median_max=med + 1, solid_num=1, solid_den=3, invert=True),
                    dict(solid_num=0xFFFFFFFF, solid_den=0xFFFFFFFF), dict(median_max=0xFFFFFFFF, min_valid=0xFFFFFFFF)]


# ------------------------------------------------------------------ 1. the restatement, every key width and boundary
_parts = {}


def golden_part(oracle, golden_dir):
    if "g" not in _parts:
        whole = stream_of("golden", oracle, golden_dir)
        ends = np.flatnonzero(whole == M.NL)
        _parts["g"] = (whole, whole[: int(ends[599]) + 1].copy())
    return _parts["g"]


def streams(kind, k, oracle, golden_dir):
    """-> (the stream to count, the stream to summarise)"""
    if kind == "golden":
        return golden_part(oracle, golden_dir)
    counted, s, _ = handmade_correct(k)
    return counted, s


def parity_case(dev, kind, k, amin, order, tmins, oracle, golden_dir):
    counted, stream = streams(kind, k, oracle, golden_dir)
    with count(counted, dev, k, abundance_min=amin, partition_order=order) as kc:
        table = model_of(kc, k)
        for tmin in tmins:
            want, want_st = M.summaries(stream, table, k, tmin)
            got, st = summarise(kc, dev, stream, tmin)
            print("read summaries", kind, k, amin, order, tmin, st)
            assert st == want_st
            same_table(got, want)
            assert (kc.read_summaries_numpy() == got).all()
            check_marks(kc, dev, want, data_rules(want))
        if kind == "golden" and k <= 96:                                     # (the golden reads have 100 letters)
            assert want_st["n_solid"] > 0 and want_st["n_valid"] > want_st["n_solid"]


@pytest.mark.parametrize("kind,k", [("golden", k) for k in KS] + [("hand", k) for k in [1, 4] + KS])
def test_device_equals_the_model(oracle, golden_dir, dev, kind, k):
    """table, stats and marks, trust_min 0 and 3, on the golden reads and on the correction's handmade stream (every separator, lower case, N)"""
    parity_case(dev, kind, k, 2 if kind == "golden" else 1, False, (0, 3), oracle, golden_dir)


@pytest.mark.parametrize("k", [31, 65])
def test_partition_order(oracle, golden_dir, dev, k):
    parity_case(dev, "golden", k, 2, True, (0, 3), oracle, golden_dir)


def test_trust_min_above_and_below_abundance_min(oracle, golden_dir, dev):
    """abundance_min 2: trust_min 1 and 2 mark the same positions solid, 5 fewer"""
    parity_case(dev, "golden", 31, 2, False, (1, 2, 5), oracle, golden_dir)
    with count(golden_part(oracle, golden_dir)[0], dev, 31, abundance_min=2) as kc:
        part = golden_part(oracle, golden_dir)[1]
        s = [summarise(kc, dev, part, t)[1]["n_solid"] for t in (1, 2, 5)]
        assert s[0] == s[1] > s[2] > 0


@pytest.mark.parametrize("k", [4, 21])
def test_the_tables_written_out_by_hand(dev, k):
    """counts crafted to the hand-made abundances (one line of k letters per occurrence) -> the table written out in the restatement's test"""
    stream, table, tmin, want, want_stats = HAND[k]
    lines = {4: [("ACGT", 7), ("CGTA", 2), ("AAAA", 5), ("GTAC", 9)], 21: [(S21[i: i + 21], W21[i]) for i in range(10)]}[k]
    counted = as_np("".join((s + "\n") * c for s, c in lines))
    with count(counted, dev, k, abundance_min=1) as kc:
        assert model_of(kc, k) == table
        got, st = summarise(kc, dev, as_np(stream), tmin)
        same_table(got, expected_array(want))
        assert st == want_stats
        check_marks(kc, dev, expected_array(want), RULES)


# ------------------------------------------------------------------ 2. a second path to the same table
@pytest.mark.parametrize("kind,k", [("golden", 15), ("hand", 33), ("hand", 127), ("golden", 64)])
def test_reductions_over_query_reads_and_k_enumerate(oracle, golden_dir, dev, kind, k):
    """per record: numpy reductions over the output of dskgpu_query_reads at the positions dskgpu_k_enumerate calls valid"""
    counted, stream = streams(kind, k, oracle, golden_dir)
    tmin = 3
    with count(counted, dev, k, abundance_min=1) as kc:
        got, st = summarise(kc, dev, stream, tmin)
        t = torch.from_numpy(stream).to(dev)
        a = kc.query_reads_tensor(t).cpu().numpy().view(np.uint32).astype(np.int64)
        kmers = torch.zeros((len(stream), kc.words), dtype=torch.int64, device=dev)
        valid = torch.zeros(len(stream), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        kc.k_enumerate(t.data_ptr(), len(stream), kmers.data_ptr(), valid.data_ptr())
        torch.cuda.synchronize()
        valid = valid.cpu().numpy() != 0
        recs = M.records(bytes(stream))
        assert len(recs) == len(got) == st["n_records"]
        for (start, ln), s in zip(recs, got):
            v = np.sort(a[start: start + ln][valid[start: start + ln]])
            want = (start, int(v.sum()), ln, len(v), int((v >= tmin).sum()), int(v[len(v) // 2]) if len(v) else 0)
            assert tuple(int(x) for x in s) == want
        assert st["n_valid"] == int(valid.sum())


# ------------------------------------------------------------------ 3. geometry
K_GEO, GEO_TMIN = 5, 45
_geo = {}


def geometry_stream():
    """records of every length at which a path changes, at k = 5 (512 canonical k-mers: large and varied abundances, many ties), one record
    of 70 000 A -- abundance 69 996 > 2^16, on the block path -- and 5 000 records of one byte"""
    if "s" not in _geo:
        rng = np.random.default_rng(77)
        lens = [0, 1, K_GEO - 1, K_GEO, K_GEO + 1, 31, 32, 33, 63, 64, 65, RS_WAVE_CAP - 1, RS_WAVE_CAP, RS_WAVE_CAP + 1, 4095, 4096, 4097, 0, 0,
                RS_WAVE_CAP + 64, 2 * RS_WAVE_CAP + 1, 127, 128, 129, 191, 192, 193]
        recs = ["".join("ACGT"[i] for i in rng.integers(0, 4, n)) for n in lens]
        recs.insert(9, "A" * 70000)
        recs[20] = recs[20][:100] + "N" + recs[20][101:200] + "n" + recs[20][201:]
        ones = ["ACGTN"[i] for i in rng.integers(0, 5, 5000)]
        _geo["s"] = (as_np("\n".join(recs + ones) + "\n"), len(recs))
    return _geo["s"]


@pytest.fixture(scope="module")
def geo(dev):
    """the geometry stream counted at k = 5, its model table and the model's summaries (computed once, shared, never changed)"""
    stream, n_first = geometry_stream()
    with count(stream, dev, K_GEO, abundance_min=1) as kc:
        table = model_of(kc, K_GEO)
        want, want_st = M.summaries(stream, table, K_GEO, GEO_TMIN)
        yield kc, stream, want, want_st, n_first


def test_every_length_at_which_a_path_changes(dev, geo):
    kc, stream, want, want_st, n_first = geo
    assert want_st["max_len"] == 70000 and want_st["n_records"] == n_first + 5000
    long_one = want[9]
    assert (int(long_one["len"]), int(long_one["n_valid"])) == (70000, 69996) and int(long_one["median"]) >= 69996 > 1 << 16      # (poly-A elsewhere adds to it)
    assert int(long_one["sum"]) == 69996 * int(long_one["median"]) > 1 << 32
    assert 0 < want_st["n_solid"] - 69996 < want_st["n_valid"] - 69996
    assert (want["len"] == RS_WAVE_CAP).any() and (want["len"] == RS_WAVE_CAP + 1).any() and (want["len"] == RS_WAVE_CAP - 1).any()
    got, st = summarise(kc, dev, stream, GEO_TMIN)
    assert st == want_st
    same_table(got, want)
    check_marks(kc, dev, want, data_rules(want))


@pytest.mark.parametrize("off", [1, 2, 3, 15])
def test_streams_at_odd_addresses(dev, geo, off):
    """the stream at offsets 1..3 and 15 of a 16-byte aligned allocation (offset 0: the test above): the same table"""
    kc, stream, want, want_st, _ = geo
    got, st = summarise(kc, dev, stream, GEO_TMIN, off)
    assert st == want_st
    same_table(got, want)


@pytest.mark.parametrize("shift", [1, 17, 4095, 4096 - 70001 % 4096])
def test_records_moved_across_the_blocks(dev, geo, shift):
    """`shift` bytes of a record without a window in front: the same summaries `shift` bytes further on (the words of the frame, the 16-byte
    loads and the 4096-byte blocks of the record kernels cut the records elsewhere)"""
    kc, stream, want, want_st, _ = geo
    moved = np.concatenate([np.full(shift - 1, ord("N"), dtype=np.uint8), as_np("\n"), stream[:80000]])
    want2, want_st2 = M.summaries(moved, model_of(kc, K_GEO), K_GEO, GEO_TMIN)
    got, st = summarise(kc, dev, moved, GEO_TMIN)
    assert st == want_st2
    same_table(got, want2)
    nrec = len(got) - 1
    assert (got["start"][1:] == want["start"][:nrec] + shift).all() and (got["median"][1:nrec] == want["median"][:nrec - 1]).all()


def test_many_records_of_one_byte(dev, geo):
    """5 000 one-byte records and nothing else: many records per block of the record kernels, none with a window"""
    kc, stream, _, _, n_first = geo
    ones = stream[-10000:]
    got, st = summarise(kc, dev, ones)
    assert st == dict(n_records=5000, n_empty=5000, n_valid=0, n_solid=0, max_len=1)
    assert (got["start"] == 2 * np.arange(5000)).all() and (got["len"] == 1).all()
    for f in ("sum", "n_valid", "n_solid", "median"):
        assert (got[f] == 0).all()
    got, st = summarise(kc, dev, ones[:-1])                                  # and without the final newline
    assert st["n_records"] == 5000 and int(got["len"][-1]) == 1 and int(got["start"][-1]) == 9998
    got, st = summarise(kc, dev, as_np("\n" * 4097))
    assert st == dict(n_records=4097, n_empty=4097, n_valid=0, n_solid=0, max_len=0) and (got["start"] == np.arange(4097)).all()


# ------------------------------------------------------------------ 4. the median's corner cases
def craft_abundances(kc, dev, new_ab):
    """overwrite the abundance column of the result on the device (rows in result order): counts no stream of a test's size can reach"""
    _, ap, n = kc.result_device()
    assert n == len(new_ab)
    t = torch.from_numpy(np.asarray(new_ab, dtype=np.uint32).view(np.int32)).to(dev)
    torch.cuda.synchronize()
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(C.c_void_p(ap), C.c_void_p(t.data_ptr()), C.c_size_t(4 * n), 3) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("length", [40, 3 * RS_WAVE_CAP + 7])
def test_median_corner_cases(dev, length):
    """all values equal; all zero; exactly half zero (the median is the first non-zero at even n_valid); a single valid window; values that
    differ only in bit 31 -- on the wave path (40 letters) and on the block path"""
    k = 13
    rng = np.random.default_rng(length)
    rnd = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, n))      # noqa: E731
    half = (length - k + 1) // 2
    seen, absent = rnd(length), rnd(length)
    while {M.canon(absent[i: i + k]) for i in range(length - k + 1)} & {M.canon(seen[i: i + k]) for i in range(length - k + 1)}:
        absent = rnd(length)
    equal = "AC" * (length // 2)                                             # two k-mers, each other's neighbours, the same count
    recs = [equal, absent, seen[: k - 1 + half] + "N" + absent[: k - 1 + half], absent[:k - 1 + half] + "N" + seen[: k - 1 + half], seen[:k], seen, seen[: length - 1]]
    stream = as_np("\n".join(recs) + "\n")
    counted = as_np("\n".join([equal, equal, seen, seen, seen]) + "\n")
    with count(counted, dev, k, abundance_min=1) as kc:
        table = model_of(kc, k)
        assert not any(M.canon(absent[i: i + k]) in table for i in range(length - k + 1))
        want, want_st = M.summaries(stream, table, k, 3)
        got, st = summarise(kc, dev, stream, 3)
        same_table(got, want)
        assert st == want_st
        nv = length - k + 1
        assert int(want["n_valid"][0]) == len(equal) - k + 1 and int(want["median"][0]) * int(want["n_valid"][0]) == int(want["sum"][0])      # all equal
        assert (int(want["n_valid"][1]), int(want["sum"][1]), int(want["median"][1])) == (nv, 0, 0)        # all zero
        assert int(want["n_valid"][2]) == int(want["n_valid"][3]) == 2 * half and int(want["median"][2]) == int(want["median"][3]) == 3
        assert int(want["n_valid"][4]) == 1 and int(want["median"][4]) == 3
        # values that differ only in bit 31: every second row gets it
        kk, ab = kc.rows()
        crafted = (ab.astype(np.uint32) | (np.arange(len(ab), dtype=np.uint32) & 1) << 31).astype(np.uint32)
        craft_abundances(kc, dev, crafted)
        table = model_of(kc, k)
        assert sorted(table.values())[-1] >= 1 << 31 and sorted(table.values())[0] < 1 << 31
        want, want_st = M.summaries(stream, table, k, 1 << 31)
        got, st = summarise(kc, dev, stream, 1 << 31)
        same_table(got, want)
        assert st == want_st and int(want["sum"].max()) > 1 << 32 and 0 < want_st["n_solid"] < want_st["n_valid"]
        assert (want["median"] >= 1 << 31).any() and ((want["median"] > 0) & (want["median"] < 1 << 31)).any()
        check_marks(kc, dev, want, [dict(median_min=1 << 31), dict(median_max=(1 << 31) - 1), dict(solid_num=1, solid_den=2)])


# ------------------------------------------------------------------ 5. the selection
def test_selection_equals_the_model(dev, geo):
    """all kept, none kept, alternating, only the long record, the marks of a rule; the sizing run then the real one; odd addresses"""
    kc, stream, want, _, n_first = geo
    nr = len(want)
    keeps = {"all": np.ones(nr, dtype=np.uint8), "none": np.zeros(nr, dtype=np.uint8), "even": (np.arange(nr) % 2 == 0).astype(np.uint8),
             "odd": (np.arange(nr) % 2 == 1).astype(np.uint8) * 7, "long": (np.arange(nr) == 9).astype(np.uint8),
             "rule": M.marks(want, dict(min_valid=1, median_min=int(np.median(want["median"][:n_first]))))}
    for name, keep in keeps.items():
        for off_in, off_out in ((0, 0), (3, 5)):
            got = device_select(kc, dev, stream, keep, off_in, off_out)
            exp = M.select(stream, keep)
            assert len(got) == len(exp) and (got == exp).all(), (name, off_in, off_out)
    assert (M.select(stream, keeps["all"]) == stream).all() and len(M.select(stream, keeps["long"])) == 70001
    head = stream[: 80000 if stream[79999] != M.NL else 79999]                 # a last record without a newline gets one
    nh = len(M.records(bytes(head)))
    got = device_select(kc, dev, head, np.ones(nh, dtype=np.uint8), 1, 1)
    assert (got[:-1] == head).all() and got[-1] == M.NL
    t, kp = torch.from_numpy(stream).to(dev), torch.from_numpy(keeps["rule"]).to(dev)
    assert (kc.select_reads_tensor(t, kp).cpu().numpy() == M.select(stream, keeps["rule"])).all()
    assert (kc.select_reads_tensor(t, kp != 0).cpu().numpy() == M.select(stream, keeps["rule"])).all()
    assert kc.select_reads_tensor(t, torch.zeros(nr, dtype=torch.uint8, device=dev)).numel() == 0


def test_capacity_one_byte_short(dev, geo):
    """DSKGPU_E_ARG, the need reported, the output buffer untouched"""
    kc, stream, want, _, _ = geo
    keep = (np.arange(len(want)) % 3 == 0).astype(np.uint8)
    need = len(M.select(stream, keep))
    src, kp, out = put(dev, stream), put(dev, keep), guarded(dev, need)
    torch.cuda.synchronize()
    ob, orec = C.c_uint64(0), C.c_uint64(0)
    lib, h = kc._lib, kc._h
    assert lib.dskgpu_select_reads(h, src.data_ptr(), len(stream), kp.data_ptr(), len(keep), out.data_ptr() + GUARD, need - 1, C.byref(ob), C.byref(orec)) == E_ARG
    torch.cuda.synchronize()
    assert ob.value == need and (out == FILL).all()
    assert lib.dskgpu_select_reads(h, src.data_ptr(), len(stream), kp.data_ptr(), len(keep), out.data_ptr() + GUARD, need, None, None) == 0
    torch.cuda.synchronize()
    assert (inside(out, need) == M.select(stream, keep)).all()


@pytest.mark.parametrize("k", [31, 64])
def test_the_selection_counts_back_to_the_kept_records(oracle, golden_dir, dev, k):
    """the selected stream pushed into a fresh KmerCounter and counted equals the oracle's count of the model's selection"""
    whole, part = golden_part(oracle, golden_dir)
    with count(whole, dev, k, abundance_min=2) as kc:
        T, st = summarise(kc, dev, part, 3)
        rule = dict(min_valid=1, median_min=int(np.median(T["median"])), solid_num=1, solid_den=2)
        keep, mst = device_marks(kc, dev, len(T), **rule)
        assert 0 < mst["n_kept"] < len(T)
        sel = device_select(kc, dev, part, keep)
        assert len(sel) == mst["kept_bytes"]
    exp = M.select(part, M.marks(T, rule))
    assert (sel == exp).all()
    ref = oracle.count(exp, k)
    pairs = sorted((int(v), int(a)) for v, a in zip(ref.values(), ref.ab))
    with count(sel, dev, k, abundance_min=1) as kc2:
        kk, ab = kc2.rows()
        assert sorted(zip(row_values(kk), (int(a) for a in ab))) == pairs
        assert kc2.stats()["n_kmers"] == mst["kept_valid"]


def test_select_on_a_context_that_has_never_counted(dev):
    from dsk_amd import KmerCounter
    stream = as_np("ACGT\n\nNNNN\r\nacgtacgt\nTT")
    keep = np.array([1, 0, 1, 0, 1], dtype=np.uint8)
    with KmerCounter(kmer_size=31) as kc:
        got = device_select(kc, dev, stream, keep, 1, 2)
        assert bytes(got) == b"ACGT\nNNNN\r\nTT\n"
        assert kc.select_reads(0, 0, 0, 0) == (0, 0)


# ------------------------------------------------------------------ 6. the contract
def test_bad_arguments(dev, geo):
    from dsk_amd import engine
    kc, stream, want, want_st, _ = geo
    lib, h = kc._lib, kc._h
    src = put(dev, stream)
    nr = len(want)
    kp, out = put(dev, np.ones(nr, dtype=np.uint8)), guarded(dev, len(stream) + 1)
    torch.cuda.synchronize()
    p, n = src.data_ptr(), len(stream)
    st = engine._ReadSummaryStats()
    assert lib.dskgpu_read_summaries(h, None, n, None, C.byref(st)) == E_ARG
    for par in (engine._ReadSummaryParams(flags=1), engine._ReadSummaryParams(reserved=(0, 0, 1)), engine._ReadSummaryParams(trust_min=3, reserved=(1, 0, 0))):
        assert lib.dskgpu_read_summaries(h, p, n, C.byref(par), C.byref(st)) == E_ARG
    assert lib.dskgpu_read_summaries(h, p, (0x7FFFFFFF << 11) + 1, None, None) == E_ARG
    assert lib.dskgpu_read_summaries(h, p, n, None, None) == 0               # params and stats may be NULL
    assert lib.dskgpu_read_summaries_table(h, None) == E_ARG
    ms = engine._ReadMarkStats()
    assert lib.dskgpu_read_marks(h, None, None, None) == E_ARG               # neither d_keep nor stats
    for rule in (engine._ReadRule(flags=2), engine._ReadRule(flags=3), engine._ReadRule(reserved=1)):
        assert lib.dskgpu_read_marks(h, C.byref(rule), None, C.byref(ms)) == E_ARG
    assert lib.dskgpu_read_marks(h, None, None, C.byref(ms)) == 0 and ms.n_kept == ms.n_records == nr and ms.kept_bytes == n      # a null rule keeps everything
    ob, orec = C.c_uint64(0), C.c_uint64(0)
    sel = lambda *a: lib.dskgpu_select_reads(h, *a, C.byref(ob), C.byref(orec))      # noqa: E731
    assert sel(None, n, kp.data_ptr(), nr, None, 0) == E_ARG
    assert sel(p, n, None, nr, None, 0) == E_ARG
    for wrong in (nr - 1, nr + 1, 0):
        assert sel(p, n, kp.data_ptr(), wrong, out.data_ptr() + GUARD, n + 1) == E_ARG
    assert sel(p, (0x7FFFFFFF << 11) + 1, kp.data_ptr(), nr, None, 0) == E_ARG
    assert sel(None, 0, None, 1, None, 0) == E_ARG
    torch.cuda.synchronize()
    assert (out == FILL).all()
    assert sel(p, n, kp.data_ptr(), nr, None, 0) == 0 and (ob.value, orec.value) == (n, nr)
    got, st2 = summarise(kc, dev, stream, GEO_TMIN)                              # and the context still answers
    same_table(got, want)
    assert st2 == want_st


def test_state_errors_and_an_empty_stream(oracle, golden_dir, dev):
    """no result; a table or marks call with nothing kept; nbytes == 0"""
    from dsk_amd import KmerCounter
    buf = torch.zeros(1024, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p = buf.data_ptr()
    with KmerCounter(kmer_size=31) as kc:
        for call in (lambda: kc.read_summaries(p, 64), lambda: kc.read_summaries(0, 0), lambda: kc.read_summaries_table(p), lambda: kc.read_marks(p),
                     lambda: kc.read_marks(0)):
            assert code_of(call) == E_STATE
    whole, part = golden_part(oracle, golden_dir)
    with count(whole, dev, 31, abundance_min=2) as kc:
        assert code_of(lambda: kc.read_summaries_table(p)) == E_STATE and code_of(lambda: kc.read_marks(p)) == E_STATE
        T, st = summarise(kc, dev, part)
        assert st["n_records"] == 600
        assert kc.read_summaries(0, 0) == ZERO                                # an empty stream: a table of zero records is kept
        out = guarded(dev, 64)
        torch.cuda.synchronize()
        kc.read_summaries_table(out.data_ptr() + GUARD)
        assert kc.read_marks(out.data_ptr() + GUARD) == dict.fromkeys(M.MARK_STATS, 0)
        torch.cuda.synchronize()
        assert (out == FILL).all()
        assert len(kc.read_summaries_numpy()) == 0


def test_a_result_without_rows(oracle, golden_dir, dev):
    """every value is 0: n_valid is still counted"""
    whole, part = golden_part(oracle, golden_dir)
    with count(whole, dev, 31, abundance_min=10 ** 6) as kc:
        assert kc.stats()["n_solid"] == 0
        T, st = summarise(kc, dev, part)
        assert st == dict(n_records=600, n_empty=0, n_valid=600 * 70, n_solid=0, max_len=100)
        assert (T["n_valid"] == 70).all() and (T["sum"] == 0).all() and (T["median"] == 0).all() and (T["n_solid"] == 0).all()
        keep, mst = device_marks(kc, dev, 600, median_min=1)
        assert mst["n_kept"] == 0 and not keep.any()


def test_a_rank_of_a_group_is_a_state_error(oracle, golden_dir, dev):
    """world_size > 1: DSKGPU_E_STATE, and the text names world_size"""
    from dsk_amd import KmerGroup
    s = stream_of("golden", oracle, golden_dir)
    recs = bytes(s).split(b"\n")
    buf = torch.zeros(1024, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p = buf.data_ptr()
    with KmerGroup([0, 0], kmer_size=31, abundance_min=2) as g:
        for r in range(2):
            g.rank(r).push_reads(b"\n".join(recs[r::2]) + b"\n")
        g.count()
        kc = g.rank(0)
        assert code_of(lambda: kc.read_summaries(p, 64)) == E_STATE
        assert "world_size" in kc._lib.dskgpu_last_error(kc._h).decode()


def test_the_lifetime_of_the_table_and_the_context_left_alone(oracle, golden_dir, dev):
    """dropped by a new count and by filter_rows; rows, stats and histogram before and after; count -> summaries -> count: identical rows"""
    whole, part = golden_part(oracle, golden_dir)
    buf = torch.zeros(32 * 600, dtype=torch.uint8, device=dev)
    with count(whole, dev, 31, abundance_min=2) as kc:
        k1, a1 = kc.rows(); h1 = kc.histogram(); s1 = kc.stats()
        T, st = summarise(kc, dev, part, 3)
        k2, a2 = kc.rows()
        assert (k1 == k2).all() and (a1 == a2).all() and (kc.histogram() == h1).all() and kc.stats() == s1
        kc.count()                                                           # a new count drops the table ...
        assert code_of(lambda: kc.read_summaries_table(buf.data_ptr())) == E_STATE and code_of(lambda: kc.read_marks(buf.data_ptr())) == E_STATE
        k3, a3 = kc.rows()
        assert (k1 == k3).all() and (a1 == a3).all()                         # ... and gives identical rows
        T2, st2 = summarise(kc, dev, part, 3)
        same_table(T2, T)
        assert st2 == st
        keep = torch.from_numpy((a1 >= 4).astype(np.uint8)).to(dev)
        left = kc.filter_rows_tensor(keep)                                   # filter_rows drops it too
        assert 0 < left < len(a1)
        assert code_of(lambda: kc.read_summaries_table(buf.data_ptr())) == E_STATE
        T3, st3 = summarise(kc, dev, part, 3)                                # and the next table is that of the rows left
        want, want_st = M.summaries(part, model_of(kc, 31), 31, 3)
        same_table(T3, want)
        assert st3 == want_st and st3["n_solid"] < st["n_solid"]


def test_stage_times_name_the_stages(oracle, golden_dir, dev):
    whole, part = golden_part(oracle, golden_dir)
    names = ("read values", "read records", "read summaries")
    with count(whole, dev, 31, abundance_min=2, timing=True) as kc:
        before = dict(kc.stage_times())
        assert not any(n in before for n in names + ("query index", "read select"))
        T, _ = summarise(kc, dev, part)
        after = dict(kc.stage_times())
        assert all(after[n] > 0 for n in names) and after["query index"] > 0 and "read select" not in after
        device_select(kc, dev, part, np.ones(len(T), dtype=np.uint8))
        assert dict(kc.stage_times())["read select"] > 0
