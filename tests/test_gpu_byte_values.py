"""Every byte value through every entry that reads a byte stream.  k_encode (csrc/kernels.h) decides "is this byte a base?" for all of them,
four bytes per 32-bit word; the streams of tests/byte_streams.py put each of the 248 values that are no base between two fragments of
bases, at every position of a word, and the 24 values that differ from a base in their top two bits only among them.

All comparisons are exact.  The reference for "is a base" is membership in ACGTacgt: the table of byte_streams.encode_reference, the
oracle's table, the string models' _BASES -- never the device's arithmetic.  That these inputs can fail is shown on the CPU
(tests/test_byte_streams_restatement.py): any one value taken for a base changes the oracle's answer at every k used here.
  a  dskgpu_k_encode against the table: layout, pad, both load paths, every alignment, short streams, the grid-stride loop
  b  dskgpu_k_enumerate / dskgpu_k_minimizers against the oracle
  c  the count against the oracle: device-resident at two alignments, pushed in pieces, from a kept encoding; both row orders
  d  query_reads, thread_place / thread_reads, correct_reads, read_summaries / read_marks / select_reads, colors_add against their models
  e  FASTA / FASTQ text through the device parser
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import byte_streams as B      # noqa: E402
from tests import color_model, read_summary_model      # noqa: E402
from tests import test_gpu_colors as TC      # noqa: E402
from tests import test_gpu_correct as TK      # noqa: E402
from tests import test_gpu_query as TQ      # noqa: E402
from tests import test_gpu_raw_parse as TR      # noqa: E402
from tests import test_gpu_read_summaries as TS      # noqa: E402
from tests import test_gpu_thread as TT      # noqa: E402
from tests.test_correct_restatement import CorrectRestatement      # noqa: E402
from tests.test_gpu_parity import check_against_oracle      # noqa: E402
from tests.test_gpu_unitigs import count, row_values      # noqa: E402
from tests.test_thread_restatement import ThreadRestatement      # noqa: E402

GUARD_WORDS = 8
PATTERN64, PATTERN32 = 0x5AA5C33C0FF0699A, 0x5AA5C33C


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


all_stream, cut_streams = B.device_all_stream, B.device_cut_streams      # (the streams the CPU file has checked)


def put(dev, stream, off):
    """the stream at byte `off` of a 16-byte aligned allocation, newlines around it -> (the allocation, the stream's device address)"""
    t = torch.full((len(stream) + off + 64,), 10, dtype=torch.uint8, device=dev)
    t[off: off + len(stream)] = torch.from_numpy(np.ascontiguousarray(stream)).to(dev)
    assert t.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    return t, t.data_ptr() + off


def unchanged(t, stream, off):
    back = t.cpu().numpy()
    return (back[off: off + len(stream)] == stream).all() and (back[:off] == 10).all() and (back[off + len(stream):] == 10).all()


# ------------------------------------------------------------------ a. k_encode against the table
def encode(kc, dev, stream, off):
    """one dskgpu_k_encode with guard words before and behind both outputs -> (packed u64[nw], inval u32[nw])"""
    n = len(stream)
    nw = (n + 31) // 32
    src, p = put(dev, stream, off)
    packed = torch.from_numpy(np.full(nw + 2 * GUARD_WORDS, PATTERN64, dtype=np.uint64).view(np.int64)).to(dev)
    inval = torch.from_numpy(np.full(nw + 2 * GUARD_WORDS, PATTERN32, dtype=np.uint32).view(np.int32)).to(dev)
    torch.cuda.synchronize()
    kc.k_encode(p, n, packed.data_ptr() + 8 * GUARD_WORDS, inval.data_ptr() + 4 * GUARD_WORDS)
    torch.cuda.synchronize()
    gp, gi = packed.cpu().numpy().view(np.uint64), inval.cpu().numpy().view(np.uint32)
    for g, pattern in ((gp, PATTERN64), (gi, PATTERN32)):
        assert (g[:GUARD_WORDS] == pattern).all() and (g[GUARD_WORDS + nw:] == pattern).all(), "exactly (n + 31) // 32 words are written"
    assert unchanged(src, stream, off), "the input is left as it was"
    return gp[GUARD_WORDS: GUARD_WORDS + nw], gi[GUARD_WORDS: GUARD_WORDS + nw]


def check_encode(kc, dev, stream, off, ref=None):
    packed, inval = encode(kc, dev, stream, off)
    want_p, want_i, mask = ref if ref is not None else B.encode_reference(stream)
    bad = np.flatnonzero(inval != want_i)
    assert len(bad) == 0, ("inval", len(stream), off, len(bad), bad[:5], [hex(int(x)) for x in inval[bad[:5]]], [hex(int(x)) for x in want_i[bad[:5]]])
    bad = np.flatnonzero((packed & mask) != want_p)
    assert len(bad) == 0, ("packed", len(stream), off, len(bad), bad[:5], [hex(int(x)) for x in packed[bad[:5]]], [hex(int(x)) for x in want_p[bad[:5]]])


@pytest.mark.parametrize("off", range(16))
def test_encode_at_every_alignment(dev, off):
    """the "all" stream from every byte offset of a 16-byte aligned allocation: offset 0 takes the two 16-byte loads, the others byte loads"""
    from dsk_amd import KmerCounter
    s = all_stream(31)
    assert len(s) % 32 != 0
    with KmerCounter(kmer_size=31) as kc:
        check_encode(kc, dev, s, off)


def test_encode_short_streams(dev):
    """0 .. 33, 63, 64, 65 bytes and one block's worth (8192) less, exactly and more; each length cut from the stream twice, so that once a
    byte that is no base and once a base is the last one; the pad of the last word reads as invalid"""
    from dsk_amd import KmerCounter
    with KmerCounter(kmer_size=31) as kc:
        for n in list(range(34)) + [63, 64, 65, 8191, 8192, 8193]:
            s = all_stream(4 if n <= 65 else 31)                                 # (short fragments for the short cuts)
            at, _ = B.separators(s)
            ends = [int(at[at >= max(n, 1) - 1][3]) + 1, int(at[at >= max(n, 1)][5])] if n else [0]      # behind a separator / before one: behind a base
            for end in ends:
                cut = s[end - n: end]
                assert len(cut) == n and (n == 0 or bool(B.IS_BASE[cut[-1]]) == (end != ends[0]))
                for off in (0, 5):
                    check_encode(kc, dev, cut, off)


def test_encode_grid_stride(dev):
    """1.5 x (CUs x 16 blocks x 8192 bytes): the kernel's grid-stride loop runs a second time for half of the blocks"""
    from dsk_amd import KmerCounter
    n = 3 * torch.cuda.get_device_properties(dev).multi_processor_count * 16 * 8192 // 2
    print("encode grid stride", torch.cuda.get_device_properties(dev).multi_processor_count, "CUs", n, "bytes")
    assert n > 16 * 8192
    s = np.resize(all_stream(31), n)
    ref = B.encode_reference(s)
    with KmerCounter(kmer_size=31) as kc:
        check_encode(kc, dev, s, 0, ref)


# ------------------------------------------------------------------ b. k_enumerate and k_minimizers against the oracle
@pytest.mark.parametrize("k", B.ENUM_KS)
def test_enumerate_matches_oracle(oracle, dev, k):
    from dsk_amd import KmerCounter
    s = all_stream(k)
    wo = (k + 31) // 32
    words, valid = oracle.enumerate_words(s, k)
    assert 0 < valid.sum() < len(s)
    with KmerCounter(kmer_size=k) as kc:
        for off in (0, 3):
            src, p = put(dev, s, off)
            out = torch.zeros(wo * len(s), dtype=torch.int64, device=dev)
            val = torch.full((len(s),), 7, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            kc.k_enumerate(p, len(s), out.data_ptr(), val.data_ptr())
            got_v, got = val.cpu().numpy(), out.cpu().numpy().view(np.uint64).reshape(-1, wo)
            bad = np.flatnonzero(got_v != valid)
            assert len(bad) == 0, (k, off, len(bad), bad[:5], s[bad[:5]], got_v[bad[:5]])
            bad = np.flatnonzero((got != words[:, :wo]).any(axis=1))
            assert len(bad) == 0, (k, off, len(bad), bad[:5])
            assert unchanged(src, s, off)


@pytest.mark.parametrize("k,m", B.MINIMIZER_KM)
def test_minimizers_match_oracle(oracle, dev, k, m):
    from dsk_amd import KmerCounter
    s = all_stream(k)
    ref_m, ref_v = oracle.minimizers(s, k, m)
    assert 0 < ref_v.sum() < len(s) and len(np.unique(ref_m[ref_v != 0])) > 1
    with KmerCounter(kmer_size=k, minimizer_size=m) as kc:
        for off in (0, 3):
            src, p = put(dev, s, off)
            mm = torch.zeros(len(s), dtype=torch.int32, device=dev)
            val = torch.full((len(s),), 7, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            kc.k_minimizers(p, len(s), mm.data_ptr(), val.data_ptr())
            bad = np.flatnonzero(val.cpu().numpy() != ref_v)
            assert len(bad) == 0, (k, m, off, len(bad), bad[:5], s[bad[:5]])
            got_m = mm.cpu().numpy().view(np.uint32)
            bad = np.flatnonzero(got_m != ref_m)
            assert len(bad) == 0, (k, m, off, len(bad), bad[:5], [hex(int(x)) for x in got_m[bad[:5]]], [hex(int(x)) for x in ref_m[bad[:5]]])
            assert unchanged(src, s, off)


# ------------------------------------------------------------------ c. the count against the oracle
def same_as_oracle(kc, ref, k, partition_order):
    kmers, ab = kc.rows()
    st = kc.stats()
    assert (st["n_kmers"], st["n_distinct"], st["n_solid"]) == (ref.total, ref.distinct, ref.distinct), st      # (abundance_min 1)
    assert (kc.histogram() == ref.histogram(10000)).all()
    assert kmers.shape == (ref.distinct, (k + 31) // 32)
    if partition_order:                                                          # (ascending inside each partition: the same rows)
        order = np.lexsort(kmers.T)
        kmers, ab = kmers[order], ab[order]
    assert (kmers == ref.words()).all() and (ab == ref.ab).all()


@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k", B.COUNT_KS)
def test_count_matches_oracle(oracle, dev, k, partition_order):
    """rows, abundances, histogram, n_kmers and n_distinct at abundance_min 1: the reads device-resident at offsets 0 and 7 of an aligned
    allocation, pushed in three pieces (a separator is implied behind a push), and from the encoding kept by encode_reads()"""
    from dsk_amd import KmerCounter
    s = all_stream(k)
    ref = oracle.count(s, k)
    assert ref.total > 0
    if not partition_order:
        check_against_oracle(oracle, s, k, dev, amin=1)
    for off in (0, 7):
        src, p = put(dev, s, off)
        with KmerCounter(kmer_size=k, abundance_min=1, partition_order=partition_order) as kc:
            kc.set_reads_device(p, len(s))
            kc.count()
            same_as_oracle(kc, ref, k, partition_order)
        assert unchanged(src, s, off)
    # three pushes, cut inside fragments: bytes, a numpy array, bytes
    at, _ = B.separators(s)
    long = [int(a) + k + 1 for a, b in zip(at[:-1], at[1:]) if b - a - 1 >= 2 * k + 3]
    cuts = [0, long[len(long) // 3], long[2 * len(long) // 3], len(s)]
    pushed = np.concatenate([np.concatenate([s[a: b], [B.NL]]) for a, b in zip(cuts[:-1], cuts[1:])]).astype(np.uint8)
    ref_pushed = oracle.count(pushed, k)
    assert ref_pushed.total < ref.total
    with KmerCounter(kmer_size=k, abundance_min=1, partition_order=partition_order) as kc:
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            kc.push_reads(s[a: b].copy() if i == 1 else s[a: b].tobytes())
        kc.count()
        same_as_oracle(kc, ref_pushed, k, partition_order)
    # the kept encoding: the bytes are overwritten before the count
    src, p = put(dev, s, 7)
    with KmerCounter(kmer_size=k, abundance_min=1, partition_order=partition_order) as kc:
        kc.set_reads_device(p, len(s))
        kc.encode_reads()
        src.fill_(ord("A"))
        torch.cuda.synchronize()
        kc.count()
        same_as_oracle(kc, ref, k, partition_order)


# ------------------------------------------------------------------ d. the entries with string models
@pytest.mark.parametrize("k", B.MODEL_KS)
def test_query_reads(oracle, dev, k):
    counted, alias, _, subst = cut_streams(k)
    ref = oracle.count(counted, k)
    with count(counted, dev, k, abundance_min=1) as kc:
        for stream, in_off, out_off in ((alias, 0, 0), (alias, 3, 1), (subst, 5, 0)):
            got = TQ.query_reads(kc, stream, dev, in_off, out_off)
            exp = TQ.expected_reads(oracle, ref, stream, k, 1, 2147483647)
            bad = np.flatnonzero(got != exp)
            assert len(bad) == 0, (k, in_off, len(bad), bad[:5], stream[bad[:5]], got[bad[:5]], exp[bad[:5]])
        valid = oracle.enumerate_words(alias, k)[1]
        got = TQ.query_reads(kc, alias, dev)
        assert ((got != 0) == (valid != 0)).all()                            # every window of a fragment of the counted reads is a row


@pytest.mark.parametrize("k", B.MODEL_KS)
def test_thread_place_and_reads(dev, k):
    counted, alias, _, subst = cut_streams(k)
    with count(counted, dev, k, abundance_min=1) as kc:
        kk, ab = kc.rows()
        exp = ThreadRestatement(row_values(kk), ab, k)
        for stream, odd in ((alias, False), (alias, True), (subst, True)):
            T = exp.thread(stream)
            exp.check_facts(T)
            assert T.stats["n_placed"] > 0 and T.stats["n_walks"] > 100
            TT.check_against_restatement(kc, T, TT.on_device(stream, dev, odd))


@pytest.mark.parametrize("mode", ["out", "inplace"])
@pytest.mark.parametrize("k", B.MODEL_KS)
def test_correct_reads(dev, k, mode):
    """states, stats and output bytes equal the restatement's; every byte it does not correct comes back as it went in, the values from
    0x80 on included"""
    counted, alias, _, subst = cut_streams(k)
    with count(counted, dev, k, abundance_min=1) as kc:
        kk, ab = kc.rows()
        exp = CorrectRestatement(row_values(kk), ab, k)
        for stream, offs in ((subst, (0, 0, 0)), (subst, (3, 1, 5)), (alias, (7, 2, 1))):
            R = exp.correct(stream)
            got = TK.run(kc, dev, stream, 0, offs, mode)
            TK.same(got, R)
            corrected = np.array([g[3] for g in R.gaps if g[4] == "corrected"], dtype=np.int64)
            rest = np.ones(len(stream), dtype=bool)
            rest[corrected] = False
            assert (got[0][rest] == stream[rest]).all() and (got[0][corrected] != stream[corrected]).all()
            assert int((stream[rest] >= 0x80).sum()) >= 128
            if stream is subst:
                assert R.stats["n_corrected"] >= 20 and R.stats["n_head"] > 0 and R.stats["n_tail"] > 0 and R.stats["n_interior"] > 0
            else:
                assert R.stats["n_gaps"] == 0 and R.stats["n_trusted"] == R.stats["n_valid"] > 0


@pytest.mark.parametrize("k", B.MODEL_KS)
def test_read_summaries_marks_and_selection(dev, k):
    """records split at '\\n' and at nothing else; the table, the stats and the marks equal the model's; the selected records are copied
    byte for byte"""
    counted, _, recs_stream, _ = cut_streams(k)
    M = read_summary_model
    parts = bytes(recs_stream).split(b"\n")
    starts = np.cumsum([0] + [len(r) + 1 for r in parts[:-1]])
    with count(counted, dev, k, abundance_min=1) as kc:
        table = TS.model_of(kc, k)
        for tmin, off in ((0, 0), (2, 3)):
            want, want_st = M.summaries(recs_stream, table, k, tmin)
            got, st = TS.summarise(kc, dev, recs_stream, tmin, off)
            assert st == want_st and st["n_records"] == len(parts) and st["n_solid"] > 0
            TS.same_table(got, want)
            assert (got["start"] == starts).all() and (got["len"] == [len(r) for r in parts]).all()
            TS.check_marks(kc, dev, want, TS.data_rules(want))
        keeps = [np.ones(len(parts), dtype=np.uint8), (np.arange(len(parts)) % 2 == 1).astype(np.uint8),
                 M.marks(want, dict(min_valid=1, median_min=int(np.median(want["median"]))))]
        for keep in keeps:
            for off_in, off_out in ((0, 0), (3, 5)):
                got = TS.device_select(kc, dev, recs_stream, keep, off_in, off_out)
                exp = b"".join(r + b"\n" for r, kp in zip(parts, keep) if kp)
                assert 0 < len(exp) and bytes(got) == exp == bytes(M.select(recs_stream, keep))


@pytest.mark.parametrize("k", B.MODEL_KS)
def test_colors_add_two_banks(dev, k):
    counted, alias, recs_stream, _ = cut_streams(k)
    M = color_model
    with count(counted, dev, k, abundance_min=1) as kc:
        rows = M.rows_of(row_values(kc.rows()[0]), k)
        for stream, off in ((recs_stream, 0), (recs_stream, 5), (alias, 3)):
            ends = M.split_at_records(stream, 2) if stream is recs_stream else [len(stream) // 2 + 1, len(stream)]
            model = M.Colours(rows, 2, k)
            want = model.add(stream, ends)
            kc.colors_begin(2)
            st = TC.add(kc, dev, stream, ends, 0, off)
            assert st == want and st["n_placed"] == st["n_valid"] > 0
            TC.check_against(kc, dev, model)


# ------------------------------------------------------------------ e. file text through the device parser
@pytest.mark.parametrize("fmt", ["fa", "fq"])
def test_raw_text_with_every_value(oracle, dev, fmt):
    """The k = 21 and k = 31 texts whole and in 7 random pieces; the k = 7 text, which carries every value as well and is short (under
    6000 bytes), in pieces of one byte: a cut at every position.  The stream the parser leaves has the length the rules give, and its count is
    the oracle's count of the records a host parser hands on.  ' ', '\\t' and '\\r' inside a FASTA line are dropped with the 24 alias
    values as their neighbours too"""
    rng = np.random.default_rng(23)
    for k in (21, 31):
        text = B.device_text(fmt, k)
        assert len(text) < 200_000
        TR.check(oracle, [(text, fmt)], k)
        TR.check(oracle, [(text, fmt)], k, rng, 7)
    small = B.device_text(fmt, 7)
    assert len(small) < 6000

    class EveryCut:                                                          # (what check() asks of its generator: the cut positions)
        def integers(self, lo, hi, n):
            return np.arange(lo + 1, hi - 1)
    assert TR.random_cuts(EveryCut(), len(small), 1) == list(range(len(small) + 1))
    TR.check(oracle, [(small, fmt)], 7, EveryCut(), 1)
