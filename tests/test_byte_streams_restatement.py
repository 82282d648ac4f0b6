"""The inputs of tests/test_gpu_byte_values.py (tests/byte_streams.py) checked on the CPU, with the oracle and the Python models alone:
what the builder promises, counted; that the inputs CAN fail -- turning any one of the 248 values that are no base into a base changes the
oracle's answers at every k the device tests use; the table reference of the encoded stream on streams worked out by hand; and the five
string models on bytes that str.upper() would not leave in place."""
from collections import Counter

import numpy as np
import pytest

pytest.importorskip("torch")          # (the modules the models come from import it at the top)
from tests import byte_streams as B      # noqa: E402
from tests import color_model, read_summary_model      # noqa: E402
from tests.test_correct_restatement import CorrectRestatement      # noqa: E402
from tests.test_gpu_raw_parse import host_records, model_stream      # noqa: E402
from tests.test_read_summary_restatement import kmer_counts      # noqa: E402
from tests.test_thread_restatement import ThreadRestatement      # noqa: E402
from tests.test_unitigs_restatement import solid_rows      # noqa: E402

# every stream below is the one tests/test_gpu_byte_values.py feeds: byte_streams.device_all_stream / device_cut_streams / device_text
DEVICE_STREAMS = [("all", k) for k in B.ALL_KS] + [(form, k) for k in B.MODEL_KS for form in ("alias", "alias_nl", "alias_subst")]


def device_stream(form, k):
    return B.device_all_stream(k) if form == "all" else B.device_cut_streams(k)[("alias", "alias_nl", "alias_subst").index(form) + 1]


# ------------------------------------------------------------------ the builder's promises
def test_the_values_that_are_no_base():
    assert len(B.NON_BASES) == 248 and len(B.ALIAS) == 24 and set(B.ALIAS) <= set(B.NON_BASES)
    assert int(B.IS_BASE.sum()) == 8 and all(B.IS_BASE[c] for c in b"ACGTacgt")
    assert bytes(v for v in B.ALIAS if 0x20 < v < 0x7F) == b"!#'4"              # the four printable ones are quality characters
    # the 24: the low five bits of a base under other top bits
    assert sorted(B.ALIAS) == sorted(v for v in B.NON_BASES if any((v & 31) == (c & 31) for c in b"ACGT"))


def test_the_k_of_the_device_tests():
    assert B.ALL_KS == [1, 4, 5, 11, 16, 21, 31, 32, 33, 63, 64, 65, 96, 128] and B.MODEL_KS == [31, 65] and B.TEXT_KS == [7, 21, 31]
    assert all(k in B.ALL_KS for k in B.ENUM_KS + B.COUNT_KS + [k for k, _ in B.MINIMIZER_KM])


@pytest.mark.parametrize("form,k", DEVICE_STREAMS)
def test_what_the_builder_promises(form, k):
    s = device_stream(form, k)
    assert s.dtype == np.uint8
    at, vals = B.separators(s)
    lens = np.diff(np.concatenate([[-1], at, [len(s)]])) - 1               # the fragments: before, between and behind the separators
    assert B.IS_BASE[s[0]] and B.IS_BASE[s[-1]] and (lens >= (k + 1) // 2).all() and (lens >= 1).all()      # one byte, a base on both sides
    lanes = {}
    for p, v in zip(at, vals):
        lanes.setdefault(int(v), []).append(int(p) % 4)
    assert sorted(lanes) == B.NON_BASES
    recs = bytes(s).split(b"\n")
    for v in B.NON_BASES:
        if form == "alias_nl" and v == B.NL:
            assert len(lanes[v]) == len(recs) - 1 >= 60
        elif form == "all" or v in B.ALIAS:
            assert sorted(lanes[v]) == [0, 1, 2, 3], (v, lanes[v])
        else:
            assert len(lanes[v]) == 1, (v, lanes[v])
    assert len(at) == {"all": 992, "alias": 320, "alias_subst": 320, "alias_nl": 319 + len(recs) - 1}[form]
    nominal = B.fragment_lengths(k)
    assert set(nominal) <= set(int(n) for n in lens)                         # every nominal length occurs unpadded
    assert (lens <= max(nominal) + 3).all()
    letters = Counter(bytes(s[B.IS_BASE[s]]))
    assert len(letters) == 8                                                 # both cases of all four
    if form == "alias_nl":                                                   # five fragments in every record (the last one may be short)
        assert all(len(B.separators(np.frombuffer(r, dtype=np.uint8))[0]) == 4 for r in recs[:-1])


def test_fragments_cut_from_a_source_are_its_substrings():
    src = B.clean_source(3000, 9)
    text = bytes(src)
    s = B.byte_stream_nl(31, "alias", 4, source=src)
    at, _ = B.separators(s)
    up = B.upper_bases(s).encode("latin-1")
    a = 0
    for b in list(at) + [len(s)]:
        assert up[a: b] in text
        a = int(b) + 1
    assert any(c in bytes(s) for c in b"acgt")


# ------------------------------------------------------------------ the inputs can fail
@pytest.mark.parametrize("form,k", DEVICE_STREAMS)
def test_every_value_taken_for_a_base_changes_the_oracles_answers(oracle, form, k):
    """for each of the 248 values: that value read as 'A' throughout the stream changes the validity of the oracle's enumeration, the total of
    its count and, at the k of the minimizer tests, the validity of its minimizers"""
    s = device_stream(form, k)
    valid = oracle.enumerate_words(s, k)[1]
    total = oracle.count(s, k).total
    assert total == int(valid.sum()) > 0
    ms = [m for kk, m in B.MINIMIZER_KM if kk == k] if form == "all" else []
    mvalid = {m: oracle.minimizers(s, k, m)[1] for m in ms}
    for v in B.NON_BASES:
        t = s.copy()
        t[t == v] = ord("A")
        v2 = oracle.enumerate_words(t, k)[1]
        assert (v2 != valid).any() and oracle.count(t, k).total > total, (form, v)
        if k <= 64:
            assert (oracle.enumerate(t, k)[2] == v2).all()
        for m in ms:
            assert (oracle.minimizers(t, k, m)[1] != mvalid[m]).any(), (v, m)


@pytest.mark.parametrize("k", B.TEXT_KS)
def test_every_value_in_the_file_text(oracle, k):
    """the FASTA and FASTQ texts: which values their lines carry; the two statements of the parsing rules agree on them; a value taken for a
    base changes the count of the records"""
    fa, fq = B.device_text("fa", k), B.device_text("fq", k)
    assert len(fa) < 200_000 and len(fq) < 200_000
    seq = [ln for ln in fa.split(b"\n") if not ln.startswith(b">")]
    assert set(b"".join(seq)) == set(range(256)) - {B.NL} and not any(ln[:1] in (b">", b"@", b"+") for ln in seq if ln)
    lines = fq.split(b"\n")
    assert lines[-1] == b"" and len(lines) % 4 == 1
    assert set(b"".join(lines[1::4])) == set(range(256)) - set(b"\n \t")
    assert set(b"".join(lines[3::4])) == set(range(256)) - set(b"\n\r")
    assert all(len(s.replace(b"\r", b"")) == len(q) for s, q in zip(lines[1::4], lines[3::4]))
    assert all(h[:1] == b"@" for h in lines[0:-1:4]) and all(p == b"+" for p in lines[2::4])
    for text, fmt, fixed in ((fa, "fa", b"\n"), (fq, "fq", b"\n \t\r")):
        host = np.frombuffer(host_records(text, fmt), dtype=np.uint8)
        ref = oracle.count(host, k)
        assert oracle.count(np.frombuffer(model_stream([(text, fmt)]), dtype=np.uint8), k).total == ref.total > 0
        for v in B.NON_BASES:
            if v in fixed or (fmt == "fa" and v in b" \t\r"):                  # (the record separator / not in a line / dropped from it)
                continue
            assert v in host
            changed = host.copy()
            changed[changed == v] = ord("A")
            assert oracle.count(changed, k).total > ref.total, (fmt, v)
    # dropping ' ', '\t' and '\r' joins their neighbours: without them the FASTA text counts the same
    assert oracle.count(np.frombuffer(host_records(fa.translate(None, b" \t\r"), "fa"), dtype=np.uint8), k).total == \
        oracle.count(np.frombuffer(host_records(fa, "fa"), dtype=np.uint8), k).total


# ------------------------------------------------------------------ the table reference, by hand
def test_encode_reference_by_hand():
    packed, inval, mask = B.encode_reference(np.frombuffer(b"ACTGacgt\x01N", dtype=np.uint8))
    assert packed.dtype == np.uint64 and inval.dtype == np.uint32 and len(packed) == len(inval) == len(mask) == 1
    assert int(packed[0]) == 0b00_01_10_11_00_01_11_10 << 48                  # A C T G a c g t
    assert int(inval[0]) == 0xFFFFFFFF >> 8                                   # 0x01, N and the pad read as invalid
    assert int(mask[0]) == 0xFFFF << 48
    s = np.frombuffer(b"G" * 31 + b"\xC7" + b"T" + b"\n" + b"c" * 31, dtype=np.uint8)      # 64 bytes and one more
    packed, inval, mask = B.encode_reference(s)
    assert int(packed[0]) == 0xFFFFFFFFFFFFFFFC and int(inval[0]) == 1 and int(mask[0]) == 0xFFFFFFFFFFFFFFFC
    assert int(packed[1]) == (2 << 62) | int("01" * 30, 2) and int(inval[1]) == 1 << 30 and int(mask[1]) == 0xFFFFFFFFFFFFFFFF ^ (3 << 60)
    assert int(packed[2]) == 1 << 62 and int(inval[2]) == 0x7FFFFFFF and int(mask[2]) == 3 << 62
    for n in (0, 1, 31, 32, 33):
        p, i, m = B.encode_reference(s[:n])
        assert len(p) == len(i) == len(m) == (n + 31) // 32
    big = np.tile(s, 3)                                                      # chunked and whole: the same
    for a, b in zip(B.encode_reference(big, chunk=64), B.encode_reference(big)):
        assert (a == b).all()
    # the table against membership, value by value
    for v in range(256):
        p, i, m = B.encode_reference(np.array([v], dtype=np.uint8))
        assert (int(i[0]) >> 31 == 0) == (v in b"ACGTacgt") == (int(m[0]) != 0)
        if v in b"ACGTacgt":
            assert int(p[0]) >> 62 == "ACTG".index(chr(v).upper())


# ------------------------------------------------------------------ the five string models on bytes that str.upper() moves
def test_upper_bases_keeps_every_byte_in_its_place():
    every = bytes(range(256))
    assert len(every.decode("latin-1").upper()) == 257                       # what the models did before
    up = B.upper_bases(every)
    assert len(up) == 256
    for v in range(256):
        assert up[v] == (chr(v).upper() if v in b"acgt" else chr(v))
    s = B.byte_stream(31, "all", 1)
    ascii_only = bytes(np.where(s < 0x80, s, ord("N")).astype(np.uint8))
    old, new = ascii_only.decode("latin-1").upper(), B.upper_bases(ascii_only)
    run = 0
    for p, c in enumerate(ascii_only):                                       # on text that upper() keeps in place: the same windows
        run = run + 1 if c in b"ACGTacgt" else 0
        if run >= 31:
            assert old[p - 30: p + 1] == new[p - 30: p + 1]


def moved_stream(k):
    """reads of a genome, then fragments of it with 0xDF, 0xB5 and 0xFF between them -> (the reads, the stream, the stream with N there)"""
    src = B.clean_source(400 + 4 * k, 77)
    reads = np.concatenate([src, [B.NL], src[: 200 + 2 * k], [B.NL]]).astype(np.uint8)
    rng = np.random.default_rng(78)
    parts = []
    for i, v in enumerate([0xDF, 0xB5, 0xFF, 0xDF, 0xDF, B.NL, 0xFF, 0xB5, 0xDF]):
        at = int(rng.integers(0, len(src) - 2 * k - 3))
        f = src[at: at + (k + 2 if i % 2 else 2 * k + 3)].copy()
        if i == 4:
            f[k + 1] = ord("ACGT"[("ACGT".index(chr(f[k + 1])) + 1) & 3])     # a substitution in the middle: an interior gap
        if i % 3 == 0:
            f |= 0x20
        parts += [f, np.array([v], dtype=np.uint8)]
    stream = np.concatenate(parts + [src[5: 5 + 2 * k]]).astype(np.uint8)
    plain = stream.copy()
    plain[np.isin(plain, [0xDF, 0xB5, 0xFF])] = ord("N")
    return reads, stream, plain


@pytest.mark.parametrize("k", [15, 31, 65])
def test_the_models_on_bytes_that_upper_moves(oracle, k):
    reads, stream, plain = moved_stream(k)
    values, ab = solid_rows(oracle, reads, k, 1)
    n_valid = oracle.count(stream, k).total
    assert n_valid == oracle.count(plain, k).total > 6 * k
    # the correction
    cr = CorrectRestatement(values, ab, k)
    R, P = cr.correct(stream), cr.correct(plain)
    assert (R.state == P.state).all() and R.stats == P.stats and R.gaps == P.gaps and R.stats["n_valid"] == n_valid
    assert R.stats["n_trusted"] > 0 and R.stats["n_corrected"] >= 1
    moved = np.isin(stream, [0xDF, 0xB5, 0xFF])
    assert (R.out[moved] == stream[moved]).all() and (R.out[~moved] == P.out[~moved]).all()
    # the colours' windows
    w, wp = color_model.windows(stream, k), color_model.windows(plain, k)
    assert w == wp and len(w) == n_valid
    # the read summaries
    table = read_summary_model.table_of(values, ab, k)
    va, aa = read_summary_model.values(bytes(stream), table, k)
    vp, ap = read_summary_model.values(bytes(plain), table, k)
    assert (va == vp).all() and (aa == ap).all() and int(va.sum()) == n_valid and (aa > 0).sum() > 0
    T, st = read_summary_model.summaries(stream, table, k)
    Tp, stp = read_summary_model.summaries(plain, table, k)
    assert (T == Tp).all() and st == stp and st["n_records"] == 2
    assert kmer_counts(bytes(stream), k) == kmer_counts(bytes(plain), k)
    # the threading
    tr = ThreadRestatement(values, ab, k)
    A, Bp = tr.thread(stream), tr.thread(plain)
    tr.check_facts(A)
    assert (A.U == Bp.U).all() and (A.j == Bp.j).all() and A.stats == Bp.stats and A.stats["n_valid"] == n_valid and A.stats["n_placed"] > 0
    assert (A.steps == Bp.steps).all() and (A.edge_support == Bp.edge_support).all()
