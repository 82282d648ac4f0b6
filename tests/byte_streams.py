"""Every byte value as input: streams whose separators run over all 248 values that are no base, and the table reference of the encoded
stream.  Not a test module: tests/test_byte_streams_restatement.py checks what is promised here on the CPU before
tests/test_gpu_byte_values.py feeds the streams to the device.

"Is a base" is membership in the eight letters ACGTacgt and nothing else, here as in the oracle's g_code table and the models' _BASES.
Nothing in this file restates the device's arithmetic on the bits of a byte."""
import numpy as np

BASES = b"ACGTacgt"
IS_BASE = np.zeros(256, dtype=bool)
IS_BASE[list(BASES)] = True
NON_BASES = [v for v in range(256) if v not in BASES]
# the values that share their low five bits with a base but not their top two: what a wrong mask lets through as A, C, G or T
ALIAS = [0x01, 0x03, 0x07, 0x14, 0x21, 0x23, 0x27, 0x34, 0x81, 0x83, 0x87, 0x94,
         0xA1, 0xA3, 0xA7, 0xB4, 0xC1, 0xC3, 0xC7, 0xD4, 0xE1, 0xE3, 0xE7, 0xF4]
NL = 0x0A

_UPPER = bytes.maketrans(b"acgt", b"ACGT")
_LETTERS = np.frombuffer(BASES, dtype=np.uint8)


def upper_bases(raw):
    """the bytes as a string of the same length: acgt upper-cased, every other value as it is (str.upper() makes two letters of 0xDF)"""
    return bytes(raw).translate(_UPPER).decode("latin-1")


def fragment_lengths(k):
    return [max(1, n) for n in ((k + 1) // 2, k - 1, k, k + 1, 2 * k + 3)]


def clean_source(n, seed):
    """n random upper-case bases: what the fragments of a stream are cut from when the rows of a count are to be found in it"""
    return np.random.default_rng(seed).choice(np.frombuffer(b"ACGT", dtype=np.uint8), n)


def _plan(lanes):
    """-> [(separator value, None or the list of stream positions mod 4 still wanted for it)] in stream order"""
    if lanes == "all":
        return [(v, [0, 1, 2, 3]) for v in NON_BASES]
    assert lanes == "alias"
    return [(v, [0, 1, 2, 3] if v in ALIAS else None) for v in NON_BASES]


def _build(k, lanes, seed, source, newline_every):
    rng = np.random.default_rng(seed)
    lens = fragment_lengths(k)
    out, pos, nfrag = [], 0, 0

    def fragment(n):
        nonlocal pos, nfrag
        if source is None:
            f = rng.choice(_LETTERS, n)
        else:
            at = int(rng.integers(0, len(source) - n + 1))
            f = source[at: at + n] | (rng.integers(0, 2, n, dtype=np.uint8) << 5)      # (mixed case)
        out.append(f.astype(np.uint8))
        pos += n
        nfrag += 1

    def separator(v):
        nonlocal pos
        out.append(np.array([v], dtype=np.uint8))
        pos += 1

    def next_length():
        return lens[nfrag % len(lens)]

    for v, want in _plan(lanes):
        if newline_every and v == NL:                                             # (the records' own separator)
            continue
        for _ in range(1 if want is None else len(want)):
            if newline_every and nfrag % newline_every == newline_every - 1:      # this fragment is the last of its record
                fragment(next_length())
                separator(NL)
            n = next_length()
            pad = 0
            if want is not None:                                                  # the lane still wanted that costs the fewest extra bases
                pad = min((lane - (pos + n)) % 4 for lane in want)
                want.remove((pos + n + pad) % 4)
            fragment(n + pad)
            separator(v)
    fragment(next_length())                                                       # the stream ends inside a fragment
    return np.concatenate(out)


def byte_stream(k, lanes="all", seed=0, source=None):
    """Fragments of random ACGTacgt (or of `source`, in mixed case) with exactly one byte that is no base between two of them; the nominal
    lengths cycle over (k + 1) // 2, k - 1, k, k + 1, 2 k + 3 (never below 1).  lanes = "all": each of the 248 values at every stream
    position mod 4; "alias": each value once and the 24 of ALIAS at every position mod 4.  A separator is steered to its position by
    lengthening the fragment before it.  The stream begins with a fragment and ends inside one."""
    return _build(k, lanes, seed, source, 0)


def byte_stream_nl(k, lanes="alias", seed=0, source=None):
    """byte_stream with a newline behind every fifth fragment: records of five fragments for the entries that split at '\\n'"""
    return _build(k, lanes, seed, source, 5)


def separators(stream):
    """-> (positions, values) of the bytes that are no base"""
    at = np.flatnonzero(~IS_BASE[stream])
    return at, stream[at]


def with_substitutions(stream, k):
    """-> (a copy with one base substituted, its case kept, in every fragment of 2 k + 3 letters and more: the first, the one at offset
    k + 1 or the last in turn; how many): something for a correction to do in a stream cut from the counted reads"""
    s = stream.copy()
    at, _ = separators(s)
    bounds = np.concatenate([[-1], at, [len(s)]])
    n = 0
    for a, b in zip(bounds[:-1], bounds[1:]):
        if b - a - 1 >= 2 * k + 3:
            p = int(a) + 1 + (0, k + 1, int(b - a) - 2)[n % 3]
            s[p] = b"ACGT"[(b"ACGT".index(s[p] & 0xDF) + 1) & 3] | (s[p] & 0x20)
            n += 1
    return s, n


# ------------------------------------------------------------------ the streams the device tests feed
# Built here and nowhere else: tests/test_byte_streams_restatement.py counts the promises and shows the sensitivity on these very bytes.
ENUM_KS = [1, 4, 31, 32, 33, 64, 65, 128]                                  # dskgpu_k_enumerate
MINIMIZER_KM = [(31, 10), (21, 8), (63, 10), (11, 4), (16, 16), (5, 1)]     # dskgpu_k_minimizers: the pairs of test_gpu_parity.py
COUNT_KS = [31, 63, 96]                                                    # the count
MODEL_KS = [31, 65]                                                        # the entries with string models
TEXT_KS = [7, 21, 31]                                                      # file text (7: the short text that is pushed byte by byte)
ALL_KS = sorted(set(ENUM_KS + [k for k, _ in MINIMIZER_KM] + COUNT_KS))      # every k at which an "all" stream goes to the device
_device_all, _device_cut, _device_text = {}, {}, {}


def device_all_stream(k):
    """the "all" stream of k (computed once, shared, never changed)"""
    if k not in _device_all:
        _device_all[k] = byte_stream(k, "all", 100 + k)
    return _device_all[k]


def device_cut_streams(k):
    """-> (the clean reads to count: a genome of 3000 bases and its first half again; the "alias" stream and the record stream, both cut from
    the genome; the "alias" stream with substitutions)"""
    if k not in _device_cut:
        src = clean_source(3000, 40 + k)
        counted = np.concatenate([src, [NL], src[:1500], [NL]]).astype(np.uint8)
        alias = byte_stream(k, "alias", 50 + k, source=src)
        _device_cut[k] = (counted, alias, byte_stream_nl(k, "alias", 60 + k, source=src), with_substitutions(alias, k)[0])
    return _device_cut[k]


def device_text(fmt, k):
    """the FASTA ("fa") or FASTQ ("fq") text of k"""
    if (fmt, k) not in _device_text:
        _device_text[(fmt, k)] = (fasta_text if fmt == "fa" else fastq_text)(k, 5)
    return _device_text[(fmt, k)]


# ------------------------------------------------------------------ the encoded stream, from a table
_CODE = np.zeros(256, dtype=np.uint64)
for _letters, _c in ((b"Aa", 0), (b"Cc", 1), (b"Tt", 2), (b"Gg", 3)):
    _CODE[list(_letters)] = _c
_SHIFT = (62 - 2 * np.arange(32)).astype(np.uint64)
_BIT = (31 - np.arange(32)).astype(np.uint32)


def encode_reference(stream, chunk=1 << 22):
    """-> (packed u64[(n + 31) // 32], inval u32[(n + 31) // 32], valid_mask u64[...]).  Base j of word w is byte 32 w + j; its code (A C T G =
    0 1 2 3) sits in bits 63 - 2 j .. 62 - 2 j of packed[w]; bit 31 - j of inval[w] is set iff that byte is no base or lies at or beyond n.
    The code bits under an invalid position are no part of the contract: valid_mask has both bits of every VALID position set, and packed is
    to be compared under it (the reference leaves 0 there)."""
    stream = np.ascontiguousarray(stream, dtype=np.uint8)
    n = len(stream)
    nw = (n + 31) // 32
    packed, inval, mask = np.zeros(nw, dtype=np.uint64), np.zeros(nw, dtype=np.uint32), np.zeros(nw, dtype=np.uint64)
    assert chunk % 32 == 0
    for a in range(0, n, chunk):
        part = stream[a: a + chunk]
        w = (len(part) + 31) // 32
        valid = np.zeros(32 * w, dtype=bool)
        valid[: len(part)] = IS_BASE[part]
        code = np.zeros(32 * w, dtype=np.uint64)
        code[: len(part)] = _CODE[part]
        code[~valid] = 0
        valid = valid.reshape(w, 32)
        sl = slice(a // 32, a // 32 + w)
        packed[sl] = np.bitwise_or.reduce(code.reshape(w, 32) << _SHIFT, axis=1)
        mask[sl] = np.bitwise_or.reduce((valid.astype(np.uint64) * np.uint64(3)) << _SHIFT, axis=1)
        inval[sl] = np.bitwise_or.reduce((~valid).astype(np.uint32) << _BIT, axis=1)
    return packed, inval, mask


# ------------------------------------------------------------------ file text with every byte value
def _line_values(exclude):
    return [v for v in range(256) if v not in exclude]


def _lines(k, seed, values, n_lines):
    """sequence lines: fragments of random bases with one byte of `values` between them, every value at least once over the lines, no line
    beginning with '>', '@' or '+' (a line begins with a fragment)"""
    rng = np.random.default_rng(seed)
    lens = fragment_lengths(k)
    per = -(-len(values) // n_lines)
    lines, nfrag = [], 0
    for i in range(n_lines):
        line = bytearray()
        for v in values[i * per: (i + 1) * per]:
            line += rng.choice(_LETTERS, lens[nfrag % len(lens)]).tobytes() + bytes([v])
            nfrag += 1
        line += rng.choice(_LETTERS, lens[nfrag % len(lens)]).tobytes()
        nfrag += 1
        lines.append(bytes(line))
    return lines


def fasta_text(k, seed=0, n_lines=12):
    """FASTA text whose sequence lines carry every value except '\\n': three lines per record, so that wrapped lines join.  ' ', '\\t' and
    '\\r' inside a line are dropped and their neighbours join; one line per kind has an ALIAS byte on both sides of such a byte."""
    rng = np.random.default_rng(seed + 1)
    lines = _lines(k, seed, _line_values(b"\n"), n_lines)
    for blank in b" \t\r":
        lines.append(rng.choice(_LETTERS, k).tobytes() + bytes([0x21, blank, 0xE7]) + rng.choice(_LETTERS, k).tobytes()
                     + bytes([0x94, blank]) + rng.choice(_LETTERS, k // 2).tobytes() + bytes([blank]) + rng.choice(_LETTERS, k - k // 2).tobytes())
    out = bytearray()
    for i, ln in enumerate(lines):
        if i % 3 == 0:
            out += b">record %d\n" % (i // 3)
        out += ln + b"\n"
    return bytes(out)


def fastq_text(k, seed=0, n_records=12):
    """FASTQ text: the sequence lines carry every value except '\\n', ' ' and '\\t' ('\\r' is dropped from them), the quality lines every
    value except '\\n' and '\\r', as many characters as their sequence line has without its '\\r'"""
    lines = _lines(k, seed, _line_values(b"\n \t"), n_records)
    quals = _line_values(b"\n\r")
    out, q = bytearray(), 0
    for i, ln in enumerate(lines):
        n = len(ln.replace(b"\r", b""))
        qual = bytes(quals[(q + j) % len(quals)] for j in range(n))
        q += n
        out += b"@read %d\n" % i + ln + b"\n+\n" + qual + b"\n"
    return bytes(out)
