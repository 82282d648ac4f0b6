"""The per-read summaries, the rule and the selection (include/dskgpu.h: "per-read abundance summaries and read selection"), restated in
plain Python / numpy from the definitions.  Not a test module: tests/test_read_summary_restatement.py checks it on the CPU before
tests/test_gpu_read_summaries.py trusts it on the device.  It shares no code with the engine: the dtype below is its own copy, the k-mers are
STRINGS in the lexicographic canonical form of the correction's restatement (tests/test_correct_restatement.py: _BASES, canon), and the
table is a dict canonical string -> abundance of which only lookups are asked."""
import numpy as np

from tests.byte_streams import upper_bases
from tests.test_correct_restatement import _BASES, canon

FIELDS = ("start", "sum", "len", "n_valid", "n_solid", "median")
SUMMARY_DTYPE = np.dtype([("start", "<u8"), ("sum", "<u8"), ("len", "<u4"), ("n_valid", "<u4"), ("n_solid", "<u4"), ("median", "<u4")])
STATS = ("n_records", "n_empty", "n_valid", "n_solid", "max_len")
MARK_STATS = ("n_records", "n_kept", "kept_bytes", "kept_valid")
NL = 0x0A


def value_to_string(value, k):
    """the k letters of a k-mer value: two bits per base, A C T G = 0 1 2 3, the first base in the highest bits"""
    return "".join("ACTG"[(value >> (2 * (k - 1 - i))) & 3] for i in range(k))


def table_of(values, ab, k):
    """canonical k-mer VALUES (Python ints) and their abundances -> the dict the model looks up"""
    t = {canon(value_to_string(int(v), k)): int(a) for v, a in zip(values, ab)}
    assert len(t) == len(values)
    return t


def records(raw):
    """-> [(start, len)] of the records of the stream"""
    out, start = [], 0
    for p in np.flatnonzero(np.frombuffer(raw, dtype=np.uint8) == NL):
        out.append((start, int(p) - start))
        start = int(p) + 1
    if len(raw) > 0 and raw[-1] != NL:
        out.append((start, len(raw) - start))
    return out


def values(raw, table, k):
    """-> (valid bool[n], a int64[n]): the window ending at every byte"""
    n = len(raw)
    text = upper_bases(raw)
    valid, a = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64)
    run = 0
    for p in range(n):
        run = run + 1 if raw[p] in _BASES else 0
        if run >= k:
            valid[p] = True
            a[p] = table.get(canon(text[p - k + 1: p + 1]), 0)
    return valid, a


def summaries(stream, table, k, trust_min=0):
    """-> (the table of summaries, SUMMARY_DTYPE; the stats)"""
    raw = bytes(stream)
    valid, a = values(raw, table, k)
    recs = records(raw)
    out = np.zeros(len(recs), dtype=SUMMARY_DTYPE)
    tmin = max(trust_min, 1)
    for i, (start, ln) in enumerate(recs):
        assert ln <= 0xFFFFFFFF
        v = sorted(int(x) for x in a[start: start + ln][valid[start: start + ln]])
        out[i] = (start, sum(v), ln, len(v), sum(1 for x in v if x >= tmin), v[len(v) // 2] if v else 0)
    st = dict(n_records=len(recs), n_empty=int((out["n_valid"] == 0).sum()), n_valid=int(out["n_valid"].sum()), n_solid=int(out["n_solid"].sum()),
              max_len=max((r[1] for r in recs), default=0))
    return out, st


def marks(table, rule=None):
    """rule: dict of min_valid, median_min, median_max, solid_num, solid_den, invert (all optional); None keeps everything -> uint8[n_records]"""
    rule = rule or {}
    keep = np.zeros(len(table), dtype=np.uint8)
    for i, s in enumerate(table):
        nv, ns, med = int(s["n_valid"]), int(s["n_solid"]), int(s["median"])
        kp = nv >= rule.get("min_valid", 0) and med >= rule.get("median_min", 0)
        kp = kp and (rule.get("median_max", 0) == 0 or med <= rule["median_max"])
        kp = kp and (rule.get("solid_den", 0) == 0 or ns * rule["solid_den"] >= rule.get("solid_num", 0) * nv)
        keep[i] = 1 if kp != bool(rule.get("invert", False)) else 0
    return keep


def mark_stats(table, keep):
    k = keep != 0
    return dict(n_records=len(table), n_kept=int(k.sum()), kept_bytes=int((table["len"][k].astype(np.int64) + 1).sum()), kept_valid=int(table["n_valid"][k].sum()))


def select(stream, keep):
    """-> uint8 array: the kept records in stream order, one newline behind each"""
    raw = bytes(stream)
    recs = records(raw)
    assert len(recs) == len(keep)
    out = b"".join(raw[s: s + n] + b"\n" for (s, n), kp in zip(recs, keep) if kp)
    return np.frombuffer(out, dtype=np.uint8).copy()
