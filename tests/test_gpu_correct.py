"""Substitution errors in reads corrected against the count on the device (include/dskgpu.h: dskgpu_correct_reads; csrc/correct.h).

All comparisons are exact.  Part 1 compares the device -- output bytes, states and stats -- with the string restatement of
tests/test_correct_restatement.py (which the CPU suite checks first) and the default trial kernel with the staged pair in a fresh child
process.  Part 2 is geometry: the smallest shapes at which the frame, the packed state stores, the gap walk and the block sums can go wrong.
Part 3 is the contract of the arguments, part 4 the consequence for a recount, part 5 lifetime and errors.

Every test here fails before the feature: KmerCounter has no correct_reads and the library no dskgpu_correct_reads.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests.test_correct_restatement import CORRECT_PINNED, KS, STATS, CorrectRestatement, check_handmade, handmade_correct, planted_stream      # noqa: E402
from tests.test_gpu_unitigs import code_of, count, row_values, stream_of      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_STATE = -1, -4
ZERO = dict.fromkeys(STATS, 0)
GUARD, FILL = 64, 0xEE


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


# ------------------------------------------------------------------ the streams and the expectation (computed once, shared, never changed)
def streams(kind, k, golden=None):
    """-> (the stream to count, the stream to correct)"""
    if kind == "planted":
        s = planted_stream(k)[0]
        return s, s
    if kind == "hand":
        counted, s, _ = handmade_correct(k)
        return counted, s
    return golden, golden


_expected = {}


def expected(kc, kind, stream, k, amin, tmin):
    """what the restatement built from the rows of kc gives for the stream; cached per trusted set (kind, k, threshold)"""
    kk, ab = kc.rows()
    exp = CorrectRestatement(row_values(kk), ab, k, tmin)
    key = (kind, k, max(amin, tmin, 1))
    if key not in _expected:
        _expected[key] = (exp.trusted, exp.correct(stream))
    assert _expected[key][0] == exp.trusted
    return _expected[key][1]


def run(kc, dev, stream, trust_min=0, offs=(0, 0, 0), mode="out", want_state=True):
    """one call with guard bytes round both outputs.  offs: the offsets of d_bytes, d_out and d_state from their allocations.  mode: out
    of place, "inplace", or "dry" (d_out NULL).  -> (output bytes or None, states or None, stats)"""
    n = len(stream)
    oi, oo, os_ = offs
    src = torch.full((n + oi + GUARD,), 10, dtype=torch.uint8, device=dev)
    src[oi: oi + n] = torch.from_numpy(stream).to(dev)
    out = torch.full((n + oo + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    st = torch.full((n + os_ + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p_in = src.data_ptr() + oi
    assert src.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and st.data_ptr() % 16 == 0
    d_out = {"out": out.data_ptr() + GUARD + oo, "inplace": p_in, "dry": 0}[mode]
    stats = kc.correct_reads(p_in, n, d_out, st.data_ptr() + GUARD + os_ if want_state else 0, trust_min)
    torch.cuda.synchronize()
    for buf, o, used in ((out, oo, mode == "out"), (st, os_, want_state)):
        b = buf.cpu().numpy()
        assert (b[: GUARD + o] == FILL).all() and (b[GUARD + o + n:] == FILL).all(), "guard bytes"
        if not used:
            assert (b == FILL).all()
    got_in = src[oi: oi + n].cpu().numpy()
    assert (src[:oi] == 10).all() and (src[oi + n:] == 10).all()
    if mode == "inplace":
        res = got_in
    else:
        assert (got_in == stream).all(), "the input is left as it was"
        res = out[GUARD + oo: GUARD + oo + n].cpu().numpy() if mode == "out" else None
    return res, st[GUARD + os_: GUARD + os_ + n].cpu().numpy() if want_state else None, stats


def same(got, R):
    out, state, stats = got
    print("correct stats", stats, "expected", R.stats)
    assert stats == R.stats
    bad = np.nonzero(state != R.state)[0]
    assert len(bad) == 0, ("states", len(bad), bad[:5], state[bad[:5]], R.state[bad[:5]])
    bad = np.nonzero(out != R.out)[0]
    assert len(bad) == 0, ("bytes", len(bad), bad[:5], out[bad[:5]], R.out[bad[:5]])


def digest(got):
    out, state, stats = got
    return [hashlib.sha1(out.tobytes()).hexdigest(), hashlib.sha1(state.tobytes()).hexdigest(), [stats[n] for n in STATS]]


# ------------------------------------------------------------------ 1. the string restatement, every key width and boundary
PARITY = [("planted", k) for k in KS] + [("golden", k) for k in KS] + [("hand", k) for k in [1, 4] + KS]
_digests = {}


def parity_case(dev, kind, k, amin, order, golden, check=True):
    counted, stream = streams(kind, k, golden)
    with count(counted, dev, k, abundance_min=amin, partition_order=order) as kc:
        for tmin in (0, 3):
            got = run(kc, dev, stream, tmin)
            _digests["%s:%d:%d:%d:%d" % (kind, k, amin, int(order), tmin)] = digest(got)
            if not check:
                continue
            R = expected(kc, kind, stream, k, amin, tmin)
            same(got, R)
            if max(amin, tmin) == 3 and (kind, k) in CORRECT_PINNED and kind != "hand":
                assert R.summary() == CORRECT_PINNED[(kind, k)]
            if kind == "hand":
                assert R.summary() == CORRECT_PINNED[(kind, k)]
                if k >= 15:
                    check_handmade(k, stream, handmade_correct(k)[2], R)
            if kind == "planted" and max(amin, tmin) == 3:
                assert (got[0] == planted_stream(k)[1]).all() and got[2]["n_corrected"] == got[2]["n_gaps"] == planted_stream(k)[2]
            if kind != "hand" and max(amin, tmin) == 1:                      # every k-mer of the stream is a row: no gap at all
                assert got[2]["n_gaps"] == 0 and got[2]["n_trusted"] == got[2]["n_valid"] and (got[0] == stream).all()


@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("amin", [1, 3])
@pytest.mark.parametrize("kind,k", PARITY)
def test_device_equals_the_restatement(oracle, golden_dir, dev, kind, k, amin, partition_order):
    """output bytes, states and stats, trust_min 0 and 3, on the planted stream, the handmade stream and the golden reads"""
    parity_case(dev, kind, k, amin, partition_order, stream_of("golden", oracle, golden_dir) if kind == "golden" else None)


def child_main(golden_path):
    """the parity runs again, without the restatement -> one JSON line of digests (run by test_the_other_trial_kernels... in a fresh process)"""
    golden = np.load(golden_path)
    d = torch.device("cuda:0")
    for kind, k in PARITY:
        for amin in (1, 3):
            for order in (False, True):
                parity_case(d, kind, k, amin, order, golden, check=False)
    print("DIGESTS " + json.dumps(_digests, sort_keys=True))


def test_the_other_trial_kernels_in_a_fresh_process_give_the_same(oracle, golden_dir, dev, tmp_path):
    """DSKGPU_CORRECT_STAGED (read when a context is created): the staged pair of trial kernels instead of the default, one thread per
    candidate and 3 x m windows in sequence -- identical bytes, states and stats on every parity run.  (The plain kernel measured faster and is the default, so the
    switch selects the other one.)"""
    golden = stream_of("golden", oracle, golden_dir)
    for kind, k in PARITY:
        for amin in (1, 3):
            for order in (False, True):
                if "%s:%d:%d:%d:0" % (kind, k, amin, int(order)) not in _digests:
                    parity_case(dev, kind, k, amin, order, golden, check=False)
    mine = json.loads(json.dumps(_digests, sort_keys=True))
    path = str(tmp_path / "golden.npy")
    np.save(path, golden)
    code = "import sys; sys.path.insert(0, %r); from tests.test_gpu_correct import child_main; child_main(%r)" % (ROOT, path)
    env = dict(os.environ, DSKGPU_CORRECT_STAGED="1")
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    line = [ln for ln in r.stdout.decode().split("\n") if ln.startswith("DIGESTS ")]
    assert len(line) == 1
    theirs = json.loads(line[0][len("DIGESTS "):])
    assert len(theirs) == len(PARITY) * 8 and theirs.keys() == mine.keys()
    assert [key for key in mine if mine[key] != theirs[key]] == []


# ------------------------------------------------------------------ 2. geometry
@pytest.mark.parametrize("j", [0, 1, 7, 31, 33])
@pytest.mark.parametrize("k", [31, 64, 97])
def test_separators_in_front_shift_the_corrections(dev, j, k):
    """j separator bytes in front of the handmade stream: the same corrections, shifted by j (the frame's words and the 16-position loads of the gap kernel start elsewhere).  Fails before the feature: no correct_reads."""
    counted, stream, _ = handmade_correct(k)
    shifted = np.concatenate([np.full(j, ord("\n"), dtype=np.uint8), stream])
    with count(counted, dev, k, abundance_min=1) as kc:
        R = expected(kc, "hand", stream, k, 1, 0)
        out, state, stats = run(kc, dev, shifted)
        assert (out[:j] == ord("\n")).all() and (state[:j] == 0).all()
        same((out[j:], state[j:], stats), R)


@pytest.mark.parametrize("k,block", [(31, 32), (63, 32), (127, 32), (31, 4096), (63, 2048), (127, 1024), (63, 4096), (127, 4096)])
def test_a_gap_across_a_boundary(dev, k, block):
    """a multiple of 32 positions (one packed word); 256 x N positions, one block of the state kernel (N = 16, 8, 4 for the three key
    widths); 4096 positions, one block of the gap kernel.  nbytes is no multiple of 32."""
    stream = planted_stream(k)[0]
    with count(stream, dev, k, abundance_min=3) as kc:
        R = expected(kc, "planted", stream, k, 3, 0)
        g = next(g for g in R.gaps if g[1] - g[0] + 1 == k and g[0] > block)
        pad = (block - (g[0] + k // 2) % block) % block                      # newlines in front: the middle of the gap on a multiple of `block`
        assert (g[0] + pad) // block < (g[1] + pad) // block, "the gap straddles the boundary"
        s = np.concatenate([np.full(pad, ord("\n"), dtype=np.uint8), stream])
        if len(s) % 32 == 0:
            s = np.concatenate([s, np.full(1, ord("\n"), dtype=np.uint8)])
        assert len(s) % 32 != 0
        out, state, stats = run(kc, dev, s)
        n = len(stream)
        same((out[pad: pad + n], state[pad: pad + n], stats), R)
        assert (out[:pad] == ord("\n")).all() and (state[:pad] == 0).all() and (out[pad + n:] == ord("\n")).all() and (state[pad + n:] == 0).all()


@pytest.mark.parametrize("offs", [(1, 5, 0), (5, 0, 1), (0, 1, 5), (1, 1, 1)])
@pytest.mark.parametrize("k", [31, 64, 128])
def test_pointers_at_odd_addresses(dev, k, offs):
    """d_bytes, d_out and d_state at offsets 0, 1 and 5 from their allocations; guard bytes before and after each output"""
    counted, stream, _ = handmade_correct(k)
    assert len(stream) % 32 != 0
    with count(counted, dev, k, abundance_min=1) as kc:
        R = expected(kc, "hand", stream, k, 1, 0)
        same(run(kc, dev, stream, 0, offs), R)
        out, _, stats = run(kc, dev, stream, 0, offs, mode="inplace")
        assert (out == R.out).all() and stats == R.stats


# ------------------------------------------------------------------ 3. the contract of the arguments
@pytest.mark.parametrize("kind,k", [("hand", 33), ("planted", 31), ("planted", 96)])
def test_in_place_dry_run_state_alone_and_idempotence(dev, kind, k):
    """In place equals out of place; the dry run gives the same stats and states and writes nothing; d_state alone; the input is unchanged out of place; a second application corrects nothing.  Fails before the feature: no correct_reads."""
    counted, stream = streams(kind, k)
    amin = 1 if kind == "hand" else 3
    with count(counted, dev, k, abundance_min=amin) as kc:
        R = expected(kc, kind, stream, k, amin, 0)
        assert R.stats["n_corrected"] > 0
        same(run(kc, dev, stream), R)                                        # (run checks that the input is unchanged)
        out, state, stats = run(kc, dev, stream, mode="inplace")
        assert (out == R.out).all() and (state == R.state).all() and stats == R.stats
        out, state, stats = run(kc, dev, stream, mode="dry")                 # statistics and states only
        assert out is None and (state == R.state).all() and stats == R.stats
        out, state, stats = run(kc, dev, stream, mode="dry", want_state=False)
        assert out is None and state is None and stats == R.stats
        out, state, stats = run(kc, dev, stream, want_state=False)
        assert (out == R.out).all() and state is None and stats == R.stats
        # one application is final
        out2, state2, stats2 = run(kc, dev, R.out)
        assert (out2 == R.out).all() and stats2["n_corrected"] == 0
        for name in ("n_ambiguous", "n_unfixable", "n_skipped", "n_valid"):
            assert stats2[name] == R.stats[name], name
        for a, b, _, _, outcome, _ in R.gaps:
            if outcome == "corrected":
                assert (state2[a: b + 1] == 2).all()
        o, st = kc.correct_reads_tensor(torch.from_numpy(stream).to(dev))
        assert (o.cpu().numpy() == R.out).all() and st == R.stats
        o, st, s = kc.correct_reads_tensor(torch.from_numpy(stream).to(dev), trust_min=3, want_state=True)
        assert o.dtype == torch.uint8 and s.dtype == torch.uint8 and (s.cpu().numpy() == R.state).all() and (o.cpu().numpy() == R.out).all()


# ------------------------------------------------------------------ 4. the consequence
@pytest.mark.parametrize("k", [31, 64])
def test_the_corrected_stream_counts_back_to_the_error_free_rows(dev, k):
    """Counting the corrected planted stream with abundance_min 1 gives exactly the rows of the error-free stream.  Fails before the feature: no correct_reads."""
    stream, truth, plants = planted_stream(k)
    with count(stream, dev, k, abundance_min=3) as kc:
        out, st = kc.correct_reads_tensor(kc._reads_keepalive)
        assert st["n_corrected"] == plants
    with count(out.cpu().numpy(), dev, k, abundance_min=1) as a, count(truth, dev, k, abundance_min=1) as b, count(stream, dev, k, abundance_min=1) as c:
        ka, aa = a.rows()
        kb, ab = b.rows()
        assert ka.shape == kb.shape and (ka == kb).all() and (aa == ab).all()
        assert c.stats()["n_solid"] > a.stats()["n_solid"]


# ------------------------------------------------------------------ 5. lifetime and errors
def test_the_context_is_left_as_it_was(oracle, golden_dir, dev):
    """rows, stats and histogram before and after; and the call after simplify() agrees with the restatement of the rows left"""
    k = 31
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, k, abundance_min=3) as kc:
        k1, a1 = kc.rows(); h1 = kc.histogram(); s1 = kc.stats()
        R = expected(kc, "golden", stream, k, 3, 0)
        same(run(kc, dev, stream), R)
        k2, a2 = kc.rows()
        assert (k1 == k2).all() and (a1 == a2).all() and (kc.histogram() == h1).all() and kc.stats() == s1
        sst = kc.simplify()
        assert 0 < sst["n_rows_left"] < len(a1)
        kk, ab = kc.rows()
        after = CorrectRestatement(row_values(kk), ab, k)
        assert after.trusted < _expected[("golden", k, 3)][0]
        Ra = after.correct(stream)
        same(run(kc, dev, stream), Ra)
        assert Ra.stats["n_trusted"] < R.stats["n_trusted"]


def test_before_any_count_is_a_state_error(dev):
    """No result: DSKGPU_E_STATE, also for an empty stream.  Fails before the feature: no correct_reads."""
    from dsk_amd import KmerCounter
    buf = torch.zeros(1024, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p = buf.data_ptr()
    with KmerCounter(kmer_size=31) as kc:
        for call in (lambda: kc.correct_reads(p, 64, p), lambda: kc.correct_reads(p, 64), lambda: kc.correct_reads(0, 0)):
            assert code_of(call) == E_STATE


def test_bad_arguments_and_an_empty_stream(dev):
    """Null d_bytes, non-zero flags or reserved words, a stream longer than one launch takes: DSKGPU_E_ARG, nothing written; NULL params / d_out / d_state / stats are allowed; nbytes == 0 succeeds with all-zero stats.  Fails before the feature: no correct_reads."""
    from dsk_amd import engine
    import ctypes as C
    k = 33
    counted, stream, _ = handmade_correct(k)
    with count(counted, dev, k, abundance_min=1) as kc:
        R = expected(kc, "hand", stream, k, 1, 0)
        t = torch.from_numpy(stream).to(dev)
        out = torch.full((len(stream),), FILL, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        lib, h, p, n = kc._lib, kc._h, t.data_ptr(), t.numel()
        st = engine._CorrectStats()
        assert lib.dskgpu_correct_reads(h, None, n, None, out.data_ptr(), None, C.byref(st)) == E_ARG
        for par in (engine._CorrectParams(flags=1), engine._CorrectParams(reserved=(0, 0, 1)), engine._CorrectParams(trust_min=3, reserved=(1, 0, 0))):
            assert lib.dskgpu_correct_reads(h, p, n, C.byref(par), out.data_ptr(), None, C.byref(st)) == E_ARG
        assert lib.dskgpu_correct_reads(h, p, (0x7FFFFFFF << 11) + 1, None, None, None, None) == E_ARG
        torch.cuda.synchronize()
        assert (out == FILL).all()
        assert lib.dskgpu_correct_reads(h, p, n, None, None, None, None) == 0        # params, d_out, d_state and stats may all be NULL
        assert lib.dskgpu_correct_reads(h, p, n, None, out.data_ptr(), None, C.byref(st)) == 0      # NULL params: the defaults
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == R.out).all() and {name: int(getattr(st, name)) for name in STATS} == R.stats
        st = engine._CorrectStats(n_valid=7, n_gaps=7)
        assert lib.dskgpu_correct_reads(h, None, 0, None, None, None, C.byref(st)) == 0 and {name: int(getattr(st, name)) for name in STATS} == ZERO
        assert kc.correct_reads(0, 0) == ZERO
        same(run(kc, dev, stream), R)                                        # and the context still answers


def test_a_result_without_rows(oracle, golden_dir, dev):
    """Every valid window is state 1, every read one skipped gap, nothing is corrected.  Fails before the feature: no correct_reads."""
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31, abundance_min=10 ** 6) as kc:
        assert kc.stats()["n_solid"] == 0
        out, state, st = run(kc, dev, stream)
        assert (out == stream).all() and int((state == 1).sum()) == st["n_valid"] == kc.stats()["n_kmers"] == 350000 and not (state == 2).any()
        assert st == dict(ZERO, n_valid=350000, n_gaps=5000, n_skipped=5000)


def test_a_rank_of_a_group_is_a_state_error(oracle, golden_dir, dev):
    """world_size > 1: DSKGPU_E_STATE, and the text names world_size.  Fails before the feature: no correct_reads."""
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
        assert kc.stats()["n_solid"] > 0
        assert code_of(lambda: kc.correct_reads(p, 64, p)) == E_STATE
        assert "world_size" in kc._lib.dskgpu_last_error(kc._h).decode()


def test_stage_times_name_the_correction(oracle, golden_dir, dev):
    """The three stage marks, and "query index" for the index built on first use.  Fails before the feature: no correct_reads."""
    stream = stream_of("golden", oracle, golden_dir)
    names = ("correct states", "correct gaps", "correct trials")
    with count(stream, dev, 31, abundance_min=3, timing=True) as kc:
        before = dict(kc.stage_times())
        assert not any(n in before for n in names + ("query index",))
        kc.correct_reads_tensor(kc._reads_keepalive)
        after = dict(kc.stage_times())
        assert all(after[n] > 0 for n in names) and after["query index"] > 0
        assert all(after[n] == v for n, v in before.items())
