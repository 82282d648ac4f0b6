"""The bubbles of the compacted de Bruijn graph reported as variants on the device (include/dskgpu.h: dskgpu_variants / _variants_table /
_variants_stream; csrc/variants.h).

All comparisons are exact.  Tests 1 to 5 compare the device with the restatement of tests/test_variants_restatement.py, made of the rows as
the context returns them: the records, the stats, the line offsets and the variant stream.  Test 6 needs no oracle and no restatement:
identities on a medium-sized count.  All of it fails before the feature: KmerCounter has no variants().
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from tests import test_gpu_unitig_edges as edges_mod      # noqa: E402
from tests import test_gpu_unitigs as unitigs_mod      # noqa: E402
from tests.test_bubbles_restatement import BUBBLES_PINNED, BUBBLES_STREAM_K, bubbles_stream      # noqa: E402
from tests.test_gpu_unitigs import code_of, count, row_values, stream_of      # noqa: E402
from tests.test_variants_restatement import (COMPLEX, INDEL, MULTI, SNP, VARIANTS_PINNED, check_bubbles_stream, check_popped_bubbles_stream,      # noqa: E402
                                             check_variants_stream, restate, variants_stream)

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
ZERO = dict(n_variants=0, n_snps=0, n_multi=0, n_indels=0, n_complex=0, n_unitigs=0, stream_bytes=0, max_letters=0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda:0")


_streams, _done = {}, {}


def made_stream(which, k):
    if (which, k) not in _streams:
        _streams[(which, k)] = (bubbles_stream if which == "bubbles" else variants_stream)(k)[0]
    return _streams[(which, k)]


def restated(key, kc, k, max_nodes, max_diff=4):
    """the restatement of the rows of kc, cached per (input, k, abundance_min, row order, parameters) and never changed"""
    if key not in _done:
        kk, ab = kc.rows()
        _done[key] = restate(row_values(kk), ab, k, max_nodes, max_diff)
    return _done[key]


def device_variants(kc):
    rec = kc.variants_tensor()
    off, text = kc.variants_stream_tensor()
    assert rec.dtype == torch.int64 and off.dtype == torch.int64 and text.dtype == torch.uint8
    return rec.cpu().numpy(), off.cpu().numpy(), text.cpu().numpy()


def check_variants(kc, exp, max_nodes, max_diff=4):
    """one call on the device against the restatement of the same rows: stats, records, offsets, stream"""
    st = kc.variants(max_nodes, max_diff)
    print("variant stats", st, "expected", exp.variant_stats)
    rec, off, text = device_variants(kc)
    assert rec.shape == exp.records.shape, (rec.shape, exp.records.shape)
    bad = np.nonzero((rec != exp.records).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), bad[:4], rec[bad[:4]], exp.records[bad[:4]])
    assert len(off) == len(exp.v_offsets) and (off == exp.v_offsets).all()
    assert len(text) == len(exp.v_stream) and (text == exp.v_stream).all()
    assert st == exp.variant_stats
    return st


# ------------------------------------------------------------------ 1. the golden reads after clip_tips()
@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k,amin", [(31, 2), (63, 2), (16, 2)])
def test_golden_reads_match_the_restatement(oracle, golden_dir, dev, k, amin, partition_order):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, k, abundance_min=amin, partition_order=partition_order) as kc:
        kc.clip_tips()
        kk, ab = kc.rows()
        assert len(kk) == BUBBLES_PINNED[(k, amin)][0][0]
        exp = restated(("golden", k, amin, partition_order), kc, k, 2 * k)
        s0 = kc.stats(); u0 = unitigs_mod.device_answer(kc); e0 = edges_mod.device_edges(kc)
        st = check_variants(kc, exp, 2 * k)
        assert st["n_variants"] == VARIANTS_PINNED[(k, amin)][0] == st["n_snps"]      # the row order changes the numbering, never the counts
        assert st["n_unitigs"] == kc.graph_bubbles(2 * k)["n_in_bubbles"]
        assert kc.variants() == st                                           # the defaults: max_nodes = 2 k, max_diff = 4
        # the call changed nothing: rows, stats, unitigs and edges
        k2, a2 = kc.rows()
        assert (k2 == kk).all() and (a2 == ab).all() and kc.stats() == s0
        for before, after in zip(u0 + e0, unitigs_mod.device_answer(kc) + edges_mod.device_edges(kc)):
            assert (before == after) if isinstance(before, dict) else (before == after).all()


# ------------------------------------------------------------------ 2. the bubbles stream, before and after a round of pops
@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k", BUBBLES_STREAM_K)
def test_bubbles_stream(dev, k, partition_order):
    with count(made_stream("bubbles", k), dev, k, abundance_min=1, partition_order=partition_order) as kc:
        exp4 = restated(("bubbles", k, partition_order, 4), kc, k, 2 * k, 4)
        exp6 = restated(("bubbles", k, partition_order, 6), kc, k, 2 * k, 6)
        check_bubbles_stream(exp4, exp6, k)
        check_variants(kc, exp6, 2 * k, 6)
        st = check_variants(kc, exp4, 2 * k, 4)                              # the next call replaces what the last one kept
        assert (st["n_variants"], st["n_snps"], st["n_unitigs"]) == (7, 7, 11)
        total = kc.pop_bubbles(2 * k, 4, max_rounds=1)
        assert total["n_popped"] == 5
        buf = torch.zeros(64, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        assert code_of(lambda: kc.variants_table(buf.data_ptr())) == E_STATE      # the pop dropped the kept variants
        assert code_of(lambda: kc.variants_stream(buf.data_ptr(), 0)) == E_STATE
        after = restated(("bubbles popped", k, partition_order), kc, k, 2 * k, 4)
        check_popped_bubbles_stream(after, k)
        st = check_variants(kc, after, 2 * k, 4)
        assert st["n_multi"] == 1


# ------------------------------------------------------------------ 3. the other kinds, texts of more than 64 and more than 256 letters
@pytest.mark.parametrize("partition_order", [False, True])
@pytest.mark.parametrize("k", BUBBLES_STREAM_K)
def test_variants_stream(dev, k, partition_order):
    with count(made_stream("variants", k), dev, k, abundance_min=1, partition_order=partition_order) as kc:
        exp = restated(("variants", k, partition_order), kc, k, 2 * k, 4)
        check_variants_stream(exp, k)
        st = check_variants(kc, exp, 2 * k, 4)
        rec = kc.variants_tensor().cpu().numpy()
        assert sorted(rec[:, 7].tolist()) == [MULTI, INDEL, INDEL, COMPLEX]
        off = kc.variants_stream_tensor()[0].cpu().numpy()
        run = [int(r[5]) for i, r in enumerate(rec) if r[7] == INDEL and abs(int(off[2 * i + 2] - off[2 * i + 1]) - int(off[2 * i + 1] - off[2 * i])) == 1]
        assert run == [k - 1 - 5]                                            # the capped lcs
        assert st["max_letters"] == 2 * k + 2 and (k < 33 or st["max_letters"] > 64) and (k < 128 or st["max_letters"] > 256)


# ------------------------------------------------------------------ 4. writes stay inside their arrays; the NULL rules
def test_writes_stay_inside_their_arrays(dev):
    k = 33
    with count(made_stream("variants", k), dev, k, abundance_min=1) as kc:
        exp = restated(("variants", k, False), kc, k, 2 * k, 4)
        st = kc.variants(2 * k)
        n, nb = st["n_variants"], st["stream_bytes"]
        assert n == 4 and nb == len(exp.v_stream)
        r = torch.full((8 + 8 * n + 8,), -7, dtype=torch.int32, device=dev)
        o = torch.full((4 + 2 * n + 1 + 4,), -7, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        kc.variants_table(r.data_ptr() + 32)
        assert (r[:8] == -7).all() and (r[8 + 8 * n:] == -7).all() and (r[8: 8 + 8 * n].cpu().numpy().reshape(n, 8) == exp.records).all()
        for shift in (0, 3):
            b = torch.full((64 + shift + nb + 64,), 249, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            kc.variants_stream(o.data_ptr() + 32, b.data_ptr() + 64 + shift, nb + 5)      # a larger capacity writes no more
            res = b.cpu().numpy()
            assert (res[: 64 + shift] == 249).all() and (res[64 + shift + nb:] == 249).all(), "variants_stream wrote outside its stream_bytes"
            assert (res[64 + shift: 64 + shift + nb] == exp.v_stream).all()
        assert (o[:4] == -7).all() and (o[4 + 2 * n + 1:] == -7).all() and (o[4: 4 + 2 * n + 1].cpu().numpy() == exp.v_offsets).all()
        # a capacity too small: DSKGPU_E_ARG and nothing written, the offsets neither
        b = torch.full((nb + 64,), 249, dtype=torch.uint8, device=dev)
        o2 = torch.full((2 * n + 1,), -7, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        for cap in (0, nb - 1):
            assert code_of(lambda: kc.variants_stream(o2.data_ptr(), b.data_ptr(), cap)) == E_ARG
        assert (b == 249).all() and (o2 == -7).all()
        # the NULL rules: either output alone, both NULL refused, a NULL table refused
        assert kc._lib.dskgpu_variants_stream(kc._h, None, None, nb) == E_ARG
        assert kc._lib.dskgpu_variants_table(kc._h, None) == E_ARG
        kc.variants_stream(o2.data_ptr(), 0, 0)
        assert (o2.cpu().numpy() == exp.v_offsets).all()
        kc.variants_stream(0, b.data_ptr(), nb)
        assert (b[:nb].cpu().numpy() == exp.v_stream).all() and (b[nb:] == 249).all()
        assert kc._lib.dskgpu_variants(kc._h, C.byref(_params(2 * k)), None) == 0      # stats may be NULL
        assert kc.variants(2 * k) == st


def _params(max_nodes, max_diff=4):
    from dsk_amd.engine import _VariantParams
    return _VariantParams(max_nodes=max_nodes, max_diff=max_diff)


# ------------------------------------------------------------------ 5. states and errors
def test_states_and_errors(oracle, golden_dir, dev):
    from dsk_amd import KmerCounter
    from dsk_amd.engine import _VariantStats
    k = 31
    buf = torch.zeros(4096, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    p = buf.data_ptr()
    with KmerCounter(kmer_size=k) as kc:
        for call in (kc.variants, lambda: kc.variants_table(p), lambda: kc.variants_stream(p, 0)):
            assert code_of(call) == E_STATE                                  # before any count
    with count(made_stream("bubbles", k), dev, k, abundance_min=1) as kc:
        n = kc.result_device()[2]
        for call in (lambda: kc.variants_table(p), lambda: kc.variants_stream(p, 0), kc.variants_tensor, kc.variants_stream_tensor):
            assert code_of(call) == E_STATE                                  # a copy call before variants()
        for mn in (0, 65536):
            assert code_of(lambda: kc.variants(mn)) == E_ARG
        assert kc._lib.dskgpu_variants(kc._h, None, C.byref(_VariantStats())) == E_ARG
        assert kc.result_device()[2] == n
        # a kept threading survives variants()
        reads = torch.from_numpy(made_stream("bubbles", k)).to(dev)
        t0 = kc.thread_reads_tensor(reads)
        w0 = [t.cpu().numpy() for t in kc.thread_walks_tensor()]
        st = kc.variants()
        assert st["n_variants"] == 7
        assert all((a == b).all() for a, b in zip(w0, (t.cpu().numpy() for t in kc.thread_walks_tensor())))
        assert t0["n_walks"] > 0 and kc.variants_tensor().shape == (7, 8)
        # a new count drops the kept variants ...
        kc.count()
        assert code_of(lambda: kc.variants_table(p)) == E_STATE and code_of(kc.variants_stream_tensor) == E_STATE
        # ... and so does filter_rows
        assert kc.variants()["n_variants"] == 7
        keep = torch.ones(n, dtype=torch.uint8, device=dev)
        keep[0] = 0
        assert kc.filter_rows_tensor(keep) == n - 1
        assert code_of(lambda: kc.variants_table(p)) == E_STATE and code_of(lambda: kc.variants_stream(p, 0)) == E_STATE
        assert kc.variants()["n_variants"] <= 7                              # and the next call serves the rows left


def test_a_result_without_rows_and_a_result_without_variants(oracle, golden_dir, dev):
    stream = stream_of("golden", oracle, golden_dir)
    with count(stream, dev, 31, abundance_min=10 ** 6) as kc:
        assert kc.stats()["n_solid"] == 0
        assert kc.variants() == ZERO
        o = torch.full((8,), -7, dtype=torch.int64, device=dev)
        b = torch.full((8,), 249, dtype=torch.uint8, device=dev)
        r = torch.full((8,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        kc.variants_stream(o.data_ptr(), b.data_ptr(), 8)
        kc.variants_table(r.data_ptr())
        assert int(o[0]) == 0 and (o[1:] == -7).all() and (b == 249).all() and (r == -7).all()
        assert kc.variants_tensor().shape == (0, 8) and kc.variants_stream_tensor()[1].numel() == 0
    with count(stream, dev, 63, abundance_min=2) as kc:                       # rows, and no bubble among them
        kc.clip_tips()
        assert kc.result_device()[2] > 0 and kc.variants() == ZERO
        o = torch.full((8,), -7, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        kc.variants_stream(o.data_ptr(), 0, 0)
        assert int(o[0]) == 0 and (o[1:] == -7).all()


def test_a_rank_of_a_group_is_a_state_error(oracle, golden_dir, dev):
    from dsk_amd import KmerGroup
    s = stream_of("golden", oracle, golden_dir)
    recs = bytes(s).split(b"\n")
    with KmerGroup([0, 0], kmer_size=31, abundance_min=2) as g:
        for r in range(2):
            g.rank(r).push_reads(b"\n".join(recs[r::2]) + b"\n")
        g.count()
        kc = g.rank(0)
        n = kc.stats()["n_solid"]
        assert n > 0
        assert code_of(kc.variants) == E_STATE
        assert "world_size" in kc._lib.dskgpu_last_error(kc._h).decode()
        assert kc.result_device()[2] == n


# ------------------------------------------------------------------ 6. identities, no oracle, medium size
@pytest.fixture(scope="module")
def reads100k(dev):
    from dsk_amd import synth
    return synth.make_reads(synth.make_genome(300_000, dev), 100_000, 150)


def test_identities_on_the_reads(reads100k, dev):
    from dsk_amd import KmerCounter
    k = 31
    with KmerCounter(kmer_size=k, abundance_min=2) as kc:
        kc.set_reads_device(reads100k.data_ptr(), reads100k.numel())
        kc.count()
        assert kc.result_device()[2] > 100_000
        st = kc.variants()
        print("variant stats", st)
        rec, off, text = device_variants(kc)
        n = st["n_variants"]
        assert n > 0 and rec.shape == (n, 8) and st["n_snps"] + st["n_multi"] + st["n_indels"] + st["n_complex"] == n
        assert st["n_unitigs"] == kc.graph_bubbles(2 * k)["n_in_bubbles"] and st["stream_bytes"] == len(text) == int(off[-1])
        a, b = rec[:, 0] >> 1, rec[:, 1] >> 1
        assert (rec[:, 0] & 1 == 0).all() and (a < b).all()
        pairs = a * (1 << 32) + b
        assert (np.diff(pairs) > 0).all()                                    # ascending (a, b), each pair once
        # the stream counts back to the rows of the flagged unitigs, each as often as its unitig has variants
        nu = kc.unitigs()["n_unitigs"]
        per_unitig = np.bincount(np.concatenate([a, b]), minlength=nu)
        assert int((per_unitig > 0).sum()) == st["n_unitigs"]
        unitig = kc.unitigs_rows_tensor()[0].cpu().numpy()
        kk, _ = kc.rows()
        times = per_unitig[unitig]
        want = sorted(zip(kk[times > 0, 0].tolist(), times[times > 0].tolist()))
        stream = kc.variants_stream_tensor()[1]
        with KmerCounter(kmer_size=k, abundance_min=1) as again:
            again.set_reads_device(stream.data_ptr(), stream.numel())
            again.count()
            k2, a2 = again.rows()
            assert sorted(zip(k2[:, 0].tolist(), a2.tolist())) == want
        # lcp, lcs, n_mismatch and kind again, with numpy, from the stream's own lines
        nodes = np.diff(kc.unitigs_table_tensor()[0].cpu().numpy()) - k
        for i in range(n):
            ta, tb = text[off[2 * i]: off[2 * i + 1] - 1], text[off[2 * i + 1]: off[2 * i + 2] - 1]
            assert text[off[2 * i + 1] - 1] == 10 and text[off[2 * i + 2] - 1] == 10
            assert len(ta) == k + nodes[a[i]] - 1 and len(tb) == k + nodes[b[i]] - 1
            m = min(len(ta), len(tb))
            front, back = np.nonzero(ta[:m] != tb[:m])[0], np.nonzero(ta[::-1][:m] != tb[::-1][:m])[0]
            lcp = int(front[0]) if len(front) else m
            lcs = min(int(back[0]) if len(back) else m, m - lcp)
            if len(ta) == len(tb):
                nm = int((ta != tb).sum())
                kind = SNP if nm == 1 else MULTI
            else:
                nm, kind = 0, (INDEL if lcp + lcs == m else COMPLEX)
            assert rec[i, 4:].tolist() == [lcp, lcs, nm, kind], (i, rec[i])
        assert st["max_letters"] == int(np.diff(off).max()) - 1
        kinds = np.bincount(rec[:, 7], minlength=5)
        assert (st["n_snps"], st["n_multi"], st["n_indels"], st["n_complex"]) == tuple(int(x) for x in kinds[1:5])


# ------------------------------------------------------------------ 7. the FASTA file; the stage time
def test_write_variants_round_trip(dev, tmp_path):
    from dsk_amd.engine import VARIANT_KINDS
    k = 33
    with count(made_stream("variants", k), dev, k, abundance_min=1, timing=True) as kc:
        assert "variants" not in dict(kc.stage_times())
        st = kc.variants()
        times = dict(kc.stage_times())
        assert times["variants"] > 0 and times["unitig edges"] > 0
        out = kc.write_variants(str(tmp_path / "variants.fa"))
        assert out == {name: st[name] for name in ("n_variants", "n_snps", "n_multi", "n_indels", "n_complex")}
        rec, off, text = device_variants(kc)
        offsets, ab_sum, _ = (t.cpu().numpy() for t in kc.unitigs_table_tensor())
        lines = open(str(tmp_path / "variants.fa")).read().split("\n")
        assert lines[-1] == "" and len(lines) == 4 * st["n_variants"] + 1
        gfa = lambda U: "%d%s" % (U >> 1, "-" if U & 1 else "+")      # noqa: E731
        for i, r in enumerate(rec.tolist()):
            for j, side in enumerate("ab"):
                head, seq = lines[4 * i + 2 * j], lines[4 * i + 2 * j + 1]
                U = r[j]
                name, *fields = head.split(" ")
                assert name == ">v%d|%s|%s|%s" % (i, side, VARIANT_KINDS[r[7]], gfa(U))
                assert dict(f.split("=") for f in fields) == {"from": gfa(r[2]), "to": gfa(r[3]), "L": str(int(offsets[(U >> 1) + 1] - offsets[U >> 1]) - k),
                                                              "S": str(int(ab_sum[U >> 1])), "lcp": str(r[4]), "lcs": str(r[5]), "n_mismatch": str(r[6])}
                assert seq.encode() == text[off[2 * i + j]: off[2 * i + j + 1] - 1].tobytes()
        kc.variants()
        assert dict(kc.stage_times())["variants"] > times["variants"]
