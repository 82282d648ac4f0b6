"""CPU-side checks of the boundary of the per-read summaries and the read selection: the four functions in include/dskgpu.h, in
engine.EXPORTS and in the built library with the documented argument lists, the sizes of the four structures and of a summary, the
KmerCounter methods, and readsum.h beside the twelve other graph headers in one translation unit.  No GPU is needed: nothing is run."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from tests.test_graph_headers_compose import CSRC, FLAGS, HEADERS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "dskgpu_read_summaries": "dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, const dskgpu_read_summary_params* params, dskgpu_read_summary_stats* stats",
    "dskgpu_read_summaries_table": "dskgpu_ctx* ctx, void* d_records",
    "dskgpu_read_marks": "dskgpu_ctx* ctx, const dskgpu_read_rule* rule, void* d_keep, dskgpu_read_mark_stats* stats",
    "dskgpu_select_reads": "dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, const void* d_keep, uint64_t n_records, void* d_out, uint64_t capacity, "
                           "uint64_t* out_bytes, uint64_t* out_records",
}


def header():
    src = open(os.path.join(ROOT, "include", "dskgpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_the_header_declares_the_four_functions():
    src = header()
    for name, args in SIGNATURES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, name
        assert " ".join(m.group(1).split()) == args, name
    assert re.search(r"#define\s+DSKGPU_READS_INVERT\s+1u", src)
    for struct, fields in (("dskgpu_read_summary_params", "uint32_t trust_min, flags; uint64_t reserved[3];"),
                           ("dskgpu_read_summary_stats", "uint64_t n_records, n_empty, n_valid, n_solid, max_len, reserved[3];"),
                           ("dskgpu_read_rule", "uint32_t min_valid, median_min, median_max, solid_num, solid_den, flags; uint64_t reserved;"),
                           ("dskgpu_read_mark_stats", "uint64_t n_records, n_kept, kept_bytes, kept_valid, reserved[4];")):
        m = re.search(r"typedef struct %s\s*\{([^}]*)\}\s*%s;" % (struct, struct), src)
        assert m, struct
        assert " ".join(m.group(1).split()) == fields, struct


def test_exports_and_argtypes():
    from dsk_amd import engine
    for name in SIGNATURES:
        assert name in engine.EXPORTS, name
    if not os.path.exists(engine.library_path()):
        import __graft_entry__ as g
        g.build()
    lib = engine.load_library()
    vp, u64 = C.c_void_p, C.c_uint64
    want = {
        "dskgpu_read_summaries": [vp, vp, u64, C.POINTER(engine._ReadSummaryParams), C.POINTER(engine._ReadSummaryStats)],
        "dskgpu_read_summaries_table": [vp, vp],
        "dskgpu_read_marks": [vp, C.POINTER(engine._ReadRule), vp, C.POINTER(engine._ReadMarkStats)],
        "dskgpu_select_reads": [vp, vp, u64, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)],
    }
    for name, argtypes in want.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == argtypes, name
        assert fn.restype is C.c_int, name


def test_structure_sizes_and_the_summary_dtype():
    from dsk_amd import engine
    assert [C.sizeof(s) for s in (engine._ReadSummaryParams, engine._ReadSummaryStats, engine._ReadRule, engine._ReadMarkStats)] == [32, 64, 32, 64]
    assert [f[0] for f in engine._ReadSummaryStats._fields_] == ["n_records", "n_empty", "n_valid", "n_solid", "max_len", "reserved"]
    assert [f[0] for f in engine._ReadMarkStats._fields_] == ["n_records", "n_kept", "kept_bytes", "kept_valid", "reserved"]
    assert [f[0] for f in engine._ReadRule._fields_] == ["min_valid", "median_min", "median_max", "solid_num", "solid_den", "flags", "reserved"]
    assert engine._ReadRule.flags.offset == 20 and engine._ReadRule.reserved.offset == 24 and engine._ReadSummaryParams.reserved.offset == 8
    d = engine.READ_SUMMARY_DTYPE
    assert d.itemsize == 32 and d.names == ("start", "sum", "len", "n_valid", "n_solid", "median")
    assert [d.fields[n][1] for n in d.names] == [0, 8, 16, 20, 24, 28]
    assert [d.fields[n][0].itemsize for n in d.names] == [8, 8, 4, 4, 4, 4] and all(d.fields[n][0].kind == "u" for n in d.names)
    assert engine.READS_INVERT == 1
    from tests.read_summary_model import SUMMARY_DTYPE
    assert SUMMARY_DTYPE == d                                                # the model's own copy says the same


def test_the_methods_exist():
    from dsk_amd import KmerCounter
    for name in ("read_summaries", "read_summaries_table", "read_summaries_numpy", "read_marks", "select_reads", "select_reads_tensor"):
        assert callable(getattr(KmerCounter, name)), name


def test_thirteen_headers_in_one_translation_unit(tmp_path):
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        pytest.skip("no hipcc")
    headers = HEADERS + ["readsum.h"]
    assert len(headers) == 13 and len(set(headers)) == 13
    for h in headers:
        assert os.path.exists(os.path.join(CSRC, h)), h
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "readsum.hip" in re.search(r"^KERNEL_SRCS\s*:=(.*)$", makefile, flags=re.M).group(1)
    assert "readsum.h" in re.search(r"^HDRS\s*:=(.*)$", makefile, flags=re.M).group(1).split()
    assert re.search(r"^#define RS_WAVE_CAP \d+", open(os.path.join(CSRC, "readsum.h")).read(), flags=re.M)
    for order in (headers, ["readsum.h"] + HEADERS):
        src = tmp_path / ("all_%s.hip" % order[0].split(".")[0])
        src.write_text("#include <hip/hip_runtime.h>\n" + "".join('#include "%s"\n' % h for h in order))
        out = subprocess.run([hipcc, *FLAGS, "-fsyntax-only", "-I", CSRC, str(src)], capture_output=True, text=True)
        print(out.stdout, out.stderr)
        assert out.returncode == 0, out.stdout + out.stderr
