"""CPU-side checks of the boundary of the sample colours: the four functions in include/dskgpu.h, in engine.EXPORTS and in the built
library with the documented argument lists, the statistics structure of 64 bytes, the KmerCounter methods, and colors.h beside the twelve
graph headers and readsum.h in one translation unit.  No GPU is needed: nothing is run.

This file fails before the feature: the header declares none of the four names, the library exports none and colors.h does not exist."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from tests.test_graph_headers_compose import CSRC, FLAGS, HEADERS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "dskgpu_colors_begin": "dskgpu_ctx* ctx, uint32_t n_colors",
    "dskgpu_colors_add": "dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, const uint64_t* end_offsets, uint32_t n_banks, uint32_t first_color, "
                         "dskgpu_color_stats* stats",
    "dskgpu_colors_rows": "dskgpu_ctx* ctx, uint32_t min_count, void* d_counts, void* d_mask",
    "dskgpu_colors_unitigs": "dskgpu_ctx* ctx, uint32_t min_count, void* d_sum, void* d_all, void* d_any",
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
    m = re.search(r"typedef struct dskgpu_color_stats\s*\{([^}]*)\}\s*dskgpu_color_stats;", src)
    assert m and " ".join(m.group(1).split()) == "uint64_t n_valid, n_placed, n_rows, n_colors, reserved[4];"


def test_the_header_defines_the_terms():
    text = open(os.path.join(ROOT, "include", "dskgpu.h")).read()
    for term in ("COLOURS", "BANK", "CELL", "MASK", "UNITIG COLOURS", "VARIANT COLOURS", "modulo 2^32", "fewer than 2^32 bytes per colour cannot wrap"):
        assert term in text, term


def test_exports_and_argtypes():
    from dsk_amd import engine
    for name in SIGNATURES:
        assert name in engine.EXPORTS, name
    if not os.path.exists(engine.library_path()):
        import __graft_entry__ as g
        g.build()
    lib = engine.load_library()
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    want = {
        "dskgpu_colors_begin": [vp, u32],
        "dskgpu_colors_add": [vp, vp, u64, C.POINTER(u64), u32, u32, C.POINTER(engine._ColorStats)],
        "dskgpu_colors_rows": [vp, u32, vp, vp],
        "dskgpu_colors_unitigs": [vp, u32, vp, vp, vp],
    }
    for name, argtypes in want.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == argtypes, name
        assert fn.restype is C.c_int, name


def test_the_structure_is_64_bytes():
    from dsk_amd import engine
    assert C.sizeof(engine._ColorStats) == 64
    assert [f[0] for f in engine._ColorStats._fields_] == ["n_valid", "n_placed", "n_rows", "n_colors", "reserved"]
    assert engine._ColorStats.reserved.offset == 32


def test_the_methods_exist():
    from dsk_amd import KmerCounter
    for name in ("colors_begin", "colors_add", "colors_add_tensor", "colors_rows", "colors_rows_tensor", "colors_unitigs", "colors_unitigs_tensor",
                 "variants_colors_tensor"):
        assert callable(getattr(KmerCounter, name)), name


def test_a_null_context_is_an_argument_error():
    """the one error that needs no device: every call checks the context first"""
    from dsk_amd import engine
    if not os.path.exists(engine.library_path()):
        import __graft_entry__ as g
        g.build()
    lib = engine.load_library()
    assert lib.dskgpu_colors_begin(None, 1) == -1
    assert lib.dskgpu_colors_add(None, None, 0, None, 0, 0, None) == -1
    assert lib.dskgpu_colors_rows(None, 1, None, None) == -1
    assert lib.dskgpu_colors_unitigs(None, 1, None, None, None) == -1


def test_fourteen_headers_in_one_translation_unit(tmp_path):
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        pytest.skip("no hipcc")
    headers = HEADERS + ["readsum.h", "colors.h"]
    assert len(headers) == 14 and len(set(headers)) == 14
    for h in headers:
        assert os.path.exists(os.path.join(CSRC, h)), h
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "colors.hip" in re.search(r"^KERNEL_SRCS\s*:=(.*)$", makefile, flags=re.M).group(1).split()
    assert "colors.h" in re.search(r"^HDRS\s*:=(.*)$", makefile, flags=re.M).group(1).split()
    for order in (headers, ["colors.h"] + HEADERS + ["readsum.h"]):
        src = tmp_path / ("all_%s.hip" % order[0].split(".")[0])
        src.write_text("#include <hip/hip_runtime.h>\n" + "".join('#include "%s"\n' % h for h in order))
        out = subprocess.run([hipcc, *FLAGS, "-fsyntax-only", "-I", CSRC, str(src)], capture_output=True, text=True)
        print(out.stdout, out.stderr)
        assert out.returncode == 0, out.stdout + out.stderr
