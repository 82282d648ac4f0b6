"""CPU-side checks of the boundary of the sample comparison: dskgpu_colors_pairs / _colors_load / _colors_marks in include/dskgpu.h, in
engine.EXPORTS and in the built library with the documented argument lists, the three structures of 64 / 32 / 64 bytes, the KmerCounter
methods and sample_distances.  No GPU is needed: nothing is run.

This file fails before the feature: the header declares none of the three names and the library exports none."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "dskgpu_colors_pairs": "dskgpu_ctx* ctx, uint32_t min_count, const void* d_select, void* d_shared, void* d_cross, void* d_min_sum, "
                           "dskgpu_color_pair_stats* stats",
    "dskgpu_colors_load": "dskgpu_ctx* ctx, const void* d_counts, uint32_t n_colors",
    "dskgpu_colors_marks": "dskgpu_ctx* ctx, const dskgpu_color_rule* rule, void* d_keep, dskgpu_color_mark_stats* stats",
}
STRUCTS = {
    "dskgpu_color_pair_stats": "uint64_t n_rows, n_selected, n_present, n_colors, reserved[4];",
    "dskgpu_color_rule": "uint64_t need_all, need_none; uint32_t min_count, min_present, max_present, flags;",
    "dskgpu_color_mark_stats": "uint64_t n_rows, n_kept, reserved[6];",
}


def header():
    src = open(os.path.join(ROOT, "include", "dskgpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def library():
    from dsk_amd import engine
    if not os.path.exists(engine.library_path()):
        import __graft_entry__ as g
        g.build()
    return engine.load_library()


def test_the_header_declares_the_three_functions_and_the_structures():
    src = header()
    for name, args in SIGNATURES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, name
        assert " ".join(m.group(1).split()) == args, name
    for name, body in STRUCTS.items():
        m = re.search(r"typedef struct %s\s*\{([^}]*)\}\s*%s;" % (name, name), src)
        assert m and " ".join(m.group(1).split()) == body, name
    assert re.search(r"^#define DSKGPU_COLORS_INVERT 1u\b", src, flags=re.M)
    assert src.index("dskgpu_colors_unitigs(") < src.index("dskgpu_colors_pairs(") < src.index("dskgpu_group_create(")


def test_the_header_defines_the_terms():
    text = open(os.path.join(ROOT, "include", "dskgpu.h")).read()
    for term in ("THRESHOLDED CELL", "shared[i][j]", "cross[i][j]", "min_sum[i][j]", "min_sum[i][i] == cross[i][i]", "element-wise sums of the ranks' matrices",
                 '"color pairs", "color marks", "color load"'):
        assert term in text, term


def test_exports_and_argtypes():
    from dsk_amd import engine
    for name in SIGNATURES:
        assert name in engine.EXPORTS, name
    lib = library()
    vp, u32 = C.c_void_p, C.c_uint32
    want = {
        "dskgpu_colors_pairs": [vp, u32, vp, vp, vp, vp, C.POINTER(engine._ColorPairStats)],
        "dskgpu_colors_load": [vp, vp, u32],
        "dskgpu_colors_marks": [vp, C.POINTER(engine._ColorRule), vp, C.POINTER(engine._ColorMarkStats)],
    }
    for name, argtypes in want.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == argtypes, name
        assert fn.restype is C.c_int, name


def test_the_structures_are_64_32_and_64_bytes():
    from dsk_amd import engine

    def layout(s):
        return [(name, getattr(s, name).offset) for name, _ in s._fields_]

    assert C.sizeof(engine._ColorPairStats) == 64
    assert layout(engine._ColorPairStats) == [("n_rows", 0), ("n_selected", 8), ("n_present", 16), ("n_colors", 24), ("reserved", 32)]
    assert C.sizeof(engine._ColorRule) == 32
    assert layout(engine._ColorRule) == [("need_all", 0), ("need_none", 8), ("min_count", 16), ("min_present", 20), ("max_present", 24), ("flags", 28)]
    assert C.sizeof(engine._ColorMarkStats) == 64
    assert layout(engine._ColorMarkStats) == [("n_rows", 0), ("n_kept", 8), ("reserved", 16)]
    assert engine.COLORS_INVERT == 1


def test_the_methods_exist():
    import dsk_amd
    from dsk_amd import KmerCounter
    for name in ("colors_load", "colors_load_tensor", "colors_pairs", "colors_pairs_tensor", "colors_marks", "colors_marks_tensor"):
        assert callable(getattr(KmerCounter, name)), name
    assert callable(dsk_amd.sample_distances)


def test_a_null_context_is_an_argument_error():
    """the one error that needs no device: every call checks the context first"""
    lib = library()
    assert lib.dskgpu_colors_pairs(None, 1, None, None, None, None, None) == -1
    assert lib.dskgpu_colors_load(None, None, 1) == -1
    assert lib.dskgpu_colors_marks(None, None, None, None) == -1
