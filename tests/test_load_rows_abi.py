"""CPU-side checks of the boundary of the row load: dskgpu_load_rows in include/dskgpu.h, in engine.EXPORTS and in the built library with
the documented argument list, the structure of 64 bytes, the four combine rules and the KmerCounter methods.  No GPU is needed: nothing is run.

This file fails before the feature: the header does not declare the name and the library does not export it."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURE = "dskgpu_ctx* ctx, const void* d_kmers, const void* d_abundance, uint64_t n, uint32_t combine, dskgpu_load_stats* stats"
FIELDS = ["n_in", "n_distinct", "n_rows", "n_below", "n_above", "n_kmers", "n_saturated", "sorted_input"]
DEFINES = {"DSKGPU_LOAD_SUM": 0, "DSKGPU_LOAD_MAX": 1, "DSKGPU_LOAD_MIN": 2, "DSKGPU_LOAD_UNIQUE": 3}


def header():
    src = open(os.path.join(ROOT, "include", "dskgpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def library():
    from dsk_amd import engine
    if not os.path.exists(engine.library_path()):
        import __graft_entry__ as g
        g.build()
    return engine.load_library()


def test_the_header_declares_the_function_the_structure_and_the_rules():
    src = header()
    m = re.search(r"\bint\s+dskgpu_load_rows\s*\(([^)]*)\)\s*;", src)
    assert m and " ".join(m.group(1).split()) == SIGNATURE
    m = re.search(r"typedef struct dskgpu_load_stats\s*\{([^}]*)\}\s*dskgpu_load_stats;", src)
    assert m and " ".join(m.group(1).split()) == "uint64_t " + ", ".join(FIELDS) + ";"
    for name, value in DEFINES.items():
        assert re.search(r"^#define %s\s+%du\b" % (name, value), src, flags=re.M), name


def test_the_section_stands_after_the_colours_and_before_the_group():
    src = header()
    assert src.index("dskgpu_colors_marks(") < src.index("DSKGPU_LOAD_SUM") < src.index("dskgpu_load_rows(") < src.index("dskgpu_group_create(")


def test_the_header_defines_the_terms():
    text = open(os.path.join(ROOT, "include", "dskgpu.h")).read()
    for term in ("A LOAD IS A COUNT WHOSE INPUT IS (k-mer, abundance) PAIRS INSTEAD OF READS", "row-major, least-significant word first", "8-byte aligned",
                 "4-byte aligned", "must NOT be memory the context owns", "n <= 2^32 - 2", "value <= revcomp(value)", "A=0 C=1 T=2 G=3", "palindromes",
                 "LOWEST offending input index", "the previous result and everything built on it are untouched", "saturated at 2^32 - 1",
                 "ignores DSKGPU_F_PARTITION_ORDER", "the load REPLACES the count's record", "the exact 64-bit sum of the INPUT abundances",
                 "the 2-D histogram is forgotten", "world_size > 1", '"load check", "load order", "load combine"'):
        assert term in text, term


def test_exports_and_argtypes():
    from dsk_amd import engine
    assert "dskgpu_load_rows" in engine.EXPORTS
    fn = library().dskgpu_load_rows
    assert list(fn.argtypes) == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(engine._LoadStats)]
    assert fn.restype is C.c_int
    assert engine.LOAD_COMBINE == {"sum": 0, "max": 1, "min": 2, "unique": 3}


def test_the_structure_is_64_bytes():
    from dsk_amd import engine
    assert C.sizeof(engine._LoadStats) == 64
    assert [(name, getattr(engine._LoadStats, name).offset) for name, _ in engine._LoadStats._fields_] == [(f, 8 * i) for i, f in enumerate(FIELDS)]


def test_the_methods_exist():
    import dsk_amd
    from dsk_amd import KmerCounter
    for name in ("load_rows", "load_rows_tensor", "load_rows_numpy", "save_rows", "load_saved", "load_ascii"):
        assert callable(getattr(KmerCounter, name)), name
    assert callable(dsk_amd.parse_ascii_rows) and dsk_amd.parse_ascii_rows is dsk_amd.engine.parse_ascii_rows


def test_a_null_context_is_an_argument_error():
    """the one error that needs no device: the call checks the context first"""
    assert library().dskgpu_load_rows(None, None, None, 0, 0, None) == -1
