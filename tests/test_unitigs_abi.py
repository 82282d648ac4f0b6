"""CPU-side checks of the unitig entry points (include/dskgpu.h "the rows' de Bruijn graph compacted into unitigs"): declared in the
header with the documented argument lists, listed in engine.EXPORTS, exported by the built library with the documented argtypes, the
statistics structure of 64 bytes, and reachable from KmerCounter.  No compute calls.  All of it fails before the feature."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dskgpu_unitigs", "dskgpu_unitigs_rows", "dskgpu_unitigs_table", "dskgpu_unitigs_stream"]


def header_text():
    src = open(os.path.join(ROOT, "include", "dskgpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def declared_args(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header_text())
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_the_four_calls():
    assert declared_args("dskgpu_unitigs") == ["dskgpu_ctx* ctx", "dskgpu_unitig_stats* stats"]
    assert declared_args("dskgpu_unitigs_rows") == ["dskgpu_ctx* ctx", "void* d_unitig", "void* d_pos"]
    assert declared_args("dskgpu_unitigs_table") == ["dskgpu_ctx* ctx", "void* d_offsets", "void* d_ab_sum", "void* d_kind"]
    assert declared_args("dskgpu_unitigs_stream") == ["dskgpu_ctx* ctx", "void* d_bytes", "uint64_t capacity"]


def test_header_declares_the_stats_structure():
    m = re.search(r"typedef\s+struct\s+dskgpu_unitig_stats\s*\{([^}]*)\}\s*dskgpu_unitig_stats\s*;", header_text())
    assert m
    assert " ".join(m.group(1).split()) == "uint64_t n_unitigs, n_cycles, n_single, max_nodes, stream_bytes, n_rounds, reserved[2];"


def library():
    from dsk_amd import engine
    if not os.path.exists(engine.library_path()):
        import __graft_entry__ as g
        g.build()
    return engine.load_library()


def test_exports_list_and_library():
    from dsk_amd import engine
    for name in NAMES:
        assert name in engine.EXPORTS, name
    lib = library()
    for name in NAMES:
        assert getattr(lib, name).restype is C.c_int, name
    assert lib.dskgpu_unitigs.argtypes == [C.c_void_p, C.POINTER(engine._UnitigStats)]
    assert lib.dskgpu_unitigs_rows.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.dskgpu_unitigs_table.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.dskgpu_unitigs_stream.argtypes == [C.c_void_p, C.c_void_p, C.c_uint64]


def test_stats_structure_is_64_bytes():
    from dsk_amd import engine
    assert C.sizeof(engine._UnitigStats) == 64
    assert [n for n, _ in engine._UnitigStats._fields_] == ["n_unitigs", "n_cycles", "n_single", "max_nodes", "stream_bytes", "n_rounds", "reserved"]


def test_null_context_is_an_argument_error():
    """The calls that need no device: a null context is refused before anything is touched."""
    lib = library()
    assert lib.dskgpu_unitigs(None, None) == -1
    assert lib.dskgpu_unitigs_rows(None, None, None) == -1
    assert lib.dskgpu_unitigs_table(None, None, None, None) == -1
    assert lib.dskgpu_unitigs_stream(None, None, 0) == -1


def test_kmer_counter_has_the_methods():
    from dsk_amd.engine import KmerCounter
    for name in ("unitigs", "unitigs_rows", "unitigs_table", "unitigs_stream",
                 "unitigs_rows_tensor", "unitigs_table_tensor", "unitigs_stream_tensor"):
        assert callable(getattr(KmerCounter, name, None)), name
