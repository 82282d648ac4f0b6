"""CPU-side checks of the de Bruijn neighbourhood entry points (include/dskgpu.h "the rows' de Bruijn neighbours"): declared in the
header with the documented argument lists, listed in engine.EXPORTS, exported by the built library, and reachable from KmerCounter.
No compute calls."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dskgpu_graph_adjacency", "dskgpu_graph_neighbors"]


def header_text():
    src = open(os.path.join(ROOT, "include", "dskgpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def declared_args(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header_text())
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_both_calls():
    assert declared_args("dskgpu_graph_adjacency") == ["dskgpu_ctx* ctx", "void* d_adj", "uint64_t* degrees"]
    assert declared_args("dskgpu_graph_neighbors") == ["dskgpu_ctx* ctx", "const void* d_kmers", "uint64_t n", "void* d_adj"]


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
    assert lib.dskgpu_graph_adjacency.argtypes == [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    assert lib.dskgpu_graph_neighbors.argtypes == [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]


def test_null_context_is_an_argument_error():
    """The calls that need no device: a null context is refused before anything is touched."""
    lib = library()
    assert lib.dskgpu_graph_adjacency(None, None, None) == -1
    assert lib.dskgpu_graph_neighbors(None, None, 0, None) == -1


def test_kmer_counter_has_the_methods():
    from dsk_amd.engine import KmerCounter
    for name in ("graph_adjacency", "graph_adjacency_tensor", "graph_neighbors", "graph_neighbors_tensor"):
        assert callable(getattr(KmerCounter, name, None)), name
