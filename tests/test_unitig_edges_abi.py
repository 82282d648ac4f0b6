"""CPU-side checks of the unitig edge entry points (include/dskgpu.h "unitig links"): declared in the header with the documented argument
lists, listed in engine.EXPORTS, exported by the built library with the documented argtypes, the statistics structure of 64 bytes, and
reachable from KmerCounter.  No compute calls.  All of it fails before the feature."""
import ctypes as C
import re

from tests.test_unitigs_abi import declared_args, header_text, library

NAMES = ["dskgpu_unitig_edges", "dskgpu_unitig_edges_table"]


def test_header_declares_the_two_calls():
    assert declared_args("dskgpu_unitig_edges") == ["dskgpu_ctx* ctx", "dskgpu_unitig_edge_stats* stats"]
    assert declared_args("dskgpu_unitig_edges_table") == ["dskgpu_ctx* ctx", "void* d_offsets", "void* d_targets", "void* d_ends"]


def test_header_declares_the_stats_structure():
    m = re.search(r"typedef\s+struct\s+dskgpu_unitig_edge_stats\s*\{([^}]*)\}\s*dskgpu_unitig_edge_stats\s*;", header_text())
    assert m
    assert " ".join(m.group(1).split()) == "uint64_t n_edges, n_self, n_dead_ends, max_degree, reserved[4];"


def test_exports_list_and_library():
    from dsk_amd import engine
    for name in NAMES:
        assert name in engine.EXPORTS, name
    lib = library()
    for name in NAMES:
        assert getattr(lib, name).restype is C.c_int, name
    assert lib.dskgpu_unitig_edges.argtypes == [C.c_void_p, C.POINTER(engine._UnitigEdgeStats)]
    assert lib.dskgpu_unitig_edges_table.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]


def test_stats_structure_is_64_bytes():
    from dsk_amd import engine
    assert C.sizeof(engine._UnitigEdgeStats) == 64
    assert [n for n, _ in engine._UnitigEdgeStats._fields_] == ["n_edges", "n_self", "n_dead_ends", "max_degree", "reserved"]


def test_null_context_is_an_argument_error():
    """The calls that need no device: a null context is refused before anything is touched."""
    lib = library()
    assert lib.dskgpu_unitig_edges(None, None) == -1
    assert lib.dskgpu_unitig_edges_table(None, None, None, None) == -1


def test_kmer_counter_has_the_methods():
    from dsk_amd.engine import KmerCounter
    for name in ("unitig_edges", "unitig_edges_table", "unitig_edges_tensor", "write_gfa"):
        assert callable(getattr(KmerCounter, name, None)), name
