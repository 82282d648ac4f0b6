"""CPU-side checks of the erroneous-connection entry points (include/dskgpu.h "erroneous connections"): declared in the header with the
documented argument lists and structure bodies, listed in engine.EXPORTS, exported by the built library with the documented argtypes,
structures of 32, 64 and 256 bytes, and reachable from KmerCounter.  No compute calls.  All of it fails before the feature."""
import ctypes as C

from tests.test_tips_abi import struct_body
from tests.test_unitigs_abi import declared_args, library

NAMES = ["dskgpu_graph_connections", "dskgpu_remove_connections", "dskgpu_simplify_all"]


def test_header_declares_the_three_calls():
    assert declared_args("dskgpu_graph_connections") == ["dskgpu_ctx* ctx", "const dskgpu_connection_params* params", "void* d_row_rem", "void* d_unitig_bits",
                                                         "dskgpu_connection_stats* stats"]
    assert declared_args("dskgpu_remove_connections") == ["dskgpu_ctx* ctx", "const dskgpu_connection_params* params", "dskgpu_connection_stats* stats"]
    assert declared_args("dskgpu_simplify_all") == ["dskgpu_ctx* ctx", "const dskgpu_tip_params* tip_params", "const dskgpu_bubble_params* bubble_params",
                                                    "const dskgpu_connection_params* connection_params", "uint32_t max_passes", "dskgpu_simplify_all_stats* stats"]
    # dskgpu_simplify and its stats stay as they are
    assert declared_args("dskgpu_simplify") == ["dskgpu_ctx* ctx", "const dskgpu_tip_params* tip_params", "const dskgpu_bubble_params* bubble_params",
                                                "uint32_t max_passes", "dskgpu_simplify_stats* stats"]
    assert struct_body("dskgpu_simplify_stats") == "uint64_t n_passes, n_rows_left, reserved[6]; dskgpu_tip_stats tips; dskgpu_bubble_stats bubbles;"


def test_header_declares_the_structures():
    assert struct_body("dskgpu_connection_params") == "uint32_t max_nodes, min_ratio, max_abundance, max_rounds, reserved[4];"
    assert struct_body("dskgpu_connection_stats") == "uint64_t n_candidates, n_one_sided, n_removed, n_rows_removed, n_rounds, n_rows_left, reserved[2];"
    assert struct_body("dskgpu_simplify_all_stats") == ("uint64_t n_passes, n_rows_left, reserved[6]; dskgpu_tip_stats tips; dskgpu_bubble_stats bubbles; "
                                                        "dskgpu_connection_stats connections;")


def test_exports_list_and_library():
    from dsk_amd import engine
    for name in NAMES:
        assert name in engine.EXPORTS, name
    lib = library()
    for name in NAMES:
        assert getattr(lib, name).restype is C.c_int, name
    assert lib.dskgpu_graph_connections.argtypes == [C.c_void_p, C.POINTER(engine._ConnectionParams), C.c_void_p, C.c_void_p, C.POINTER(engine._ConnectionStats)]
    assert lib.dskgpu_remove_connections.argtypes == [C.c_void_p, C.POINTER(engine._ConnectionParams), C.POINTER(engine._ConnectionStats)]
    assert lib.dskgpu_simplify_all.argtypes == [C.c_void_p, C.POINTER(engine._TipParams), C.POINTER(engine._BubbleParams), C.POINTER(engine._ConnectionParams),
                                                C.c_uint32, C.POINTER(engine._SimplifyAllStats)]


def test_structures_are_32_64_and_256_bytes():
    from dsk_amd import engine
    assert C.sizeof(engine._ConnectionParams) == 32 and C.sizeof(engine._ConnectionStats) == 64 and C.sizeof(engine._SimplifyAllStats) == 256
    assert [n for n, _ in engine._ConnectionParams._fields_] == ["max_nodes", "min_ratio", "max_abundance", "max_rounds", "reserved"]
    assert [n for n, _ in engine._ConnectionStats._fields_] == ["n_candidates", "n_one_sided", "n_removed", "n_rows_removed", "n_rounds", "n_rows_left", "reserved"]
    assert [n for n, _ in engine._SimplifyAllStats._fields_] == ["n_passes", "n_rows_left", "reserved", "tips", "bubbles", "connections"]
    assert (engine._SimplifyAllStats.tips.offset, engine._SimplifyAllStats.bubbles.offset, engine._SimplifyAllStats.connections.offset) == (64, 128, 192)


def test_null_context_is_an_argument_error():
    """The calls that need no device: a null context is refused before anything is touched."""
    from dsk_amd import engine
    lib = library()
    tip, bub, par = engine._TipParams(max_nodes=31), engine._BubbleParams(max_nodes=62, max_diff=4), engine._ConnectionParams(max_nodes=62, min_ratio=4)
    st, sst = engine._ConnectionStats(), engine._SimplifyAllStats()
    assert lib.dskgpu_graph_connections(None, C.byref(par), None, None, C.byref(st)) == -1
    assert lib.dskgpu_remove_connections(None, C.byref(par), C.byref(st)) == -1
    assert lib.dskgpu_simplify_all(None, C.byref(tip), C.byref(bub), C.byref(par), 0, C.byref(sst)) == -1


def test_kmer_counter_has_the_methods():
    from dsk_amd.engine import KmerCounter
    for name in ("graph_connections", "graph_connections_tensor", "remove_connections", "simplify_all"):
        assert callable(getattr(KmerCounter, name, None)), name
