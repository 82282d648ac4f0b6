"""CPU-side checks of the bubble entry points (include/dskgpu.h "bubble popping"): declared in the header with the documented argument
lists and structure bodies, listed in engine.EXPORTS, exported by the built library with the documented argtypes, structures of 32, 64 and
192 bytes, and reachable from KmerCounter.  No compute calls.  All of it fails before the feature."""
import ctypes as C

from tests.test_tips_abi import struct_body
from tests.test_unitigs_abi import declared_args, header_text, library

NAMES = ["dskgpu_graph_bubbles", "dskgpu_pop_bubbles", "dskgpu_simplify"]


def test_header_declares_the_three_calls():
    assert declared_args("dskgpu_graph_bubbles") == ["dskgpu_ctx* ctx", "const dskgpu_bubble_params* params", "void* d_row_pop", "void* d_unitig_bits",
                                                     "dskgpu_bubble_stats* stats"]
    assert declared_args("dskgpu_pop_bubbles") == ["dskgpu_ctx* ctx", "const dskgpu_bubble_params* params", "dskgpu_bubble_stats* stats"]
    assert declared_args("dskgpu_simplify") == ["dskgpu_ctx* ctx", "const dskgpu_tip_params* tip_params", "const dskgpu_bubble_params* bubble_params",
                                                "uint32_t max_passes", "dskgpu_simplify_stats* stats"]
    assert "Bubble popping is not done" not in header_text()


def test_header_declares_the_structures():
    assert struct_body("dskgpu_bubble_params") == "uint32_t max_nodes, max_diff, max_rounds, reserved[5];"
    assert struct_body("dskgpu_bubble_stats") == "uint64_t n_candidates, n_in_bubbles, n_popped, n_rows_popped, n_rounds, n_rows_left, reserved[2];"
    assert struct_body("dskgpu_simplify_stats") == "uint64_t n_passes, n_rows_left, reserved[6]; dskgpu_tip_stats tips; dskgpu_bubble_stats bubbles;"


def test_exports_list_and_library():
    from dsk_amd import engine
    for name in NAMES:
        assert name in engine.EXPORTS, name
    lib = library()
    for name in NAMES:
        assert getattr(lib, name).restype is C.c_int, name
    assert lib.dskgpu_graph_bubbles.argtypes == [C.c_void_p, C.POINTER(engine._BubbleParams), C.c_void_p, C.c_void_p, C.POINTER(engine._BubbleStats)]
    assert lib.dskgpu_pop_bubbles.argtypes == [C.c_void_p, C.POINTER(engine._BubbleParams), C.POINTER(engine._BubbleStats)]
    assert lib.dskgpu_simplify.argtypes == [C.c_void_p, C.POINTER(engine._TipParams), C.POINTER(engine._BubbleParams), C.c_uint32,
                                            C.POINTER(engine._SimplifyStats)]


def test_structures_are_32_64_and_192_bytes():
    from dsk_amd import engine
    assert C.sizeof(engine._BubbleParams) == 32 and C.sizeof(engine._BubbleStats) == 64 and C.sizeof(engine._SimplifyStats) == 192
    assert [n for n, _ in engine._BubbleParams._fields_] == ["max_nodes", "max_diff", "max_rounds", "reserved"]
    assert [n for n, _ in engine._BubbleStats._fields_] == ["n_candidates", "n_in_bubbles", "n_popped", "n_rows_popped", "n_rounds", "n_rows_left", "reserved"]
    assert [n for n, _ in engine._SimplifyStats._fields_] == ["n_passes", "n_rows_left", "reserved", "tips", "bubbles"]
    assert engine._SimplifyStats.tips.offset == 64 and engine._SimplifyStats.bubbles.offset == 128


def test_null_context_is_an_argument_error():
    """The calls that need no device: a null context is refused before anything is touched."""
    from dsk_amd import engine
    lib = library()
    tip, par, st, sst = engine._TipParams(max_nodes=31), engine._BubbleParams(max_nodes=62, max_diff=4), engine._BubbleStats(), engine._SimplifyStats()
    assert lib.dskgpu_graph_bubbles(None, C.byref(par), None, None, C.byref(st)) == -1
    assert lib.dskgpu_pop_bubbles(None, C.byref(par), C.byref(st)) == -1
    assert lib.dskgpu_simplify(None, C.byref(tip), C.byref(par), 0, C.byref(sst)) == -1


def test_kmer_counter_has_the_methods():
    from dsk_amd.engine import KmerCounter
    for name in ("graph_bubbles", "graph_bubbles_tensor", "pop_bubbles", "simplify"):
        assert callable(getattr(KmerCounter, name, None)), name
