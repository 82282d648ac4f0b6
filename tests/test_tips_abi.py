"""CPU-side checks of the row filter and tip entry points (include/dskgpu.h "tip clipping"): declared in the header with the documented
argument lists and structure bodies, listed in engine.EXPORTS, exported by the built library with the documented argtypes, structures of
32 and 64 bytes, and reachable from KmerCounter.  No compute calls.  All of it fails before the feature."""
import ctypes as C
import re

from tests.test_unitigs_abi import declared_args, header_text, library

NAMES = ["dskgpu_filter_rows", "dskgpu_graph_tips", "dskgpu_clip_tips"]


def test_header_declares_the_three_calls():
    assert declared_args("dskgpu_filter_rows") == ["dskgpu_ctx* ctx", "const void* d_keep", "uint64_t* n_kept"]
    assert declared_args("dskgpu_graph_tips") == ["dskgpu_ctx* ctx", "const dskgpu_tip_params* params", "void* d_row_tip", "void* d_unitig_tip",
                                                  "dskgpu_tip_stats* stats"]
    assert declared_args("dskgpu_clip_tips") == ["dskgpu_ctx* ctx", "const dskgpu_tip_params* params", "dskgpu_tip_stats* stats"]


def struct_body(name):
    m = re.search(r"typedef\s+struct\s+%s\s*\{([^}]*)\}\s*%s\s*;" % (name, name), header_text())
    assert m, name
    return " ".join(m.group(1).split())


def test_header_declares_both_structures():
    assert struct_body("dskgpu_tip_params") == "uint32_t max_nodes, max_abundance, max_rounds, reserved[5];"
    assert struct_body("dskgpu_tip_stats") == "uint64_t n_candidates, n_tips, n_outranked, n_rows_clipped, n_rounds, n_rows_left, reserved[2];"


def test_exports_list_and_library():
    from dsk_amd import engine
    for name in NAMES:
        assert name in engine.EXPORTS, name
    lib = library()
    for name in NAMES:
        assert getattr(lib, name).restype is C.c_int, name
    assert lib.dskgpu_filter_rows.argtypes == [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    assert lib.dskgpu_graph_tips.argtypes == [C.c_void_p, C.POINTER(engine._TipParams), C.c_void_p, C.c_void_p, C.POINTER(engine._TipStats)]
    assert lib.dskgpu_clip_tips.argtypes == [C.c_void_p, C.POINTER(engine._TipParams), C.POINTER(engine._TipStats)]


def test_structures_are_32_and_64_bytes():
    from dsk_amd import engine
    assert C.sizeof(engine._TipParams) == 32 and C.sizeof(engine._TipStats) == 64
    assert [n for n, _ in engine._TipParams._fields_] == ["max_nodes", "max_abundance", "max_rounds", "reserved"]
    assert [n for n, _ in engine._TipStats._fields_] == ["n_candidates", "n_tips", "n_outranked", "n_rows_clipped", "n_rounds", "n_rows_left", "reserved"]


def test_null_context_is_an_argument_error():
    """The calls that need no device: a null context is refused before anything is touched."""
    from dsk_amd import engine
    lib = library()
    par, st, n = engine._TipParams(max_nodes=31), engine._TipStats(), C.c_uint64(7)
    assert lib.dskgpu_filter_rows(None, None, C.byref(n)) == -1 and n.value == 7
    assert lib.dskgpu_graph_tips(None, C.byref(par), None, None, C.byref(st)) == -1
    assert lib.dskgpu_clip_tips(None, C.byref(par), C.byref(st)) == -1


def test_kmer_counter_has_the_methods():
    from dsk_amd.engine import KmerCounter
    for name in ("filter_rows", "filter_rows_tensor", "graph_tips", "graph_tips_tensor", "clip_tips", "write_gfa"):
        assert callable(getattr(KmerCounter, name, None)), name
