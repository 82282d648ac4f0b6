"""CPU-side checks of the component entry points (include/dskgpu.h "connected components"): declared in the header with the documented
argument lists and structure bodies, listed in engine.EXPORTS, exported by the built library with the documented argtypes, structures of 64,
32 and 64 bytes, and reachable from KmerCounter.  No compute calls.  All of it fails before the feature."""
import ctypes as C

from tests.test_tips_abi import struct_body
from tests.test_unitigs_abi import declared_args, header_text, library

NAMES = ["dskgpu_components", "dskgpu_components_labels", "dskgpu_components_table", "dskgpu_graph_small_components", "dskgpu_drop_components"]


def test_header_declares_the_five_calls():
    assert declared_args("dskgpu_components") == ["dskgpu_ctx* ctx", "dskgpu_component_stats* stats"]
    assert declared_args("dskgpu_components_labels") == ["dskgpu_ctx* ctx", "void* d_unitig_comp", "void* d_row_comp"]
    assert declared_args("dskgpu_components_table") == ["dskgpu_ctx* ctx", "void* d_first", "void* d_unitigs", "void* d_rows", "void* d_ab_sum", "void* d_edges"]
    assert declared_args("dskgpu_graph_small_components") == ["dskgpu_ctx* ctx", "const dskgpu_component_params* params", "void* d_row_drop",
                                                              "void* d_comp_small", "dskgpu_component_drop_stats* stats"]
    assert declared_args("dskgpu_drop_components") == ["dskgpu_ctx* ctx", "const dskgpu_component_params* params", "dskgpu_component_drop_stats* stats"]


def test_header_declares_the_structures():
    assert struct_body("dskgpu_component_stats") == "uint64_t n_components, n_single, max_unitigs, max_rows, n_rounds, reserved[3];"
    assert struct_body("dskgpu_component_params") == "uint32_t min_rows, max_abundance, reserved[6];"
    assert struct_body("dskgpu_component_drop_stats") == "uint64_t n_small, n_unitigs_dropped, n_rows_dropped, n_rows_left, reserved[4];"


def test_header_states_the_facts_the_tests_hold_the_device_to():
    import os
    import re
    from tests.test_unitigs_abi import ROOT
    text = " ".join(open(os.path.join(ROOT, "include", "dskgpu.h")).read().split())
    text = re.sub(r" \* ", " ", text)
    for phrase in ("ONE APPLICATION IS FINAL", "a second application removes nothing", "there are no rounds", "for every entry U -> V there is an entry from a reading of v to a reading of u",
                   "4 bytes per unitig + 36 per component", "n_rounds is always 3"):
        assert phrase in text, phrase


def test_exports_list_and_library():
    from dsk_amd import engine
    for name in NAMES:
        assert name in engine.EXPORTS, name
    lib = library()
    for name in NAMES:
        assert getattr(lib, name).restype is C.c_int, name
    vp = C.c_void_p
    assert lib.dskgpu_components.argtypes == [vp, C.POINTER(engine._ComponentStats)]
    assert lib.dskgpu_components_labels.argtypes == [vp, vp, vp]
    assert lib.dskgpu_components_table.argtypes == [vp, vp, vp, vp, vp, vp]
    assert lib.dskgpu_graph_small_components.argtypes == [vp, C.POINTER(engine._ComponentParams), vp, vp, C.POINTER(engine._ComponentDropStats)]
    assert lib.dskgpu_drop_components.argtypes == [vp, C.POINTER(engine._ComponentParams), C.POINTER(engine._ComponentDropStats)]


def test_structures_are_64_32_and_64_bytes():
    from dsk_amd import engine
    assert C.sizeof(engine._ComponentStats) == 64 and C.sizeof(engine._ComponentParams) == 32 and C.sizeof(engine._ComponentDropStats) == 64
    assert [n for n, _ in engine._ComponentStats._fields_] == ["n_components", "n_single", "max_unitigs", "max_rows", "n_rounds", "reserved"]
    assert [n for n, _ in engine._ComponentParams._fields_] == ["min_rows", "max_abundance", "reserved"]
    assert [n for n, _ in engine._ComponentDropStats._fields_] == ["n_small", "n_unitigs_dropped", "n_rows_dropped", "n_rows_left", "reserved"]


def test_null_context_is_an_argument_error():
    """The calls that need no device: a null context is refused before anything is touched."""
    from dsk_amd import engine
    lib = library()
    par, st, dst = engine._ComponentParams(min_rows=62), engine._ComponentStats(), engine._ComponentDropStats()
    assert lib.dskgpu_components(None, C.byref(st)) == -1
    assert lib.dskgpu_components_labels(None, None, None) == -1
    assert lib.dskgpu_components_table(None, None, None, None, None, None) == -1
    assert lib.dskgpu_graph_small_components(None, C.byref(par), None, None, C.byref(dst)) == -1
    assert lib.dskgpu_drop_components(None, C.byref(par), C.byref(dst)) == -1


def test_kmer_counter_has_the_methods():
    from dsk_amd.engine import KmerCounter
    for name in ("components", "components_labels", "components_labels_tensor", "components_table", "components_table_tensor",
                 "small_components", "small_components_tensor", "drop_components"):
        assert callable(getattr(KmerCounter, name, None)), name
