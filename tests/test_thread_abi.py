"""CPU-side checks of the read-threading entry points (include/dskgpu.h "reads threaded through the compacted graph"): declared in the
header with the documented argument lists and structure body, listed in engine.EXPORTS, exported by the built library with the documented
argtypes, a structure of 64 bytes, and reachable from KmerCounter.  No compute calls.  All of it fails before the feature."""
import ctypes as C

from tests.test_tips_abi import struct_body
from tests.test_unitigs_abi import declared_args, library

NAMES = ["dskgpu_thread_place", "dskgpu_thread_reads", "dskgpu_thread_walks", "dskgpu_thread_support"]


def test_header_declares_the_four_calls():
    assert declared_args("dskgpu_thread_place") == ["dskgpu_ctx* ctx", "const void* d_bytes", "uint64_t nbytes", "void* d_unitig", "void* d_off"]
    assert declared_args("dskgpu_thread_reads") == ["dskgpu_ctx* ctx", "const void* d_bytes", "uint64_t nbytes", "dskgpu_thread_stats* stats"]
    assert declared_args("dskgpu_thread_walks") == ["dskgpu_ctx* ctx", "void* d_offsets", "void* d_steps", "void* d_first", "void* d_last", "void* d_ends"]
    assert declared_args("dskgpu_thread_support") == ["dskgpu_ctx* ctx", "void* d_unitig_support", "void* d_edge_support"]


def test_header_declares_the_structure():
    assert struct_body("dskgpu_thread_stats") == "uint64_t n_valid, n_placed, n_walks, n_steps, max_steps, reserved[3];"


def test_exports_list_and_library():
    from dsk_amd import engine
    for name in NAMES:
        assert name in engine.EXPORTS, name
    lib = library()
    for name in NAMES:
        assert getattr(lib, name).restype is C.c_int, name
    assert lib.dskgpu_thread_place.argtypes == [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    assert lib.dskgpu_thread_reads.argtypes == [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(engine._ThreadStats)]
    assert lib.dskgpu_thread_walks.argtypes == [C.c_void_p] * 6
    assert lib.dskgpu_thread_support.argtypes == [C.c_void_p] * 3


def test_the_structure_is_64_bytes():
    from dsk_amd import engine
    assert C.sizeof(engine._ThreadStats) == 64
    assert [n for n, _ in engine._ThreadStats._fields_] == ["n_valid", "n_placed", "n_walks", "n_steps", "max_steps", "reserved"]


def test_null_context_is_an_argument_error():
    """The calls that need no device: a null context is refused before anything is touched."""
    from dsk_amd import engine
    lib = library()
    st = engine._ThreadStats()
    buf = C.create_string_buffer(64)
    assert lib.dskgpu_thread_place(None, buf, 8, buf, buf) == -1
    assert lib.dskgpu_thread_reads(None, buf, 8, C.byref(st)) == -1
    assert lib.dskgpu_thread_walks(None, buf, None, None, None, None) == -1
    assert lib.dskgpu_thread_support(None, buf, buf) == -1


def test_kmer_counter_has_the_methods():
    from dsk_amd.engine import KmerCounter
    for name in ("thread_place", "thread_place_tensor", "thread_reads", "thread_reads_tensor", "thread_walks", "thread_walks_tensor",
                 "thread_support", "thread_support_tensor", "write_gfa_walks"):
        assert callable(getattr(KmerCounter, name, None)), name
