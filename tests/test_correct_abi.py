"""CPU-side checks of the read-correction entry point (include/dskgpu.h "substitution errors in reads corrected against the count"): declared
in the header with the documented argument list and structure bodies, listed in engine.EXPORTS, exported by the built library with the
documented argtypes, structures of 32 and 128 bytes, and reachable from KmerCounter.  No compute calls.  All of it fails before the feature."""
import ctypes as C

from tests.test_tips_abi import struct_body
from tests.test_unitigs_abi import declared_args, library

NAME = "dskgpu_correct_reads"
STATS = ["n_valid", "n_trusted", "n_gaps", "n_interior", "n_head", "n_tail", "n_skipped", "n_corrected", "n_ambiguous", "n_unfixable"]


def test_header_declares_the_call():
    """fails before the feature: the header has no dskgpu_correct_reads"""
    assert declared_args(NAME) == ["dskgpu_ctx* ctx", "const void* d_bytes", "uint64_t nbytes", "const dskgpu_correct_params* params", "void* d_out",
                                   "void* d_state", "dskgpu_correct_stats* stats"]


def test_header_declares_both_structures():
    """fails before the feature: neither structure is declared"""
    assert struct_body("dskgpu_correct_params") == "uint32_t trust_min, flags; uint64_t reserved[3];"
    assert struct_body("dskgpu_correct_stats") == "uint64_t " + ", ".join(STATS) + ", reserved[6];"


def test_exports_list_and_library():
    """fails before the feature: the name is not in EXPORTS and the library does not export it"""
    from dsk_amd import engine
    assert NAME in engine.EXPORTS
    lib = library()
    assert lib.dskgpu_correct_reads.restype is C.c_int
    assert lib.dskgpu_correct_reads.argtypes == [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(engine._CorrectParams), C.c_void_p, C.c_void_p,
                                                 C.POINTER(engine._CorrectStats)]


def test_structures_are_32_and_128_bytes():
    """fails before the feature: engine has no _CorrectParams / _CorrectStats"""
    from dsk_amd import engine
    assert C.sizeof(engine._CorrectParams) == 32 and C.sizeof(engine._CorrectStats) == 128
    assert [n for n, _ in engine._CorrectParams._fields_] == ["trust_min", "flags", "reserved"]
    assert [n for n, _ in engine._CorrectStats._fields_] == STATS + ["reserved"]


def test_null_context_is_an_argument_error():
    """The call needs no device for this: a null context is refused before anything is touched.  Fails before the feature: no such symbol."""
    from dsk_amd import engine
    lib = library()
    par, st = engine._CorrectParams(trust_min=3), engine._CorrectStats()
    buf = C.create_string_buffer(64)
    assert lib.dskgpu_correct_reads(None, buf, 8, C.byref(par), buf, buf, C.byref(st)) == -1
    assert lib.dskgpu_correct_reads(None, None, 0, None, None, None, None) == -1


def test_kmer_counter_has_the_methods():
    """fails before the feature: KmerCounter has neither method"""
    from dsk_amd.engine import KmerCounter
    for name in ("correct_reads", "correct_reads_tensor"):
        assert callable(getattr(KmerCounter, name, None)), name
