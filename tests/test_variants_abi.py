"""CPU-side checks of the variant entry points (include/dskgpu.h "variant reporting"): declared in the header with the documented argument
lists and structure bodies, listed in engine.EXPORTS, exported by the built library with the documented argtypes, structures of 32 and 64
bytes, and reachable from KmerCounter.  No compute calls.  All of it fails before the feature."""
import ctypes as C

from tests.test_tips_abi import struct_body
from tests.test_unitigs_abi import declared_args, library

NAMES = ["dskgpu_variants", "dskgpu_variants_table", "dskgpu_variants_stream"]


def test_header_declares_the_three_calls():
    assert declared_args("dskgpu_variants") == ["dskgpu_ctx* ctx", "const dskgpu_variant_params* params", "dskgpu_variant_stats* stats"]
    assert declared_args("dskgpu_variants_table") == ["dskgpu_ctx* ctx", "void* d_records"]
    assert declared_args("dskgpu_variants_stream") == ["dskgpu_ctx* ctx", "void* d_offsets", "void* d_bytes", "uint64_t capacity"]


def test_header_declares_the_structures():
    assert struct_body("dskgpu_variant_params") == "uint32_t max_nodes, max_diff, reserved[6];"
    assert struct_body("dskgpu_variant_stats") == "uint64_t n_variants, n_snps, n_multi, n_indels, n_complex, n_unitigs, stream_bytes, max_letters;"


def test_exports_list_and_library():
    from dsk_amd import engine
    for name in NAMES:
        assert name in engine.EXPORTS, name
    lib = library()
    for name in NAMES:
        assert getattr(lib, name).restype is C.c_int, name
    assert lib.dskgpu_variants.argtypes == [C.c_void_p, C.POINTER(engine._VariantParams), C.POINTER(engine._VariantStats)]
    assert lib.dskgpu_variants_table.argtypes == [C.c_void_p, C.c_void_p]
    assert lib.dskgpu_variants_stream.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]


def test_structures_are_32_and_64_bytes():
    from dsk_amd import engine
    assert C.sizeof(engine._VariantParams) == 32 and C.sizeof(engine._VariantStats) == 64
    assert [n for n, _ in engine._VariantParams._fields_] == ["max_nodes", "max_diff", "reserved"]
    assert [n for n, _ in engine._VariantStats._fields_] == ["n_variants", "n_snps", "n_multi", "n_indels", "n_complex", "n_unitigs", "stream_bytes",
                                                            "max_letters"]
    assert engine.VARIANT_KINDS == {1: "SNP", 2: "MULTI", 3: "INDEL", 4: "COMPLEX"}


def test_null_context_is_an_argument_error():
    """The calls that need no device: a null context is refused before anything is touched."""
    from dsk_amd import engine
    lib = library()
    par, st = engine._VariantParams(max_nodes=62, max_diff=4), engine._VariantStats()
    assert lib.dskgpu_variants(None, C.byref(par), C.byref(st)) == -1
    assert lib.dskgpu_variants_table(None, None) == -1
    assert lib.dskgpu_variants_stream(None, None, None, 0) == -1


def test_kmer_counter_has_the_methods():
    from dsk_amd.engine import KmerCounter
    for name in ("variants", "variants_table", "variants_tensor", "variants_stream", "variants_stream_tensor", "write_variants"):
        assert callable(getattr(KmerCounter, name, None)), name
