"""CPU-side checks of the lookup entry points (include/dskgpu.h "lookups in the last result"): declared in the header, listed in
engine.EXPORTS, exported by the built library with the declared argument lists, and reachable from KmerCounter.  No compute calls."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dskgpu_query_prepare", "dskgpu_query_kmers", "dskgpu_query_reads"]


def header_text():
    src = open(os.path.join(ROOT, "include", "dskgpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_lookups():
    src = header_text()
    assert re.search(r"\bint\s+dskgpu_query_prepare\s*\(\s*dskgpu_ctx\s*\*\s*ctx\s*\)\s*;", src)
    for name, first in (("dskgpu_query_kmers", "d_kmers"), ("dskgpu_query_reads", "d_bytes")):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == 4 and args[0].startswith("dskgpu_ctx") and args[1] == "const void* " + first, (name, args)
        assert args[2].startswith("uint64_t") and args[3] == "void* d_abundance", (name, args)


def test_exports_list_and_library():
    from dsk_amd import engine
    for name in NAMES:
        assert name in engine.EXPORTS, name
    if not os.path.exists(engine.library_path()):
        import __graft_entry__ as g
        g.build()
    lib = engine.load_library()
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int, name
    assert lib.dskgpu_query_prepare.argtypes == [C.c_void_p]
    assert lib.dskgpu_query_kmers.argtypes == [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    assert lib.dskgpu_query_reads.argtypes == [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]


def test_null_context_is_an_argument_error():
    """The one call that needs no device: a null context is refused before anything is touched."""
    from dsk_amd import engine
    if not os.path.exists(engine.library_path()):
        import __graft_entry__ as g
        g.build()
    lib = engine.load_library()
    assert lib.dskgpu_query_prepare(None) == -1
    assert lib.dskgpu_query_kmers(None, None, 0, None) == -1
    assert lib.dskgpu_query_reads(None, None, 0, None) == -1


def test_kmer_counter_has_the_methods():
    from dsk_amd.engine import KmerCounter
    for name in ("query_prepare", "query_kmers", "query_reads", "query_kmers_tensor", "query_reads_tensor"):
        assert callable(getattr(KmerCounter, name, None)), name
