"""ctypes binding of include/dskgpu.h.

`KmerCounter` mirrors the one call the reference makes on this path,
`SortingCountAlgorithm<span>(bank, props).execute()` (src/DSK.cpp:55-60), and
the read-back done by dsk2ascii (utils/dsk2ascii.cpp:61-104): rows of
(kmer value, abundance) per "solid" partition plus the abundance histogram.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


class DskGpuError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"dskgpu error {code}: {msg}")
        self.code = code


class _Config(C.Structure):
    _fields_ = [
        ("kmer_size", C.c_uint32),
        ("abundance_min", C.c_uint32),
        ("abundance_max", C.c_uint32),
        ("histo_max", C.c_uint32),
        ("device", C.c_int32),
        ("nb_partitions", C.c_uint32),
        ("minimizer_size", C.c_uint32),
        ("flags", C.c_uint32),
        ("world_size", C.c_uint32),
        ("rank", C.c_uint32),
        ("max_pass_mkeys", C.c_uint32),
        ("solidity_kind", C.c_uint32),
        ("solidity_custom", C.c_uint32),
        ("reserved", C.c_uint32 * 3),
    ]


class _Stats(C.Structure):
    _fields_ = [
        ("n_bytes", C.c_uint64),
        ("n_kmers", C.c_uint64),
        ("n_distinct", C.c_uint64),
        ("n_solid", C.c_uint64),
        ("n_partitions", C.c_uint32),
        ("n_levels", C.c_uint32),
        ("n_final_bins", C.c_uint32),
        ("n_retries", C.c_uint32),
        ("sort_fallback", C.c_uint64),
        ("n_passes", C.c_uint64),
        ("n_ext_regions", C.c_uint64),
        ("n_heavy", C.c_uint64),
        ("n_read_sweeps", C.c_uint64),
    ]


class _UnitigStats(C.Structure):
    _fields_ = [
        ("n_unitigs", C.c_uint64),
        ("n_cycles", C.c_uint64),
        ("n_single", C.c_uint64),
        ("max_nodes", C.c_uint64),
        ("stream_bytes", C.c_uint64),
        ("n_rounds", C.c_uint64),
        ("reserved", C.c_uint64 * 2),
    ]


class _UnitigEdgeStats(C.Structure):
    _fields_ = [
        ("n_edges", C.c_uint64),
        ("n_self", C.c_uint64),
        ("n_dead_ends", C.c_uint64),
        ("max_degree", C.c_uint64),
        ("reserved", C.c_uint64 * 4),
    ]


class _ThreadStats(C.Structure):
    _fields_ = [
        ("n_valid", C.c_uint64),
        ("n_placed", C.c_uint64),
        ("n_walks", C.c_uint64),
        ("n_steps", C.c_uint64),
        ("max_steps", C.c_uint64),
        ("reserved", C.c_uint64 * 3),
    ]


class _CorrectParams(C.Structure):
    _fields_ = [
        ("trust_min", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint64 * 3),
    ]


class _CorrectStats(C.Structure):
    _fields_ = [
        ("n_valid", C.c_uint64),
        ("n_trusted", C.c_uint64),
        ("n_gaps", C.c_uint64),
        ("n_interior", C.c_uint64),
        ("n_head", C.c_uint64),
        ("n_tail", C.c_uint64),
        ("n_skipped", C.c_uint64),
        ("n_corrected", C.c_uint64),
        ("n_ambiguous", C.c_uint64),
        ("n_unfixable", C.c_uint64),
        ("reserved", C.c_uint64 * 6),
    ]


class _ReadSummaryParams(C.Structure):
    _fields_ = [
        ("trust_min", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint64 * 3),
    ]


class _ReadSummaryStats(C.Structure):
    _fields_ = [
        ("n_records", C.c_uint64),
        ("n_empty", C.c_uint64),
        ("n_valid", C.c_uint64),
        ("n_solid", C.c_uint64),
        ("max_len", C.c_uint64),
        ("reserved", C.c_uint64 * 3),
    ]


class _ReadRule(C.Structure):
    _fields_ = [
        ("min_valid", C.c_uint32),
        ("median_min", C.c_uint32),
        ("median_max", C.c_uint32),
        ("solid_num", C.c_uint32),
        ("solid_den", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint64),
    ]


class _ReadMarkStats(C.Structure):
    _fields_ = [
        ("n_records", C.c_uint64),
        ("n_kept", C.c_uint64),
        ("kept_bytes", C.c_uint64),
        ("kept_valid", C.c_uint64),
        ("reserved", C.c_uint64 * 4),
    ]


class _ColorStats(C.Structure):
    _fields_ = [
        ("n_valid", C.c_uint64),
        ("n_placed", C.c_uint64),
        ("n_rows", C.c_uint64),
        ("n_colors", C.c_uint64),
        ("reserved", C.c_uint64 * 4),
    ]


class _ColorPairStats(C.Structure):
    _fields_ = [
        ("n_rows", C.c_uint64),
        ("n_selected", C.c_uint64),
        ("n_present", C.c_uint64),
        ("n_colors", C.c_uint64),
        ("reserved", C.c_uint64 * 4),
    ]


class _ColorRule(C.Structure):
    _fields_ = [
        ("need_all", C.c_uint64),
        ("need_none", C.c_uint64),
        ("min_count", C.c_uint32),
        ("min_present", C.c_uint32),
        ("max_present", C.c_uint32),
        ("flags", C.c_uint32),
    ]


class _ColorMarkStats(C.Structure):
    _fields_ = [
        ("n_rows", C.c_uint64),
        ("n_kept", C.c_uint64),
        ("reserved", C.c_uint64 * 6),
    ]


COLORS_INVERT = 1


class _LoadStats(C.Structure):
    _fields_ = [
        ("n_in", C.c_uint64),
        ("n_distinct", C.c_uint64),
        ("n_rows", C.c_uint64),
        ("n_below", C.c_uint64),
        ("n_above", C.c_uint64),
        ("n_kmers", C.c_uint64),
        ("n_saturated", C.c_uint64),
        ("sorted_input", C.c_uint64),
    ]


LOAD_COMBINE = {"sum": 0, "max": 1, "min": 2, "unique": 3}      # DSKGPU_LOAD_*

# one summary of dskgpu_read_summaries_table (include/dskgpu.h: SUMMARY), 32 bytes
READ_SUMMARY_DTYPE = np.dtype([("start", "<u8"), ("sum", "<u8"), ("len", "<u4"), ("n_valid", "<u4"), ("n_solid", "<u4"), ("median", "<u4")])
READS_INVERT = 1


class _TipParams(C.Structure):
    _fields_ = [
        ("max_nodes", C.c_uint32),
        ("max_abundance", C.c_uint32),
        ("max_rounds", C.c_uint32),
        ("reserved", C.c_uint32 * 5),
    ]


class _TipStats(C.Structure):
    _fields_ = [
        ("n_candidates", C.c_uint64),
        ("n_tips", C.c_uint64),
        ("n_outranked", C.c_uint64),
        ("n_rows_clipped", C.c_uint64),
        ("n_rounds", C.c_uint64),
        ("n_rows_left", C.c_uint64),
        ("reserved", C.c_uint64 * 2),
    ]


class _BubbleParams(C.Structure):
    _fields_ = [
        ("max_nodes", C.c_uint32),
        ("max_diff", C.c_uint32),
        ("max_rounds", C.c_uint32),
        ("reserved", C.c_uint32 * 5),
    ]


class _BubbleStats(C.Structure):
    _fields_ = [
        ("n_candidates", C.c_uint64),
        ("n_in_bubbles", C.c_uint64),
        ("n_popped", C.c_uint64),
        ("n_rows_popped", C.c_uint64),
        ("n_rounds", C.c_uint64),
        ("n_rows_left", C.c_uint64),
        ("reserved", C.c_uint64 * 2),
    ]


class _SimplifyStats(C.Structure):
    _fields_ = [
        ("n_passes", C.c_uint64),
        ("n_rows_left", C.c_uint64),
        ("reserved", C.c_uint64 * 6),
        ("tips", _TipStats),
        ("bubbles", _BubbleStats),
    ]


class _ConnectionParams(C.Structure):
    _fields_ = [
        ("max_nodes", C.c_uint32),
        ("min_ratio", C.c_uint32),
        ("max_abundance", C.c_uint32),
        ("max_rounds", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class _ConnectionStats(C.Structure):
    _fields_ = [
        ("n_candidates", C.c_uint64),
        ("n_one_sided", C.c_uint64),
        ("n_removed", C.c_uint64),
        ("n_rows_removed", C.c_uint64),
        ("n_rounds", C.c_uint64),
        ("n_rows_left", C.c_uint64),
        ("reserved", C.c_uint64 * 2),
    ]


class _SimplifyAllStats(C.Structure):
    _fields_ = [
        ("n_passes", C.c_uint64),
        ("n_rows_left", C.c_uint64),
        ("reserved", C.c_uint64 * 6),
        ("tips", _TipStats),
        ("bubbles", _BubbleStats),
        ("connections", _ConnectionStats),
    ]


class _VariantParams(C.Structure):
    _fields_ = [
        ("max_nodes", C.c_uint32),
        ("max_diff", C.c_uint32),
        ("reserved", C.c_uint32 * 6),
    ]


class _VariantStats(C.Structure):
    _fields_ = [
        ("n_variants", C.c_uint64),
        ("n_snps", C.c_uint64),
        ("n_multi", C.c_uint64),
        ("n_indels", C.c_uint64),
        ("n_complex", C.c_uint64),
        ("n_unitigs", C.c_uint64),
        ("stream_bytes", C.c_uint64),
        ("max_letters", C.c_uint64),
    ]


VARIANT_KINDS = {1: "SNP", 2: "MULTI", 3: "INDEL", 4: "COMPLEX"}      # kind of a variant record (include/dskgpu.h: "variant reporting")


class _ComponentStats(C.Structure):
    _fields_ = [
        ("n_components", C.c_uint64),
        ("n_single", C.c_uint64),
        ("max_unitigs", C.c_uint64),
        ("max_rows", C.c_uint64),
        ("n_rounds", C.c_uint64),
        ("reserved", C.c_uint64 * 3),
    ]


class _ComponentParams(C.Structure):
    _fields_ = [
        ("min_rows", C.c_uint32),
        ("max_abundance", C.c_uint32),
        ("reserved", C.c_uint32 * 6),
    ]


class _ComponentDropStats(C.Structure):
    _fields_ = [
        ("n_small", C.c_uint64),
        ("n_unitigs_dropped", C.c_uint64),
        ("n_rows_dropped", C.c_uint64),
        ("n_rows_left", C.c_uint64),
        ("reserved", C.c_uint64 * 4),
    ]


MG_BUCKETS = 4096      # DSKGPU_MG_BUCKETS
MG_SPLIT = 255         # DSKGPU_MG_SPLIT


def make_table(summed_loads: np.ndarray, world_size: int) -> np.ndarray:
    """dskgpu_mg_make_table: the (deterministic) repartition table for loads summed over all ranks."""
    loads = np.ascontiguousarray(summed_loads, dtype=np.uint64)
    assert loads.size == MG_BUCKETS
    table = np.zeros(MG_BUCKETS, dtype=np.uint8)
    load_library().dskgpu_mg_make_table(loads.ctypes.data_as(C.POINTER(C.c_uint64)), world_size, table.ctypes.data_as(C.POINTER(C.c_uint8)))
    return table


F_TIMING = 1
F_NO_SORT = 2
F_HISTO2D = 4
F_MG_EXPLICIT = 8
F_PLACE = 16
F_PARTITION_ORDER = 32
SOLIDITY = {"sum": 0, "min": 1, "max": 2, "one": 3, "all": 4, "custom": 5}

# every symbol include/dskgpu.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "dskgpu_create", "dskgpu_destroy", "dskgpu_last_error", "dskgpu_version", "dskgpu_device_count", "dskgpu_set_stream",
    "dskgpu_push_reads", "dskgpu_push_raw", "dskgpu_raw_finish", "dskgpu_stream_bytes", "dskgpu_rewind_reads", "dskgpu_reserve_reads", "dskgpu_reserve_work", "dskgpu_set_reads_device", "dskgpu_encode_reads", "dskgpu_next_bank", "dskgpu_set_banks", "dskgpu_histogram2d",
    "dskgpu_count", "dskgpu_mg_scatter", "dskgpu_mg_sample", "dskgpu_mg_make_table", "dskgpu_mg_set_table",
    "dskgpu_mg_send_capacity_words", "dskgpu_mg_count", "dskgpu_mg_sent_kmers", "dskgpu_mg_count_sized",
    "dskgpu_mg_slices_prepare", "dskgpu_mg_scatter_slice", "dskgpu_mg_slices_finish", "dskgpu_mg_count_sliced", "dskgpu_get_stats", "dskgpu_histogram",
    "dskgpu_set_row_order", "dskgpu_num_partitions", "dskgpu_partition_size", "dskgpu_partition_offsets", "dskgpu_partition_copy", "dskgpu_result_device",
    "dskgpu_stage_times", "dskgpu_query_prepare", "dskgpu_query_kmers", "dskgpu_query_reads", "dskgpu_graph_adjacency", "dskgpu_graph_neighbors",
    "dskgpu_unitigs", "dskgpu_unitigs_rows", "dskgpu_unitigs_table", "dskgpu_unitigs_stream", "dskgpu_unitig_edges", "dskgpu_unitig_edges_table",
    "dskgpu_filter_rows", "dskgpu_graph_tips", "dskgpu_clip_tips",
    "dskgpu_graph_bubbles", "dskgpu_pop_bubbles", "dskgpu_simplify",
    "dskgpu_graph_connections", "dskgpu_remove_connections", "dskgpu_simplify_all",
    "dskgpu_components", "dskgpu_components_labels", "dskgpu_components_table", "dskgpu_graph_small_components", "dskgpu_drop_components",
    "dskgpu_thread_place", "dskgpu_thread_reads", "dskgpu_thread_walks", "dskgpu_thread_support",
    "dskgpu_correct_reads",
    "dskgpu_read_summaries", "dskgpu_read_summaries_table", "dskgpu_read_marks", "dskgpu_select_reads",
    "dskgpu_colors_begin", "dskgpu_colors_add", "dskgpu_colors_rows", "dskgpu_colors_unitigs",
    "dskgpu_colors_pairs", "dskgpu_colors_load", "dskgpu_colors_marks",
    "dskgpu_load_rows",
    "dskgpu_variants", "dskgpu_variants_table", "dskgpu_variants_stream",
    "dskgpu_k_encode", "dskgpu_k_enumerate", "dskgpu_k_minimizers",
    "dskgpu_group_create", "dskgpu_group_destroy", "dskgpu_group_last_error", "dskgpu_group_size", "dskgpu_group_ctx",
    "dskgpu_group_transport", "dskgpu_group_count", "dskgpu_group_exchanged_words", "dskgpu_group_sliced_steps", "dskgpu_group_histogram", "dskgpu_group_histogram2d",
    "dskgpu_group_get_stats", "dskgpu_group_num_partitions", "dskgpu_group_partition_size", "dskgpu_group_partition_copy",
]

_lib = None


SLICE_GATE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32)      # dskgpu_slice_gate: 0 = the stream waits for the slice, else the count stops


def _stats_dict(st) -> dict:
    """a stats structure of the library -> {field: int}, without the reserved words"""
    return {name: int(getattr(st, name)) for name, _ in st._fields_ if name != "reserved"}


def library_path() -> str:
    return os.environ.get("DSKGPU_LIB", os.path.join(_HERE, "libdskgpu.so"))


def load_library():
    """Load libdskgpu.so; fails loudly (no fallback) when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C dsk_amd/csrc` (there is no CPU fallback for the count path)")
    lib = C.CDLL(path)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    lib.dskgpu_create.argtypes = [C.POINTER(_Config), C.POINTER(vp)]
    lib.dskgpu_create.restype = C.c_int
    lib.dskgpu_destroy.argtypes = [vp]
    lib.dskgpu_destroy.restype = None
    lib.dskgpu_last_error.argtypes = [vp]
    lib.dskgpu_last_error.restype = C.c_char_p
    lib.dskgpu_version.argtypes = []
    lib.dskgpu_version.restype = C.c_char_p
    lib.dskgpu_set_stream.argtypes = [vp, vp]
    lib.dskgpu_push_reads.argtypes = [vp, vp, u64]
    lib.dskgpu_push_raw.argtypes = [vp, vp, u64, C.c_int, C.c_int]
    lib.dskgpu_raw_finish.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    lib.dskgpu_stream_bytes.argtypes = [vp, C.POINTER(u64)]
    lib.dskgpu_rewind_reads.argtypes = [vp, u64]
    lib.dskgpu_reserve_reads.argtypes = [vp, u64]
    lib.dskgpu_reserve_work.argtypes = [vp, u64]
    lib.dskgpu_set_reads_device.argtypes = [vp, vp, u64]
    lib.dskgpu_count.argtypes = [vp]
    lib.dskgpu_encode_reads.argtypes = [vp]
    lib.dskgpu_next_bank.argtypes = [vp]
    lib.dskgpu_set_banks.argtypes = [vp, C.POINTER(u64), u32]
    lib.dskgpu_histogram2d.argtypes = [vp, C.POINTER(u64), u32]
    lib.dskgpu_mg_scatter.argtypes = [vp, vp, u64, C.POINTER(u64)]
    lib.dskgpu_mg_sample.argtypes = [vp, C.POINTER(u64)]
    lib.dskgpu_mg_make_table.argtypes = [C.POINTER(u64), u32, C.POINTER(C.c_uint8)]
    lib.dskgpu_mg_make_table.restype = None
    lib.dskgpu_mg_set_table.argtypes = [vp, C.POINTER(C.c_uint8)]
    lib.dskgpu_mg_send_capacity_words.argtypes = [vp]
    lib.dskgpu_mg_send_capacity_words.restype = u64
    lib.dskgpu_mg_count.argtypes = [vp, vp, u64]
    lib.dskgpu_mg_sent_kmers.argtypes = [vp, C.POINTER(u64)]
    lib.dskgpu_mg_count_sized.argtypes = [vp, vp, u64, u64]
    lib.dskgpu_mg_slices_prepare.argtypes = [vp, u32, C.POINTER(u32), C.POINTER(u64), C.POINTER(u64)]
    lib.dskgpu_mg_scatter_slice.argtypes = [vp, vp, u64, u32]
    lib.dskgpu_mg_slices_finish.argtypes = [vp, C.POINTER(C.c_int)]
    lib.dskgpu_mg_count_sliced.argtypes = [vp, vp, u32, C.POINTER(u64), u64, SLICE_GATE, vp]
    lib.dskgpu_get_stats.argtypes = [vp, C.POINTER(_Stats)]
    lib.dskgpu_histogram.argtypes = [vp, C.POINTER(u64), u32]
    lib.dskgpu_num_partitions.argtypes = [vp]
    lib.dskgpu_num_partitions.restype = u32
    lib.dskgpu_set_row_order.argtypes = [vp, C.c_int]
    lib.dskgpu_partition_size.argtypes = [vp, u32]
    lib.dskgpu_partition_offsets.argtypes = [vp, vp]
    lib.dskgpu_partition_size.restype = u64
    lib.dskgpu_partition_copy.argtypes = [vp, u32, vp, vp]
    lib.dskgpu_result_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    lib.dskgpu_stage_times.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]
    lib.dskgpu_query_prepare.argtypes = [vp]
    lib.dskgpu_query_prepare.restype = C.c_int
    lib.dskgpu_query_kmers.argtypes = [vp, vp, u64, vp]
    lib.dskgpu_query_kmers.restype = C.c_int
    lib.dskgpu_query_reads.argtypes = [vp, vp, u64, vp]
    lib.dskgpu_query_reads.restype = C.c_int
    lib.dskgpu_graph_adjacency.argtypes = [vp, vp, C.POINTER(u64)]
    lib.dskgpu_graph_adjacency.restype = C.c_int
    lib.dskgpu_graph_neighbors.argtypes = [vp, vp, u64, vp]
    lib.dskgpu_graph_neighbors.restype = C.c_int
    lib.dskgpu_unitigs.argtypes = [vp, C.POINTER(_UnitigStats)]
    lib.dskgpu_unitigs.restype = C.c_int
    lib.dskgpu_unitigs_rows.argtypes = [vp, vp, vp]
    lib.dskgpu_unitigs_rows.restype = C.c_int
    lib.dskgpu_unitigs_table.argtypes = [vp, vp, vp, vp]
    lib.dskgpu_unitigs_table.restype = C.c_int
    lib.dskgpu_unitigs_stream.argtypes = [vp, vp, u64]
    lib.dskgpu_unitigs_stream.restype = C.c_int
    lib.dskgpu_unitig_edges.argtypes = [vp, C.POINTER(_UnitigEdgeStats)]
    lib.dskgpu_unitig_edges.restype = C.c_int
    lib.dskgpu_unitig_edges_table.argtypes = [vp, vp, vp, vp]
    lib.dskgpu_unitig_edges_table.restype = C.c_int
    lib.dskgpu_filter_rows.argtypes = [vp, vp, C.POINTER(u64)]
    lib.dskgpu_filter_rows.restype = C.c_int
    lib.dskgpu_graph_tips.argtypes = [vp, C.POINTER(_TipParams), vp, vp, C.POINTER(_TipStats)]
    lib.dskgpu_graph_tips.restype = C.c_int
    lib.dskgpu_clip_tips.argtypes = [vp, C.POINTER(_TipParams), C.POINTER(_TipStats)]
    lib.dskgpu_clip_tips.restype = C.c_int
    lib.dskgpu_graph_bubbles.argtypes = [vp, C.POINTER(_BubbleParams), vp, vp, C.POINTER(_BubbleStats)]
    lib.dskgpu_graph_bubbles.restype = C.c_int
    lib.dskgpu_pop_bubbles.argtypes = [vp, C.POINTER(_BubbleParams), C.POINTER(_BubbleStats)]
    lib.dskgpu_pop_bubbles.restype = C.c_int
    lib.dskgpu_simplify.argtypes = [vp, C.POINTER(_TipParams), C.POINTER(_BubbleParams), C.c_uint32, C.POINTER(_SimplifyStats)]
    lib.dskgpu_simplify.restype = C.c_int
    lib.dskgpu_graph_connections.argtypes = [vp, C.POINTER(_ConnectionParams), vp, vp, C.POINTER(_ConnectionStats)]
    lib.dskgpu_graph_connections.restype = C.c_int
    lib.dskgpu_remove_connections.argtypes = [vp, C.POINTER(_ConnectionParams), C.POINTER(_ConnectionStats)]
    lib.dskgpu_remove_connections.restype = C.c_int
    lib.dskgpu_simplify_all.argtypes = [vp, C.POINTER(_TipParams), C.POINTER(_BubbleParams), C.POINTER(_ConnectionParams), C.c_uint32,
                                        C.POINTER(_SimplifyAllStats)]
    lib.dskgpu_simplify_all.restype = C.c_int
    lib.dskgpu_components.argtypes = [vp, C.POINTER(_ComponentStats)]
    lib.dskgpu_components.restype = C.c_int
    lib.dskgpu_components_labels.argtypes = [vp, vp, vp]
    lib.dskgpu_components_labels.restype = C.c_int
    lib.dskgpu_components_table.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.dskgpu_components_table.restype = C.c_int
    lib.dskgpu_graph_small_components.argtypes = [vp, C.POINTER(_ComponentParams), vp, vp, C.POINTER(_ComponentDropStats)]
    lib.dskgpu_graph_small_components.restype = C.c_int
    lib.dskgpu_drop_components.argtypes = [vp, C.POINTER(_ComponentParams), C.POINTER(_ComponentDropStats)]
    lib.dskgpu_drop_components.restype = C.c_int
    lib.dskgpu_variants.argtypes = [vp, C.POINTER(_VariantParams), C.POINTER(_VariantStats)]
    lib.dskgpu_variants.restype = C.c_int
    lib.dskgpu_variants_table.argtypes = [vp, vp]
    lib.dskgpu_variants_table.restype = C.c_int
    lib.dskgpu_variants_stream.argtypes = [vp, vp, vp, u64]
    lib.dskgpu_variants_stream.restype = C.c_int
    lib.dskgpu_thread_place.argtypes = [vp, vp, u64, vp, vp]
    lib.dskgpu_thread_place.restype = C.c_int
    lib.dskgpu_thread_reads.argtypes = [vp, vp, u64, C.POINTER(_ThreadStats)]
    lib.dskgpu_thread_reads.restype = C.c_int
    lib.dskgpu_thread_walks.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.dskgpu_thread_walks.restype = C.c_int
    lib.dskgpu_thread_support.argtypes = [vp, vp, vp]
    lib.dskgpu_thread_support.restype = C.c_int
    lib.dskgpu_correct_reads.argtypes = [vp, vp, u64, C.POINTER(_CorrectParams), vp, vp, C.POINTER(_CorrectStats)]
    lib.dskgpu_correct_reads.restype = C.c_int
    lib.dskgpu_read_summaries.argtypes = [vp, vp, u64, C.POINTER(_ReadSummaryParams), C.POINTER(_ReadSummaryStats)]
    lib.dskgpu_read_summaries.restype = C.c_int
    lib.dskgpu_read_summaries_table.argtypes = [vp, vp]
    lib.dskgpu_read_summaries_table.restype = C.c_int
    lib.dskgpu_read_marks.argtypes = [vp, C.POINTER(_ReadRule), vp, C.POINTER(_ReadMarkStats)]
    lib.dskgpu_read_marks.restype = C.c_int
    lib.dskgpu_select_reads.argtypes = [vp, vp, u64, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    lib.dskgpu_select_reads.restype = C.c_int
    lib.dskgpu_colors_begin.argtypes = [vp, u32]
    lib.dskgpu_colors_begin.restype = C.c_int
    lib.dskgpu_colors_add.argtypes = [vp, vp, u64, C.POINTER(u64), u32, u32, C.POINTER(_ColorStats)]
    lib.dskgpu_colors_add.restype = C.c_int
    lib.dskgpu_colors_rows.argtypes = [vp, u32, vp, vp]
    lib.dskgpu_colors_rows.restype = C.c_int
    lib.dskgpu_colors_unitigs.argtypes = [vp, u32, vp, vp, vp]
    lib.dskgpu_colors_unitigs.restype = C.c_int
    lib.dskgpu_colors_pairs.argtypes = [vp, u32, vp, vp, vp, vp, C.POINTER(_ColorPairStats)]
    lib.dskgpu_colors_pairs.restype = C.c_int
    lib.dskgpu_colors_load.argtypes = [vp, vp, u32]
    lib.dskgpu_colors_load.restype = C.c_int
    lib.dskgpu_load_rows.argtypes = [vp, vp, vp, C.c_uint64, u32, C.POINTER(_LoadStats)]
    lib.dskgpu_load_rows.restype = C.c_int
    lib.dskgpu_colors_marks.argtypes = [vp, C.POINTER(_ColorRule), vp, C.POINTER(_ColorMarkStats)]
    lib.dskgpu_colors_marks.restype = C.c_int
    lib.dskgpu_k_encode.argtypes = [vp, vp, u64, vp, vp]
    lib.dskgpu_k_enumerate.argtypes = [vp, vp, u64, vp, vp]
    lib.dskgpu_k_minimizers.argtypes = [vp, vp, u64, vp, vp]
    lib.dskgpu_group_create.argtypes = [C.POINTER(_Config), C.POINTER(C.c_int32), u32, C.POINTER(vp)]
    lib.dskgpu_group_destroy.argtypes = [vp]
    lib.dskgpu_group_destroy.restype = None
    lib.dskgpu_group_last_error.argtypes = [vp]
    lib.dskgpu_group_last_error.restype = C.c_char_p
    lib.dskgpu_group_size.argtypes = [vp]
    lib.dskgpu_group_size.restype = u32
    lib.dskgpu_group_ctx.argtypes = [vp, u32]
    lib.dskgpu_group_ctx.restype = vp
    lib.dskgpu_group_transport.argtypes = [vp]
    lib.dskgpu_group_transport.restype = C.c_char_p
    lib.dskgpu_group_count.argtypes = [vp]
    lib.dskgpu_group_exchanged_words.argtypes = [vp]
    lib.dskgpu_group_exchanged_words.restype = u64
    lib.dskgpu_group_sliced_steps.argtypes = [vp]
    lib.dskgpu_group_sliced_steps.restype = u32
    lib.dskgpu_group_histogram.argtypes = [vp, C.POINTER(u64), u32]
    lib.dskgpu_group_histogram2d.argtypes = [vp, C.POINTER(u64), u32]
    lib.dskgpu_group_get_stats.argtypes = [vp, C.POINTER(_Stats)]
    lib.dskgpu_group_num_partitions.argtypes = [vp]
    lib.dskgpu_group_num_partitions.restype = u32
    lib.dskgpu_group_partition_size.argtypes = [vp, u32]
    lib.dskgpu_group_partition_size.restype = u64
    lib.dskgpu_group_partition_copy.argtypes = [vp, u32, vp, vp]
    for name in EXPORTS:          # every declared symbol must resolve (fails loudly on a stale build)
        getattr(lib, name)
    _lib = lib
    return lib


def _make_config(kmer_size, abundance_min, abundance_max, histo_max, device, nb_partitions, timing, sort, world_size, rank,
                 minimizer_size, max_pass_mkeys, solidity_kind, solidity_custom, histo2d, mg_explicit, place=False, partition_order=False) -> "_Config":
    cfg = _Config()
    cfg.kmer_size = kmer_size
    cfg.abundance_min = abundance_min
    cfg.abundance_max = abundance_max
    cfg.histo_max = histo_max
    cfg.device = device
    cfg.nb_partitions = nb_partitions
    cfg.minimizer_size = minimizer_size
    cfg.max_pass_mkeys = max_pass_mkeys
    cfg.flags = (F_TIMING if timing else 0) | (0 if sort else F_NO_SORT) | (F_HISTO2D if histo2d else 0) | (F_MG_EXPLICIT if mg_explicit else 0) | (F_PLACE if place else 0) | (F_PARTITION_ORDER if partition_order else 0)
    cfg.solidity_kind = SOLIDITY[solidity_kind]
    cfg.solidity_custom = solidity_custom
    cfg.world_size = world_size
    cfg.rank = rank
    return cfg


class KmerCounter:
    """One counting context on one GPU (not thread-safe; one per device)."""

    @classmethod
    def _borrowed(cls, handle, kmer_size: int, histo_max: int, world_size: int, device: int = 0) -> "KmerCounter":
        """A view of a ctx owned by somebody else (a KmerGroup rank): never destroyed from here."""
        self = cls.__new__(cls)
        self._lib = load_library()
        self._h = C.c_void_p(handle)
        self._owned = False
        self.device = device
        self.kmer_size, self.histo_max, self.world_size = kmer_size, histo_max, world_size
        self.words = (kmer_size + 31) // 32
        return self

    def __init__(self, kmer_size: int = 31, abundance_min: int = 2, abundance_max: int = 2147483647,
                 histo_max: int = 10000, device: int = 0, nb_partitions: int = 0, timing: bool = False,
                 sort: bool = True, world_size: int = 1, rank: int = 0, stream: Optional[int] = None,
                 minimizer_size: int = 0, max_pass_mkeys: int = 0, solidity_kind: str = "sum", solidity_custom: int = 0,
                 histo2d: bool = False, mg_explicit: bool = False, place: bool = False, partition_order: bool = False):
        """partition_order: DSKGPU_F_PARTITION_ORDER -- rows ascending inside every output partition only (the reference's Partition<Count>
        contract; thousands of small partitions), one pass over the rows instead of the three of the global order.  Honoured at every
        k up to 128: partitions of at most 4096 rows for k <= 32, 2048 for k <= 64, 1024 (PS4_CAP) for 65 <= k <= 128.
        place: DSKGPU_F_PLACE -- every big device buffer becomes the best-placed of 8 candidate allocations (one-off cost of a
        few seconds at the first count, steps ~6 % faster and no longer box- and process-dependent): for contexts that count often."""
        self._lib = load_library()
        self._owned = True
        cfg = _make_config(kmer_size, abundance_min, abundance_max, histo_max, device, nb_partitions, timing, sort, world_size, rank,
                           minimizer_size, max_pass_mkeys, solidity_kind, solidity_custom, histo2d, mg_explicit, place, partition_order)
        self.kmer_size = kmer_size
        self.histo_max = histo_max
        self.device = device
        self.words = (kmer_size + 31) // 32          # 64-bit words of a k-mer at the ABI (1..4)
        self.world_size = world_size
        h = C.c_void_p()
        rc = self._lib.dskgpu_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise DskGpuError(rc, self._lib.dskgpu_last_error(None).decode())
        self._h = h
        if stream is not None:
            self._ck(self._lib.dskgpu_set_stream(self._h, C.c_void_p(stream)))

    # -- plumbing
    def _ck(self, rc: int) -> None:
        if rc != 0:
            raise DskGpuError(rc, self._lib.dskgpu_last_error(self._h).decode())

    def close(self) -> None:
        if getattr(self, "_h", None):
            if getattr(self, "_owned", True):
                self._lib.dskgpu_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- input
    def push_reads(self, data) -> None:
        """data: bytes, or a C-contiguous uint8 numpy array (no copy)."""
        if isinstance(data, (bytes, bytearray)):
            buf = (C.c_char * len(data)).from_buffer_copy(data) if isinstance(data, bytes) else (C.c_char * len(data)).from_buffer(data)
            self._ck(self._lib.dskgpu_push_reads(self._h, C.addressof(buf), len(data)))
        else:
            arr = np.ascontiguousarray(data, dtype=np.uint8)
            self._ck(self._lib.dskgpu_push_reads(self._h, arr.ctypes.data, arr.size))

    RAW_FASTA, RAW_FASTQ = 1, 2

    def push_raw(self, text, fmt=None, new_file: bool = False) -> None:
        """FASTA / FASTQ text as it lies in the file (cut anywhere between calls): parsed on the device (dskgpu_push_raw).
        fmt: RAW_FASTA / RAW_FASTQ, or None = from the first byte ('>' / '@') of a text that starts a file."""
        arr = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
        if fmt is None:
            if arr.size == 0 or arr[0] not in (ord(">"), ord("@")):
                raise ValueError("push_raw: cannot tell the format from the first byte; pass fmt")
            fmt = self.RAW_FASTA if arr[0] == ord(">") else self.RAW_FASTQ
        self._ck(self._lib.dskgpu_push_raw(self._h, C.c_void_p(arr.ctypes.data if arr.size else 0), arr.size, int(fmt), int(bool(new_file))))

    def raw_finish(self):
        """-> (bytes of the read stream, records in the raw pushes since the last finish); raises DskGpuError(DSKGPU_E_FORMAT) when the text was not what
        the device parser handles (the raw pushes are dropped then: parse on the host and push_reads)."""
        nb, ln = C.c_uint64(0), C.c_uint64(0)
        self._ck(self._lib.dskgpu_raw_finish(self._h, C.byref(nb), C.byref(ln)))
        return nb.value, ln.value

    def stream_bytes(self) -> int:
        n = C.c_uint64(0)
        self._ck(self._lib.dskgpu_stream_bytes(self._h, C.byref(n)))
        return n.value

    def rewind_reads(self, stream_bytes: int) -> None:
        """Cut the pushed read stream back to its first stream_bytes bytes (dskgpu_rewind_reads)."""
        self._ck(self._lib.dskgpu_rewind_reads(self._h, stream_bytes))

    def reserve_reads(self, nbytes: int) -> None:
        self._ck(self._lib.dskgpu_reserve_reads(self._h, nbytes))

    def reserve_work(self, nbytes: int) -> bool:
        """-> False when the engine declined (DSKGPU_NOT_RESERVED: the request exceeds 60 % of the free HBM; count() sizes its own buffers)."""
        rc = self._lib.dskgpu_reserve_work(self._h, nbytes)
        if rc == 1:
            return False
        self._ck(rc)
        return True

    def set_reads_device(self, ptr: int, nbytes: int) -> None:
        self._ck(self._lib.dskgpu_set_reads_device(self._h, C.c_void_p(ptr), nbytes))

    def encode_reads(self) -> None:
        """Encode the current reads to their 2-bit form now and let go of the bytes: the buffer given to set_reads_device may be freed."""
        self._ck(self._lib.dskgpu_encode_reads(self._h))

    def next_bank(self) -> None:
        self._ck(self._lib.dskgpu_next_bank(self._h))

    def set_banks(self, end_offsets) -> None:
        arr = (C.c_uint64 * len(end_offsets))(*end_offsets)
        self._ck(self._lib.dskgpu_set_banks(self._h, arr, len(end_offsets)))

    def histogram2d(self) -> np.ndarray:
        out = np.zeros((self.histo_max + 1, 11), dtype=np.uint64)
        self._ck(self._lib.dskgpu_histogram2d(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), self.histo_max + 1))
        return out

    def set_stream(self, stream: Optional[int]) -> None:
        """All device work of this context on the given hipStream_t handle.  None or 0 = a stream owned by the context -- NOT the
        legacy default stream (whose handle is 0): to order the context against torch work, hand it a torch.cuda.Stream()."""
        self._ck(self._lib.dskgpu_set_stream(self._h, C.c_void_p(stream) if stream else None))

    # -- hot path
    def count(self) -> None:
        self._ck(self._lib.dskgpu_count(self._h))

    def mg_send_capacity_words(self) -> int:
        n = int(self._lib.dskgpu_mg_send_capacity_words(self._h))
        if n == 0:
            raise DskGpuError(-2, "dskgpu_mg_send_capacity_words: " + (self._lib.dskgpu_last_error(self._h) or b"").decode())
        return n

    def mg_scatter(self, send_ptr: int, capacity_words: int) -> List[int]:
        counts = (C.c_uint64 * self.world_size)()
        self._ck(self._lib.dskgpu_mg_scatter(self._h, C.c_void_p(send_ptr), capacity_words, counts))
        return [int(c) for c in counts]

    def mg_sample(self) -> np.ndarray:
        """Sampled k-mer load of this rank's reads per minimizer bucket (u64[MG_BUCKETS]); sum over ranks, then make_table."""
        loads = np.zeros(MG_BUCKETS, dtype=np.uint64)
        self._ck(self._lib.dskgpu_mg_sample(self._h, loads.ctypes.data_as(C.POINTER(C.c_uint64))))
        return loads

    def mg_set_table(self, table: Optional[np.ndarray]) -> None:
        if table is None:
            self._ck(self._lib.dskgpu_mg_set_table(self._h, None))
        else:
            t = np.ascontiguousarray(table, dtype=np.uint8)
            assert t.size == MG_BUCKETS
            self._ck(self._lib.dskgpu_mg_set_table(self._h, t.ctypes.data_as(C.POINTER(C.c_uint8))))

    def mg_sent_kmers(self) -> List[int]:
        """k-mers inside the records the last mg_scatter wrote for every owner (the receivers' sizing: see mg_count)."""
        k = (C.c_uint64 * self.world_size)()
        self._ck(self._lib.dskgpu_mg_sent_kmers(self._h, k))
        return [int(c) for c in k]

    # -- a step in slices (the exchange of slice i overlaps the sender of slice i + 1 and the receiver's level 1 of slice i - 1)
    def mg_slices_prepare(self, want_slices: int):
        """-> (nslices, send_words[nslices][world], kmers_est[world]); nslices == 0: this input takes the one-piece path."""
        n = C.c_uint32(0)
        words = (C.c_uint64 * (want_slices * self.world_size))()
        est = (C.c_uint64 * self.world_size)()
        self._ck(self._lib.dskgpu_mg_slices_prepare(self._h, want_slices, C.byref(n), words, est))
        ns = int(n.value)
        return ns, [[int(words[s * self.world_size + o]) for o in range(self.world_size)] for s in range(ns)], [int(x) for x in est]

    def mg_scatter_slice(self, send_ptr: int, capacity_words: int, s: int) -> None:
        """Launches the sender of slice s on the context's stream; returns without synchronising."""
        self._ck(self._lib.dskgpu_mg_scatter_slice(self._h, C.c_void_p(send_ptr), capacity_words, s))

    def mg_slices_finish(self) -> bool:
        """True when a slice of the send layout overflowed: every rank then repeats the step in one piece."""
        o = C.c_int(0)
        self._ck(self._lib.dskgpu_mg_slices_finish(self._h, C.byref(o)))
        return bool(o.value)

    def mg_count_sliced(self, recv_ptr: int, slice_words: Sequence[int], n_kmers_est: int, gate) -> None:
        """gate(s) is called right before the first device work that reads slice s is enqueued: make the stream wait for it."""
        arr = (C.c_uint64 * len(slice_words))(*[int(w) for w in slice_words])
        failed: list = []

        def _gate(_user, s):      # ctypes would print and swallow an exception raised in here: keep it, tell the C side, re-raise below
            try:
                gate(int(s))
                return 0
            except BaseException as e:      # noqa: BLE001 -- a failed wait (collective timeout / abort) must stop the count, whatever it is
                failed.append(e)
                return 1
        cb = SLICE_GATE(_gate)
        rc = self._lib.dskgpu_mg_count_sliced(self._h, C.c_void_p(recv_ptr), len(slice_words), arr, n_kmers_est, cb, None)
        if failed:
            raise failed[0]
        self._ck(rc)

    def mg_count(self, recv_ptr: int, recv_words: int, n_kmers: int = 0) -> None:
        """n_kmers = the senders' k-mer total for this rank (sum over sources of mg_sent_kmers()[rank]); 0 = count them here."""
        self._ck(self._lib.dskgpu_mg_count_sized(self._h, C.c_void_p(recv_ptr), recv_words, n_kmers))

    # -- results
    def stats(self) -> dict:
        s = _Stats()
        self._ck(self._lib.dskgpu_get_stats(self._h, C.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in _Stats._fields_ if k != "reserved"}

    def histogram(self) -> np.ndarray:
        out = np.zeros(self.histo_max + 1, dtype=np.uint64)
        self._ck(self._lib.dskgpu_histogram(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), self.histo_max + 1))
        return out

    def num_partitions(self) -> int:
        return int(self._lib.dskgpu_num_partitions(self._h))

    def partition(self, p: int) -> Tuple[np.ndarray, np.ndarray]:
        n = int(self._lib.dskgpu_partition_size(self._h, p))
        kmers = np.zeros((n, self.words), dtype=np.uint64)
        ab = np.zeros(n, dtype=np.uint32)
        self._ck(self._lib.dskgpu_partition_copy(self._h, p, C.c_void_p(kmers.ctypes.data), C.c_void_p(ab.ctypes.data)))
        return kmers, ab

    def set_row_order(self, partition_order: bool) -> None:
        self._ck(self._lib.dskgpu_set_row_order(self._h, 1 if partition_order else 0))

    def partition_offsets(self) -> np.ndarray:
        off = np.zeros(self.num_partitions() + 1, dtype=np.uint64)
        self._ck(self._lib.dskgpu_partition_offsets(self._h, C.c_void_p(off.ctypes.data)))
        return off

    def partition_sizes(self) -> np.ndarray:
        return np.diff(self.partition_offsets().astype(np.int64))

    def rows(self) -> Tuple[np.ndarray, np.ndarray]:
        """All solid rows, partitions concatenated in index order (what dsk2ascii walks)."""
        ks, abs_ = [], []
        for p in range(self.num_partitions()):
            k, a = self.partition(p)
            ks.append(k)
            abs_.append(a)
        if not ks:
            return np.zeros((0, self.words), np.uint64), np.zeros(0, np.uint32)
        return np.concatenate(ks), np.concatenate(abs_)

    def result_device(self) -> Tuple[int, int, int]:
        k, a, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._ck(self._lib.dskgpu_result_device(self._h, C.byref(k), C.byref(a), C.byref(n)))
        return int(k.value or 0), int(a.value or 0), int(n.value)

    def stage_times(self) -> List[Tuple[str, float]]:
        cap = 64
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        n = self._lib.dskgpu_stage_times(self._h, names, ms, cap)
        return [(names[i].decode(), float(ms[i])) for i in range(min(n, cap))]

    # -- lookups in the last result (include/dskgpu.h: dskgpu_query_*)
    def query_prepare(self) -> None:
        """Build the lookup index of the last result now (the first query after a count builds it otherwise)."""
        self._ck(self._lib.dskgpu_query_prepare(self._h))

    def query_kmers(self, d_kmers: int, n: int, d_out: int) -> None:
        """d_kmers: n values of `words` u64 each on the device (LSW first); d_out: n u32 on the device <- abundance, 0 = not a solid row."""
        self._ck(self._lib.dskgpu_query_kmers(self._h, C.c_void_p(d_kmers), n, C.c_void_p(d_out)))

    def query_reads(self, d_bytes: int, nbytes: int, d_out: int) -> None:
        """d_bytes: a read stream on the device; d_out: nbytes u32 on the device <- abundance of the k-mer of the window ending at every byte, or 0."""
        self._ck(self._lib.dskgpu_query_reads(self._h, C.c_void_p(d_bytes), nbytes, C.c_void_p(d_out)))

    def query_kmers_tensor(self, kmers):
        """kmers: CUDA tensor of n x `words` 64-bit values (int64 or uint64 bit patterns, LSW first; a 1-D tensor for words == 1).
        -> int32 tensor of n abundances, to be viewed as u32 (.view(torch.uint32))."""
        import torch
        if not kmers.is_cuda or kmers.element_size() != 8:
            raise ValueError("query_kmers_tensor: a CUDA tensor of 64-bit words is needed")
        kmers = kmers.contiguous()
        if kmers.numel() % self.words:
            raise ValueError("query_kmers_tensor: %d words are not whole values of %d words" % (kmers.numel(), self.words))
        n = kmers.numel() // self.words
        out = torch.zeros(n, dtype=torch.int32, device=kmers.device)
        torch.cuda.current_stream(kmers.device).synchronize()      # the context's stream is not torch's: what torch enqueued is done before the lookup reads it
        self.query_kmers(kmers.data_ptr(), n, out.data_ptr())
        return out

    def query_reads_tensor(self, stream):
        """stream: CUDA uint8 tensor holding a read stream.  -> int32 tensor, one abundance per byte (view as u32), 0 = no valid window / not a solid row."""
        import torch
        if not stream.is_cuda or stream.dtype != torch.uint8:
            raise ValueError("query_reads_tensor: a CUDA uint8 tensor is needed")
        stream = stream.contiguous()
        out = torch.zeros(stream.numel(), dtype=torch.int32, device=stream.device)
        torch.cuda.current_stream(stream.device).synchronize()
        self.query_reads(stream.data_ptr(), stream.numel(), out.data_ptr())
        return out

    # -- the rows' de Bruijn neighbours (include/dskgpu.h: dskgpu_graph_*)
    def graph_adjacency(self, d_adj: int = 0) -> np.ndarray:
        """d_adj: n_rows bytes on the device (result order) <- bit b: successor b of the row is a row, bit 4 + b: predecessor b is; 0 = only
        the degree table.  -> uint64[5, 5], [i, o] = rows with i predecessors and o successors."""
        deg = np.zeros((5, 5), dtype=np.uint64)
        self._ck(self._lib.dskgpu_graph_adjacency(self._h, C.c_void_p(d_adj) if d_adj else None, deg.ctypes.data_as(C.POINTER(C.c_uint64))))
        return deg

    def graph_adjacency_tensor(self):
        """-> (uint8 CUDA tensor of n_rows adjacency bytes in result order, the degree table of graph_adjacency)."""
        import torch
        n = self.result_device()[2]
        out = torch.zeros(n, dtype=torch.uint8, device=torch.device("cuda", self.device))
        torch.cuda.current_stream(out.device).synchronize()       # the context's stream is not torch's: the zero fill is done before the kernel writes
        return out, self.graph_adjacency(out.data_ptr())

    def graph_neighbors(self, d_kmers: int, n: int, d_adj: int) -> None:
        """d_kmers: n values of `words` u64 each on the device (LSW first), canonical or not; d_adj: n bytes on the device <- their adjacency bytes."""
        self._ck(self._lib.dskgpu_graph_neighbors(self._h, C.c_void_p(d_kmers), n, C.c_void_p(d_adj)))

    def graph_neighbors_tensor(self, kmers):
        """kmers: CUDA tensor of n x `words` 64-bit values (as query_kmers_tensor takes them).  -> uint8 tensor of n adjacency bytes."""
        import torch
        if not kmers.is_cuda or kmers.element_size() != 8:
            raise ValueError("graph_neighbors_tensor: a CUDA tensor of 64-bit words is needed")
        kmers = kmers.contiguous()
        if kmers.numel() % self.words:
            raise ValueError("graph_neighbors_tensor: %d words are not whole values of %d words" % (kmers.numel(), self.words))
        n = kmers.numel() // self.words
        out = torch.zeros(n, dtype=torch.uint8, device=kmers.device)
        torch.cuda.current_stream(kmers.device).synchronize()
        self.graph_neighbors(kmers.data_ptr(), n, out.data_ptr())
        return out

    # -- the rows' de Bruijn graph compacted into unitigs (include/dskgpu.h: dskgpu_unitigs*)
    def unitigs(self) -> dict:
        """Build the compaction of the last result (the first of these calls after a count does) -> its stats: n_unitigs, n_cycles, n_single,
        max_nodes, stream_bytes, n_rounds."""
        st = _UnitigStats()
        self._ck(self._lib.dskgpu_unitigs(self._h, C.byref(st)))
        return _stats_dict(st)

    def unitigs_rows(self, d_unitig: int, d_pos: int) -> None:
        """d_unitig / d_pos: n_rows u32 each on the device (result order) <- the row's unitig / (position << 1) | orientation; either may be 0."""
        self._ck(self._lib.dskgpu_unitigs_rows(self._h, C.c_void_p(d_unitig) if d_unitig else None, C.c_void_p(d_pos) if d_pos else None))

    def unitigs_table(self, d_offsets: int, d_ab_sum: int, d_kind: int) -> None:
        """d_offsets: n_unitigs + 1 u64, d_ab_sum: n_unitigs u64, d_kind: n_unitigs bytes, all on the device; any may be 0."""
        self._ck(self._lib.dskgpu_unitigs_table(self._h, *(C.c_void_p(p) if p else None for p in (d_offsets, d_ab_sum, d_kind))))

    def unitigs_stream(self, d_bytes: int, capacity: int) -> None:
        """d_bytes: `capacity` >= stream_bytes bytes on the device <- the unitig sequences, each followed by a newline."""
        self._ck(self._lib.dskgpu_unitigs_stream(self._h, C.c_void_p(d_bytes) if d_bytes else None, capacity))

    def unitigs_rows_tensor(self):
        """-> (int32[n_rows] unitig of every row, int32[n_rows] (position << 1) | orientation), CUDA tensors in result order."""
        import torch
        self.unitigs()
        n = self.result_device()[2]
        dev = torch.device("cuda", self.device)
        unitig, pos = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()              # the context's stream is not torch's: the zero fill is done before the copies write
        if n:
            self.unitigs_rows(unitig.data_ptr(), pos.data_ptr())
        return unitig, pos

    def unitigs_table_tensor(self):
        """-> (int64[n_unitigs + 1] stream offsets, int64[n_unitigs] abundance sums, uint8[n_unitigs] kind: 1 = cycle), CUDA tensors."""
        import torch
        nu = self.unitigs()["n_unitigs"]
        dev = torch.device("cuda", self.device)
        off, ab = torch.zeros(nu + 1, dtype=torch.int64, device=dev), torch.zeros(nu, dtype=torch.int64, device=dev)
        kind = torch.zeros(nu, dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        self.unitigs_table(off.data_ptr(), ab.data_ptr() if nu else 0, kind.data_ptr() if nu else 0)
        return off, ab, kind

    def unitigs_stream_tensor(self):
        """-> uint8[stream_bytes] CUDA tensor: the unitig stream, a read stream that set_reads_device takes."""
        import torch
        nb = self.unitigs()["stream_bytes"]
        out = torch.zeros(nb, dtype=torch.uint8, device=torch.device("cuda", self.device))
        torch.cuda.current_stream(out.device).synchronize()
        if nb:
            self.unitigs_stream(out.data_ptr(), nb)
        return out

    # -- the edges between the unitigs (include/dskgpu.h: dskgpu_unitig_edges*)
    def unitig_edges(self) -> dict:
        """Build the edges between the oriented unitigs U = 2 u + t of the last result (the first of these calls after a count does, with
        the compaction below them) -> their stats: n_edges, n_self, n_dead_ends, max_degree."""
        st = _UnitigEdgeStats()
        self._ck(self._lib.dskgpu_unitig_edges(self._h, C.byref(st)))
        return _stats_dict(st)

    def unitig_edges_table(self, d_offsets: int, d_targets: int, d_ends: int) -> None:
        """d_offsets: 2 * n_unitigs + 1 u64 (CSR), d_targets: n_edges u32 (the oriented unitigs V), d_ends: 2 * n_unitigs u32 (last(U) as an
        oriented node 2 r + s), all on the device; any may be 0."""
        self._ck(self._lib.dskgpu_unitig_edges_table(self._h, *(C.c_void_p(p) if p else None for p in (d_offsets, d_targets, d_ends))))

    def unitig_edges_tensor(self):
        """-> (int64[2 * n_unitigs + 1] CSR offsets, int32[n_edges] targets V, int32[2 * n_unitigs] last nodes), CUDA tensors."""
        import torch
        ne = self.unitig_edges()["n_edges"]
        n_or = 2 * self.unitigs()["n_unitigs"]
        dev = torch.device("cuda", self.device)
        off = torch.zeros(n_or + 1, dtype=torch.int64, device=dev)
        targets, ends = torch.zeros(ne, dtype=torch.int32, device=dev), torch.zeros(n_or, dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()              # the context's stream is not torch's: the zero fill is done before the copies write
        self.unitig_edges_table(off.data_ptr(), targets.data_ptr() if ne else 0, ends.data_ptr() if n_or else 0)
        return off, targets, ends

    def write_gfa(self, path: str) -> dict:
        """The compacted graph of the last result as GFA 1: one S line per unitig (LN = letters, KC = sum of the member rows' abundances),
        one L line per edge U -> V with the overlap of k - 1 letters.  Plumbing on the host over the stream, the table and the edges.
        -> dict(n_segments, n_links)."""
        text = bytes(self.unitigs_stream_tensor().cpu().numpy())
        ab_sum = self.unitigs_table_tensor()[1].cpu().numpy()
        off, targets, _ = (t.cpu().numpy() for t in self.unitig_edges_tensor())
        seqs = text.decode().split("\n")[:-1]
        assert len(seqs) == len(ab_sum)
        overlap = "%dM" % (self.kmer_size - 1)
        with open(path, "w") as f:
            f.write("H\tVN:Z:1.0\n")
            for u, seq in enumerate(seqs):
                f.write("S\t%d\t%s\tLN:i:%d\tKC:i:%d\n" % (u, seq, len(seq), int(ab_sum[u])))
            for U in range(2 * len(seqs)):
                for V in targets[off[U]: off[U + 1]]:
                    f.write("L\t%d\t%s\t%d\t%s\t%s\n" % (U >> 1, "-" if U & 1 else "+", int(V) >> 1, "-" if int(V) & 1 else "+", overlap))
        return {"n_segments": len(seqs), "n_links": int(len(targets))}

    # -- reads threaded through the compacted graph (include/dskgpu.h: dskgpu_thread_*)
    def thread_place(self, d_bytes: int, nbytes: int, d_unitig: int, d_off: int) -> None:
        """d_bytes: a read stream on the device; d_unitig / d_off: nbytes u32 each on the device <- the oriented unitig U(p) = 2 u + t and the
        offset j(p) of the window ending at every byte, 0xFFFFFFFF / 0 where the window is not placed; either may be 0."""
        self._ck(self._lib.dskgpu_thread_place(self._h, C.c_void_p(d_bytes) if d_bytes else None, nbytes, C.c_void_p(d_unitig) if d_unitig else None,
                                               C.c_void_p(d_off) if d_off else None))

    def thread_reads(self, d_bytes: int, nbytes: int) -> dict:
        """Thread the stream through the compacted graph of the last result and keep the walks and the supports in the context -> the stats:
        n_valid, n_placed, n_walks, n_steps, max_steps."""
        st = _ThreadStats()
        self._ck(self._lib.dskgpu_thread_reads(self._h, C.c_void_p(d_bytes) if d_bytes else None, nbytes, C.byref(st)))
        self._thread_stats = _stats_dict(st)
        return dict(self._thread_stats)

    def thread_walks(self, d_offsets: int, d_steps: int, d_first: int, d_last: int, d_ends: int) -> None:
        """d_offsets: n_walks + 1 u64 (CSR into the steps), d_steps: n_steps u32, d_first / d_last: n_walks u64, d_ends: 2 * n_walks u32
        (j(first), j(last)), all on the device; any may be 0."""
        self._ck(self._lib.dskgpu_thread_walks(self._h, *(C.c_void_p(p) if p else None for p in (d_offsets, d_steps, d_first, d_last, d_ends))))

    def thread_support(self, d_unitig_support: int, d_edge_support: int) -> None:
        """d_unitig_support: n_unitigs u64, d_edge_support: n_edges u64 (the entries of unitig_edges_table), on the device; either may be 0."""
        self._ck(self._lib.dskgpu_thread_support(self._h, *(C.c_void_p(p) if p else None for p in (d_unitig_support, d_edge_support))))

    def thread_place_tensor(self, stream):
        """stream: CUDA uint8 tensor holding a read stream.  -> (int32[nbytes] U(p), int32[nbytes] j(p)); -1 / 0 where the window is not placed."""
        import torch
        if not stream.is_cuda or stream.dtype != torch.uint8:
            raise ValueError("thread_place_tensor: a CUDA uint8 tensor is needed")
        stream = stream.contiguous()
        n = stream.numel()
        U, j = torch.full((n,), -1, dtype=torch.int32, device=stream.device), torch.zeros(n, dtype=torch.int32, device=stream.device)
        torch.cuda.current_stream(stream.device).synchronize()      # the context's stream is not torch's: what torch enqueued is done before the kernel runs
        self.thread_place(stream.data_ptr() if n else 0, n, U.data_ptr() if n else 0, j.data_ptr() if n else 0)
        return U, j

    def thread_reads_tensor(self, stream) -> dict:
        """stream: CUDA uint8 tensor holding a read stream.  -> the stats of thread_reads; the tables: thread_walks_tensor, thread_support_tensor."""
        import torch
        if not stream.is_cuda or stream.dtype != torch.uint8:
            raise ValueError("thread_reads_tensor: a CUDA uint8 tensor is needed")
        stream = stream.contiguous()
        torch.cuda.current_stream(stream.device).synchronize()
        return self.thread_reads(stream.data_ptr() if stream.numel() else 0, stream.numel())

    def thread_walks_tensor(self):
        """-> (int64[n_walks + 1] CSR offsets, int32[n_steps] oriented unitigs, int64[n_walks] first, int64[n_walks] last,
        int32[n_walks, 2] (j(first), j(last))), CUDA tensors, of the threading the last thread_reads of this object kept (its stats size
        the tensors; when the library has dropped the threading since, the call raises DSKGPU_E_STATE)."""
        import torch
        st = getattr(self, "_thread_stats", None) or {"n_walks": 0, "n_steps": 0}
        nw, ns = st["n_walks"], st["n_steps"]
        dev = torch.device("cuda", self.device)
        off, steps = torch.zeros(nw + 1, dtype=torch.int64, device=dev), torch.zeros(ns, dtype=torch.int32, device=dev)
        first, last = torch.zeros(nw, dtype=torch.int64, device=dev), torch.zeros(nw, dtype=torch.int64, device=dev)
        ends = torch.zeros((nw, 2), dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()              # the context's stream is not torch's: the zero fill is done before the copies write
        self.thread_walks(off.data_ptr(), steps.data_ptr() if ns else 0, first.data_ptr() if nw else 0, last.data_ptr() if nw else 0,
                          ends.data_ptr() if nw else 0)
        return off, steps, first, last, ends

    def thread_support_tensor(self):
        """-> (int64[n_unitigs] placed positions per unitig, int64[n_edges] edge steps per entry of unitig_edges_tensor's table), CUDA tensors."""
        import torch
        ne = self.unitig_edges()["n_edges"]
        nu = self.unitigs()["n_unitigs"]
        dev = torch.device("cuda", self.device)
        usup, esup = torch.zeros(max(nu, 1), dtype=torch.int64, device=dev), torch.zeros(max(ne, 1), dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        self.thread_support(usup.data_ptr(), esup.data_ptr())
        return usup[:nu], esup[:ne]

    def write_gfa_walks(self, path: str) -> dict:
        """write_gfa, followed by one P line per walk of the kept threading: P <TAB> w<i> <TAB> <u>+,<u>-,... <TAB> *.
        -> dict(n_segments, n_links, n_paths)."""
        out = self.write_gfa(path)
        off, steps, _, _, _ = (t.cpu().numpy() for t in self.thread_walks_tensor())
        with open(path, "a") as f:
            for w in range(len(off) - 1):
                f.write("P\tw%d\t%s\t*\n" % (w, ",".join("%d%s" % (int(U) >> 1, "-" if int(U) & 1 else "+") for U in steps[off[w]: off[w + 1]])))
        out["n_paths"] = int(len(off) - 1)
        return out

    # -- substitution errors in reads corrected against the result (include/dskgpu.h: dskgpu_correct_reads)
    def correct_reads(self, d_bytes: int, nbytes: int, d_out: int = 0, d_state: int = 0, trust_min: int = 0) -> dict:
        """d_bytes: a read stream on the device.  d_out: nbytes u8 on the device <- the stream with every corrected byte replaced (may equal
        d_bytes: in place; 0: a dry run).  d_state: nbytes u8 <- 0 / 1 / 2 = no valid window / not trusted / trusted at every byte of the
        INPUT; may be 0.  trust_min: the abundance from which a row is trusted (0, 1: any row).  One substitution per gap of k untrusted
        windows; nothing else is corrected.  -> the stats: n_valid, n_trusted, n_gaps, n_interior, n_head, n_tail, n_skipped, n_corrected,
        n_ambiguous, n_unfixable."""
        par, st = _CorrectParams(trust_min=trust_min), _CorrectStats()
        self._ck(self._lib.dskgpu_correct_reads(self._h, C.c_void_p(d_bytes) if d_bytes else None, nbytes, C.byref(par), C.c_void_p(d_out) if d_out else None,
                                                C.c_void_p(d_state) if d_state else None, C.byref(st)))
        return _stats_dict(st)

    def correct_reads_tensor(self, t, trust_min: int = 0, want_state: bool = False):
        """t: CUDA uint8 tensor holding a read stream (left as it is).  -> (uint8[nbytes] the corrected stream, the stats of correct_reads
        [, uint8[nbytes] the states of the input])."""
        import torch
        if not t.is_cuda or t.dtype != torch.uint8:
            raise ValueError("correct_reads_tensor: a CUDA uint8 tensor is needed")
        t = t.contiguous()
        n = t.numel()
        out = torch.empty_like(t)
        state = torch.zeros(n, dtype=torch.uint8, device=t.device) if want_state else None
        torch.cuda.current_stream(t.device).synchronize()          # the context's stream is not torch's: what torch enqueued is done before the kernels run
        st = self.correct_reads(t.data_ptr() if n else 0, n, out.data_ptr() if n else 0, state.data_ptr() if want_state and n else 0, trust_min)
        return (out, st, state) if want_state else (out, st)

    # -- per-read abundance summaries and read selection (include/dskgpu.h: dskgpu_read_summaries / _read_summaries_table / _read_marks / dskgpu_select_reads)
    def read_summaries(self, d_bytes: int, nbytes: int, trust_min: int = 0) -> dict:
        """d_bytes: a read stream on the device.  Builds the summary of every record (what lies between two newlines) against the last
        result and keeps the table in the context until the rows change.  trust_min: the abundance from which a position is solid (0, 1:
        any row).  -> the stats: n_records, n_empty (no valid window), n_valid, n_solid, max_len."""
        par, st = _ReadSummaryParams(trust_min=trust_min), _ReadSummaryStats()
        self._ck(self._lib.dskgpu_read_summaries(self._h, C.c_void_p(d_bytes) if d_bytes else None, nbytes, C.byref(par), C.byref(st)))
        self._read_summary_stats = _stats_dict(st)
        return dict(self._read_summary_stats)

    def read_summaries_table(self, d_records: int) -> None:
        """d_records: 32 * n_records bytes on the device <- start u64, sum u64, len, n_valid, n_solid, median u32 of every record of the
        kept table (READ_SUMMARY_DTYPE)."""
        self._ck(self._lib.dskgpu_read_summaries_table(self._h, C.c_void_p(d_records) if d_records else None))

    def read_summaries_numpy(self) -> np.ndarray:
        """-> the kept table as a numpy array of READ_SUMMARY_DTYPE, one element per record of the stream the last read_summaries() of this
        object took (when the library has dropped the table since, the call raises DSKGPU_E_STATE)."""
        import torch
        n = (getattr(self, "_read_summary_stats", None) or {"n_records": 0})["n_records"]
        dev = torch.device("cuda", self.device)
        rec = torch.zeros((max(n, 1), 4), dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()              # the context's stream is not torch's: the zero fill is done before the copy writes
        self.read_summaries_table(rec.data_ptr())
        return rec[:n].cpu().numpy().view(READ_SUMMARY_DTYPE).reshape(n).copy()

    def read_marks(self, d_keep: int = 0, min_valid: int = 0, median_min: int = 0, median_max: int = 0, solid_num: int = 0, solid_den: int = 0,
                   invert: bool = False) -> dict:
        """The rule applied to the kept table: a record is kept when n_valid >= min_valid, median >= median_min, median <= median_max
        (0: no upper bound) and n_solid / n_valid >= solid_num / solid_den (solid_den 0: no bound); invert flips the answer.  d_keep:
        n_records bytes on the device <- 1 or 0; 0: the stats only.  -> the stats: n_records, n_kept, kept_bytes (the bytes of the
        selection by these marks), kept_valid."""
        rule, st = _ReadRule(min_valid=min_valid, median_min=median_min, median_max=median_max, solid_num=solid_num, solid_den=solid_den,
                             flags=READS_INVERT if invert else 0), _ReadMarkStats()
        self._ck(self._lib.dskgpu_read_marks(self._h, C.byref(rule), C.c_void_p(d_keep) if d_keep else None, C.byref(st)))
        return _stats_dict(st)

    def select_reads(self, d_bytes: int, nbytes: int, d_keep: int, n_records: int, d_out: int = 0, capacity: int = 0) -> Tuple[int, int]:
        """The records of the stream whose byte in d_keep (n_records of them, on the device) is non-zero -> d_out, in stream order, each with
        one newline behind it.  d_out 0: a sizing run.  Stateless: no result is needed.  -> (out_bytes, out_records)."""
        ob, orec = C.c_uint64(0), C.c_uint64(0)
        self._ck(self._lib.dskgpu_select_reads(self._h, C.c_void_p(d_bytes) if d_bytes else None, nbytes, C.c_void_p(d_keep) if d_keep else None, n_records,
                                               C.c_void_p(d_out) if d_out else None, capacity, C.byref(ob), C.byref(orec)))
        return int(ob.value), int(orec.value)

    def select_reads_tensor(self, stream, keep):
        """stream: CUDA uint8 tensor holding a read stream; keep: CUDA uint8 (or bool) tensor, one element per record, non-zero = keep.
        A sizing run, one allocation, the selection.  -> uint8[out_bytes], the kept records."""
        import torch
        if not stream.is_cuda or stream.dtype != torch.uint8 or not keep.is_cuda or keep.dtype not in (torch.uint8, torch.bool):
            raise ValueError("select_reads_tensor: CUDA tensors are needed, uint8 for the stream and uint8 or bool for the flags")
        stream, keep = stream.contiguous(), keep.contiguous().view(torch.uint8)
        n, nr = stream.numel(), keep.numel()
        torch.cuda.current_stream(stream.device).synchronize()    # the context's stream is not torch's: what torch enqueued is done before the kernels run
        args = (stream.data_ptr() if n else 0, n, keep.data_ptr() if nr else 0, nr)
        need, _ = self.select_reads(*args)
        out = torch.empty(need, dtype=torch.uint8, device=stream.device)
        if need:
            torch.cuda.current_stream(stream.device).synchronize()
            self.select_reads(*args, out.data_ptr(), need)
        return out

    # -- sample colours for rows, unitigs and variants (include/dskgpu.h: dskgpu_colors_begin / _colors_add / _colors_rows / _colors_unitigs)
    def colors_begin(self, n_colors: int) -> None:
        """A zeroed colour matrix u32[n_rows, n_colors] (n_colors 1..64) for the last result, kept in the context until the rows change;
        it replaces the one kept before."""
        self._ck(self._lib.dskgpu_colors_begin(self._h, n_colors))
        self._n_colors = n_colors

    def colors_add(self, d_bytes: int, nbytes: int, ends, first_color: int = 0) -> dict:
        """d_bytes: a read stream on the device; ends: the end offset of every bank of it (non-decreasing, the last <= nbytes).  Every valid
        window whose canonical k-mer is a row adds 1 to that row's cell of colour first_color + (the bank of the byte the window ends at).
        -> the stats of this call: n_valid (valid windows that have a bank), n_placed (those that are rows), n_rows, n_colors."""
        e = np.ascontiguousarray(ends, dtype=np.uint64).reshape(-1)
        st = _ColorStats()
        self._ck(self._lib.dskgpu_colors_add(self._h, C.c_void_p(d_bytes) if d_bytes else None, nbytes, e.ctypes.data_as(C.POINTER(C.c_uint64)) if len(e) else None,
                                             len(e), first_color, C.byref(st)))
        return _stats_dict(st)

    def colors_add_tensor(self, stream, ends, first_color: int = 0) -> dict:
        """stream: CUDA uint8 tensor holding a read stream; as colors_add."""
        import torch
        if not stream.is_cuda or stream.dtype != torch.uint8:
            raise ValueError("colors_add_tensor: a CUDA uint8 tensor is needed")
        stream = stream.contiguous()
        n = stream.numel()
        torch.cuda.current_stream(stream.device).synchronize()    # the context's stream is not torch's: what torch enqueued is done before the kernels read it
        return self.colors_add(stream.data_ptr() if n else 0, n, ends, first_color)

    def colors_rows(self, min_count: int, d_counts: int, d_mask: int) -> None:
        """d_counts: n_rows * n_colors u32 on the device (result order, row-major) <- the matrix; d_mask: n_rows u64 <- bit c: the cell of
        colour c is >= min_count; either may be 0."""
        self._ck(self._lib.dskgpu_colors_rows(self._h, min_count, C.c_void_p(d_counts) if d_counts else None, C.c_void_p(d_mask) if d_mask else None))

    def _colors_shape(self):
        self.colors_add(0, 0, [])                                 # an empty stream does nothing: DSKGPU_E_STATE when no matrix is kept
        return self.result_device()[2], self._n_colors

    def colors_rows_tensor(self, min_count: int = 1):
        """-> (int32[n_rows, n_colors] the matrix, to be viewed as u32; int64[n_rows] the masks, the bit pattern of a u64), CUDA tensors."""
        import torch
        n, nc = self._colors_shape()
        dev = torch.device("cuda", self.device)
        counts, mask = torch.zeros((n, nc), dtype=torch.int32, device=dev), torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()              # the context's stream is not torch's: the zero fill is done before the copy writes
        self.colors_rows(min_count, counts.data_ptr() if n else 0, mask.data_ptr())
        return counts, mask[:n]

    def colors_unitigs(self, min_count: int, d_sum: int, d_all: int, d_any: int) -> None:
        """d_sum: n_unitigs * n_colors u64 on the device <- the sum of every colour over the rows of every unitig; d_all / d_any: n_unitigs
        u64 <- the AND / the OR of the masks (min_count) of its rows; any may be 0.  Builds the compaction when it is not there."""
        self._ck(self._lib.dskgpu_colors_unitigs(self._h, min_count, *(C.c_void_p(p) if p else None for p in (d_sum, d_all, d_any))))

    def colors_unitigs_tensor(self, min_count: int = 1):
        """-> (int64[n_unitigs, n_colors] sums, int64[n_unitigs] all, int64[n_unitigs] any: the bit patterns of u64), CUDA tensors."""
        import torch
        _, nc = self._colors_shape()
        nu = self.unitigs()["n_unitigs"]
        dev = torch.device("cuda", self.device)
        total = torch.zeros((nu, nc), dtype=torch.int64, device=dev)
        all_, any_ = torch.zeros(max(nu, 1), dtype=torch.int64, device=dev), torch.zeros(max(nu, 1), dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        self.colors_unitigs(min_count, total.data_ptr() if nu else 0, all_.data_ptr(), any_.data_ptr())
        return total, all_[:nu], any_[:nu]

    def variants_colors_tensor(self, min_count: int = 1):
        """-> int64[n_variants, 2, n_colors]: for every kept variant (variants() first) the colour sums of the unitig of allele A and of
        allele B -- per-sample allele coverage.  A gather from colors_unitigs_tensor over the variant table."""
        total, _, _ = self.colors_unitigs_tensor(min_count)
        rec = self.variants_tensor()
        return total[rec[:, :2] >> 1]

    # -- the samples compared with each other, rows chosen by colour, a matrix put back (include/dskgpu.h: dskgpu_colors_pairs / _colors_load / _colors_marks)
    def colors_load(self, ptr: int, n_colors: int) -> None:
        """ptr: n_rows * n_colors u32 on the device (result order, row-major), 4-byte aligned -> a copy of it is the kept colour matrix of the
        last result, as if colors_begin and colors_add had built it; it replaces the one kept before."""
        self._ck(self._lib.dskgpu_colors_load(self._h, C.c_void_p(ptr) if ptr else None, n_colors))
        self._n_colors = n_colors

    def colors_load_tensor(self, t) -> None:
        """t: CUDA int32 tensor [n_rows, n_colors] (the bit patterns of u32, what colors_rows_tensor returns); as colors_load."""
        import torch
        if not t.is_cuda or t.dtype != torch.int32 or t.dim() != 2:
            raise ValueError("colors_load_tensor: a CUDA int32 tensor [n_rows, n_colors] is needed")
        n = self.result_device()[2]
        if t.shape[0] != n:
            raise ValueError("colors_load_tensor: %d rows for a result of %d" % (t.shape[0], n))
        t = t.contiguous()
        torch.cuda.current_stream(t.device).synchronize()         # the context's stream is not torch's: the matrix is written before the copy reads it
        self.colors_load(t.data_ptr() if n else 0, int(t.shape[1]))

    # -- saved rows loaded into the context, counts merged (include/dskgpu.h: dskgpu_load_rows)
    def load_rows(self, d_kmers: int, d_abundance: int, n: int, combine: str = "sum") -> dict:
        """d_kmers: n values of `words` u64 each on the device (row-major, LSW first, 8-byte aligned); d_abundance: n u32 on the device; any
        order, any repeats, not memory of this context.  The rows become the result as if a count had found them: equal values combined
        (combine: "sum", "max", "min", or "unique" = a repeat is an error), filtered by abundance_min / abundance_max, in the global order.
        -> the load's stats (n_in, n_distinct, n_rows, n_below, n_above, n_kmers, n_saturated, sorted_input)."""
        if combine not in LOAD_COMBINE:
            raise ValueError("load_rows: combine must be one of %s" % ", ".join(LOAD_COMBINE))
        st = _LoadStats()
        self._ck(self._lib.dskgpu_load_rows(self._h, C.c_void_p(d_kmers) if d_kmers else None, C.c_void_p(d_abundance) if d_abundance else None,
                                            n, LOAD_COMBINE[combine], C.byref(st)))
        self._n_colors = 0
        return _stats_dict(st)

    def load_rows_tensor(self, kmers, abundance, combine: str = "sum") -> dict:
        """kmers: CUDA tensor [n, words] of 64-bit values (int64 or uint64 bit patterns, LSW first; [n] for words == 1); abundance: CUDA tensor
        [n] of 32-bit values (int32 or uint32 bit patterns), both on the context's device; as load_rows."""
        import torch
        if not kmers.is_cuda or kmers.element_size() != 8 or not abundance.is_cuda or abundance.element_size() != 4 or abundance.is_floating_point() or kmers.is_floating_point():
            raise ValueError("load_rows_tensor: CUDA tensors of 64-bit values and of 32-bit abundances are needed")
        if kmers.device.index != self.device or abundance.device.index != self.device:
            raise ValueError("load_rows_tensor: the tensors must be on the context's device, cuda:%d" % self.device)
        kmers, abundance = kmers.contiguous(), abundance.contiguous()
        n = abundance.numel()
        if kmers.numel() != n * self.words or (kmers.dim() == 2 and kmers.shape[1] != self.words) or kmers.dim() > 2 or (kmers.dim() == 1 and self.words != 1 and n):
            raise ValueError("load_rows_tensor: kmers must be [n, %d] for %d abundances" % (self.words, n))
        torch.cuda.current_stream(kmers.device).synchronize()     # the context's stream is not torch's: the rows are written before the load reads them
        return self.load_rows(kmers.data_ptr() if n else 0, abundance.data_ptr() if n else 0, n, combine)

    def load_rows_numpy(self, kmers, abundance, combine: str = "sum") -> dict:
        """kmers: uint64 [n, words] (or [n] for words == 1), abundance: uint32 [n], host arrays: copied up, then as load_rows."""
        import torch
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1, self.words)
        abundance = np.ascontiguousarray(abundance, dtype=np.uint32).reshape(-1)
        if kmers.shape[0] != abundance.shape[0]:
            raise ValueError("load_rows_numpy: %d k-mers for %d abundances" % (kmers.shape[0], abundance.shape[0]))
        dev = torch.device("cuda", self.device)
        return self.load_rows_tensor(torch.from_numpy(kmers.view(np.int64)).to(dev), torch.from_numpy(abundance.view(np.int32)).to(dev), combine)

    def save_rows(self, path: str) -> None:
        """The rows of the last result -- and the colour matrix when one is kept -- into one .npz: k, kmers, abundance [, colors]."""
        kmers, ab = self.rows()
        data = {"k": np.array(self.kmer_size, dtype=np.int64), "kmers": kmers, "abundance": ab}
        if getattr(self, "_n_colors", 0):
            try:
                counts, _ = self.colors_rows_tensor(1)
                data["colors"] = counts.cpu().numpy().view(np.uint32)
            except DskGpuError:                                  # (no matrix is kept any more: the rows changed since)
                pass
        with open(path, "wb") as f:
            np.savez(f, **data)

    def load_saved(self, path: str, combine: str = "unique") -> dict:
        """What save_rows wrote becomes the result (load_rows_numpy); a saved colour matrix is put back (colors_load) when the load kept every
        saved row in its place -- otherwise the matrix no longer fits the rows, and this raises and says why."""
        import torch
        with np.load(path) as z:
            k = int(z["k"])
            kmers, ab = z["kmers"], z["abundance"]
            colors = z["colors"] if "colors" in z.files else None
        if k != self.kmer_size:
            raise ValueError("load_saved: %s holds rows of k = %d, this context counts k = %d" % (path, k, self.kmer_size))
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1, self.words)
        if colors is not None:
            if colors.shape[0] != kmers.shape[0]:
                raise ValueError("load_saved: %s holds %d lines of colours for %d rows" % (path, colors.shape[0], kmers.shape[0]))
            # the matrix has one line per saved row: rows saved in partition order are put in the global order with their lines here,
            # so that line r still belongs to row r once the load has ordered the rows
            order = np.lexsort(tuple(kmers[:, w] for w in range(self.words)))
            kmers, ab, colors = kmers[order], ab[order], colors[order]
        st = self.load_rows_numpy(kmers, ab, combine)
        if colors is not None:
            if st["n_rows"] != st["n_in"]:
                raise ValueError("load_saved: the colour matrix of %s is not restored: the load kept %d of the %d saved rows (%d distinct, %d below "
                                 "abundance_min, %d above abundance_max), and the matrix has one line per saved row"
                                 % (path, st["n_rows"], st["n_in"], st["n_distinct"], st["n_below"], st["n_above"]))
            self.colors_load_tensor(torch.from_numpy(np.ascontiguousarray(colors).view(np.int32)).to(torch.device("cuda", self.device)))
        return st

    def load_ascii(self, path: str, combine: str = "sum") -> dict:
        """The text `dsk2ascii` writes (`<letters> <abundance>` per line) becomes the result: parse_ascii_rows, then load_rows_numpy."""
        kmers, ab = parse_ascii_rows(path, self.kmer_size)
        return self.load_rows_numpy(kmers, ab, combine)

    def colors_pairs(self, min_count: int, shared_ptr: int, cross_ptr: int, min_sum_ptr: int, select_ptr: int = 0) -> dict:
        """shared_ptr / cross_ptr / min_sum_ptr: n_colors * n_colors u64 on the device each, any may be 0 <- the pair matrices of the kept
        matrix over the rows whose byte at select_ptr is non-zero (0: every row), cells below min_count taken as 0.  -> the stats: n_rows,
        n_selected, n_present (selected rows with a cell left), n_colors."""
        st = _ColorPairStats()
        self._ck(self._lib.dskgpu_colors_pairs(self._h, min_count, *(C.c_void_p(p) if p else None for p in (select_ptr, shared_ptr, cross_ptr, min_sum_ptr)), C.byref(st)))
        return _stats_dict(st)

    def colors_pairs_tensor(self, min_count: int = 1, select=None):
        """select: None, or a CUDA bool / uint8 tensor of n_rows flags.  -> (shared, cross, min_sum: int64[n_colors, n_colors] CUDA tensors,
        the stats)."""
        import torch
        n, nc = self._colors_shape()
        dev = torch.device("cuda", self.device)
        if select is not None:
            if not select.is_cuda or select.dtype not in (torch.bool, torch.uint8) or select.numel() != n:
                raise ValueError("colors_pairs_tensor: select must be a CUDA bool or uint8 tensor of %d flags" % n)
            select = select.contiguous().view(torch.uint8)
        out = torch.zeros((3, nc, nc), dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()              # the context's stream is not torch's: the zero fill is done before the kernel adds
        st = self.colors_pairs(min_count, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), select.data_ptr() if select is not None and n else 0)
        return out[0], out[1], out[2], st

    def colors_marks(self, keep_ptr: int, need_all: int = 0, need_none: int = 0, min_count: int = 1, min_present: int = 0, max_present: int = 0,
                     invert: bool = False) -> dict:
        """keep_ptr: n_rows bytes on the device <- 1 or 0, the form filter_rows takes: with m the mask of the row's colours that hold at least
        min_count, a row is kept when m has every bit of need_all, none of need_none, at least min_present bits and at most max_present
        (0: no upper bound); invert flips the answer.  -> the stats: n_rows, n_kept."""
        rule, st = _ColorRule(need_all=need_all, need_none=need_none, min_count=min_count, min_present=min_present, max_present=max_present,
                              flags=COLORS_INVERT if invert else 0), _ColorMarkStats()
        self._ck(self._lib.dskgpu_colors_marks(self._h, C.byref(rule), C.c_void_p(keep_ptr) if keep_ptr else None, C.byref(st)))
        return _stats_dict(st)

    def colors_marks_tensor(self, **rule):
        """-> (uint8[n_rows] CUDA tensor of the marks, the stats); the rule as colors_marks."""
        import torch
        n, _ = self._colors_shape()
        dev = torch.device("cuda", self.device)
        keep = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        st = self.colors_marks(keep.data_ptr(), **rule)
        return keep[:n], st

    # -- rows out of a result, and the tips of the compacted graph (include/dskgpu.h: dskgpu_filter_rows / _graph_tips / _clip_tips)
    def filter_rows(self, d_keep: int) -> int:
        """d_keep: n_rows bytes on the device (result order), non-zero = keep the row.  The result, its partitions and every lookup and
        graph call describe the kept rows from now on; stats() and histogram() stay the count's.  -> the rows left."""
        n = C.c_uint64(0)
        self._ck(self._lib.dskgpu_filter_rows(self._h, C.c_void_p(d_keep) if d_keep else None, C.byref(n)))
        return int(n.value)

    def filter_rows_tensor(self, keep) -> int:
        """keep: CUDA bool or uint8 tensor of n_rows flags.  -> the rows left."""
        import torch
        if not keep.is_cuda or keep.dtype not in (torch.bool, torch.uint8):
            raise ValueError("filter_rows_tensor: a CUDA bool or uint8 tensor is needed")
        n = self.result_device()[2]
        if keep.numel() != n:
            raise ValueError("filter_rows_tensor: %d flags for %d rows" % (keep.numel(), n))
        keep = keep.contiguous().view(torch.uint8)
        torch.cuda.current_stream(keep.device).synchronize()      # the context's stream is not torch's: the flags are written before the filter reads them
        return self.filter_rows(keep.data_ptr() if n else 0)

    def graph_tips(self, max_nodes: int, max_abundance: int = 0, d_row_tip: int = 0, d_unitig_tip: int = 0) -> dict:
        """One round of the tip rule on the last result, which stays as it is.  d_row_tip: n_rows bytes on the device <- 1 = the row's unitig
        is a tip; d_unitig_tip: n_unitigs bytes <- bit 0 candidate, bit 1 tip, bit 2 outranked; either may be 0.  -> the round's counts:
        n_candidates, n_tips, n_outranked, n_rows_clipped, n_rounds (1), n_rows_left."""
        par, st = _TipParams(max_nodes=max_nodes, max_abundance=max_abundance), _TipStats()
        self._ck(self._lib.dskgpu_graph_tips(self._h, C.byref(par), C.c_void_p(d_row_tip) if d_row_tip else None,
                                             C.c_void_p(d_unitig_tip) if d_unitig_tip else None, C.byref(st)))
        return _stats_dict(st)

    def graph_tips_tensor(self, max_nodes: int, max_abundance: int = 0):
        """-> (uint8[n_rows] row is on a tip, uint8[n_unitigs] candidate | tip << 1 | outranked << 2, the stats of graph_tips), CUDA tensors."""
        import torch
        nu = self.unitigs()["n_unitigs"]
        n = self.result_device()[2]
        dev = torch.device("cuda", self.device)
        row_tip, unitig_tip = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(nu, dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()              # the context's stream is not torch's: the zero fill is done before the kernels write
        st = self.graph_tips(max_nodes, max_abundance, row_tip.data_ptr() if n else 0, unitig_tip.data_ptr() if nu else 0)
        return row_tip, unitig_tip, st

    def clip_tips(self, max_nodes: Optional[int] = None, max_abundance: int = 0, max_rounds: int = 0) -> dict:
        """Rounds of (tips -> filter_rows) until a round finds no tip or max_rounds (0 = 64) rounds have clipped; max_nodes None = kmer_size.
        On return the unitigs and the edges of the rows left are built: write_gfa writes the cleaned graph.  -> the sums over the rounds,
        n_rounds = rounds that clipped, n_rows_left = the rows of the result now."""
        par = _TipParams(max_nodes=self.kmer_size if max_nodes is None else max_nodes, max_abundance=max_abundance, max_rounds=max_rounds)
        st = _TipStats()
        self._ck(self._lib.dskgpu_clip_tips(self._h, C.byref(par), C.byref(st)))
        return _stats_dict(st)

    # -- the simple bubbles of the compacted graph, and tips and bubbles in turn (include/dskgpu.h: dskgpu_graph_bubbles / _pop_bubbles / _simplify)
    def graph_bubbles(self, max_nodes: int, max_diff: int = 4, d_row_pop: int = 0, d_unitig_bits: int = 0) -> dict:
        """One round of the bubble rule on the last result, which stays as it is.  d_row_pop: n_rows bytes on the device <- 1 = the row's
        unitig is popped; d_unitig_bits: n_unitigs bytes <- bit 0 candidate, bit 1 popped, bit 2 in a bubble; either may be 0.  -> the
        round's counts: n_candidates, n_in_bubbles, n_popped, n_rows_popped, n_rounds (1), n_rows_left."""
        par, st = _BubbleParams(max_nodes=max_nodes, max_diff=max_diff), _BubbleStats()
        self._ck(self._lib.dskgpu_graph_bubbles(self._h, C.byref(par), C.c_void_p(d_row_pop) if d_row_pop else None,
                                                C.c_void_p(d_unitig_bits) if d_unitig_bits else None, C.byref(st)))
        return _stats_dict(st)

    def graph_bubbles_tensor(self, max_nodes: int, max_diff: int = 4):
        """-> (uint8[n_rows] row is popped, uint8[n_unitigs] candidate | popped << 1 | in a bubble << 2, the stats of graph_bubbles), CUDA tensors."""
        import torch
        nu = self.unitigs()["n_unitigs"]
        n = self.result_device()[2]
        dev = torch.device("cuda", self.device)
        row_pop, unitig_bits = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(nu, dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()              # the context's stream is not torch's: the zero fill is done before the kernels write
        st = self.graph_bubbles(max_nodes, max_diff, row_pop.data_ptr() if n else 0, unitig_bits.data_ptr() if nu else 0)
        return row_pop, unitig_bits, st

    def pop_bubbles(self, max_nodes: Optional[int] = None, max_diff: int = 4, max_rounds: int = 0) -> dict:
        """Rounds of (bubbles -> filter_rows) until a round pops nothing or max_rounds (0 = 64) rounds have popped; max_nodes None =
        2 * kmer_size.  On return the unitigs and the edges of the rows left are built.  -> the sums over the rounds, n_rounds = rounds that
        popped, n_rows_left = the rows of the result now."""
        par = _BubbleParams(max_nodes=2 * self.kmer_size if max_nodes is None else max_nodes, max_diff=max_diff, max_rounds=max_rounds)
        st = _BubbleStats()
        self._ck(self._lib.dskgpu_pop_bubbles(self._h, C.byref(par), C.byref(st)))
        return _stats_dict(st)

    def simplify(self, tips: Optional[dict] = None, bubbles: Optional[dict] = None, max_passes: int = 0) -> dict:
        """Passes of (clip_tips, then pop_bubbles) until a pass removes no row or max_passes (0 = 16) passes have run.  tips / bubbles: the
        keyword arguments of clip_tips / pop_bubbles (None = their defaults), or False to skip that half.  On return the unitigs and the
        edges of the rows left are built: write_gfa writes the cleaned graph.  -> {n_passes, n_rows_left, tips: the sums of clip_tips'
        dicts, bubbles: those of pop_bubbles'}."""
        tp, bp = self._tip_params_of(tips), self._bubble_params_of(bubbles)
        st = _SimplifyStats()
        self._ck(self._lib.dskgpu_simplify(self._h, C.byref(tp) if tp is not None else None, C.byref(bp) if bp is not None else None, max_passes, C.byref(st)))
        return {"n_passes": int(st.n_passes), "n_rows_left": int(st.n_rows_left), "tips": _stats_dict(st.tips), "bubbles": _stats_dict(st.bubbles)}

    def _rule_params(self, who, part, cls, args, nodes, **defaults):
        """a part of simplify / simplify_all -> its parameter structure: args is a dict of the rule's keyword arguments, None = its defaults,
        False = no such part (-> None).  max_nodes None = nodes * kmer_size; defaults: the rule's other arguments"""
        if args is False:
            return None
        a = dict(args or {})
        mn = a.pop("max_nodes", None)
        par = cls(max_nodes=nodes * self.kmer_size if mn is None else mn, max_rounds=a.pop("max_rounds", 0), **{k: a.pop(k, v) for k, v in defaults.items()})
        if a:
            raise TypeError("%s: unknown %s arguments %s" % (who, part, sorted(a)))
        return par

    def _tip_params_of(self, tips):
        return self._rule_params("simplify", "tip", _TipParams, tips, 1, max_abundance=0)

    def _bubble_params_of(self, bubbles):
        return self._rule_params("simplify", "bubble", _BubbleParams, bubbles, 2, max_diff=4)

    def _connection_params_of(self, connections):
        return self._rule_params("simplify_all", "connection", _ConnectionParams, connections, 2, min_ratio=4, max_abundance=0)

    # -- the erroneous connections of the compacted graph, and all three rules in turn (include/dskgpu.h: dskgpu_graph_connections /
    # _remove_connections / _simplify_all)
    def graph_connections(self, max_nodes: int, min_ratio: int = 4, max_abundance: int = 0, d_row_rem: int = 0, d_unitig_bits: int = 0) -> dict:
        """One round of the erroneous-connection rule on the last result, which stays as it is.  d_row_rem: n_rows bytes on the device <- 1 =
        the row's unitig is removed; d_unitig_bits: n_unitigs bytes <- bit 0 candidate, bit 1 removed, bit 2 weak at the end 2u, bit 3 weak
        at the end 2u + 1; either may be 0.  -> the round's counts: n_candidates, n_one_sided, n_removed, n_rows_removed, n_rounds (1),
        n_rows_left."""
        par, st = _ConnectionParams(max_nodes=max_nodes, min_ratio=min_ratio, max_abundance=max_abundance), _ConnectionStats()
        self._ck(self._lib.dskgpu_graph_connections(self._h, C.byref(par), C.c_void_p(d_row_rem) if d_row_rem else None,
                                                    C.c_void_p(d_unitig_bits) if d_unitig_bits else None, C.byref(st)))
        return _stats_dict(st)

    def graph_connections_tensor(self, max_nodes: int, min_ratio: int = 4, max_abundance: int = 0):
        """-> (uint8[n_rows] row is removed, uint8[n_unitigs] candidate | removed << 1 | weak at 2u << 2 | weak at 2u + 1 << 3, the stats of
        graph_connections), CUDA tensors."""
        import torch
        nu = self.unitigs()["n_unitigs"]
        n = self.result_device()[2]
        dev = torch.device("cuda", self.device)
        row_rem, unitig_bits = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(nu, dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()              # the context's stream is not torch's: the zero fill is done before the kernels write
        st = self.graph_connections(max_nodes, min_ratio, max_abundance, row_rem.data_ptr() if n else 0, unitig_bits.data_ptr() if nu else 0)
        return row_rem, unitig_bits, st

    def remove_connections(self, max_nodes: Optional[int] = None, min_ratio: int = 4, max_abundance: int = 0, max_rounds: int = 0) -> dict:
        """Rounds of (connections -> filter_rows) until a round removes nothing or max_rounds (0 = 64) rounds have removed; max_nodes None =
        2 * kmer_size.  On return the unitigs and the edges of the rows left are built.  -> the sums over the rounds, n_rounds = rounds that
        removed, n_rows_left = the rows of the result now."""
        par = _ConnectionParams(max_nodes=2 * self.kmer_size if max_nodes is None else max_nodes, min_ratio=min_ratio, max_abundance=max_abundance,
                                max_rounds=max_rounds)
        st = _ConnectionStats()
        self._ck(self._lib.dskgpu_remove_connections(self._h, C.byref(par), C.byref(st)))
        return _stats_dict(st)

    def simplify_all(self, tips: Optional[dict] = None, bubbles: Optional[dict] = None, connections: Optional[dict] = None, max_passes: int = 0) -> dict:
        """Passes of (clip_tips, pop_bubbles, then remove_connections) until a pass removes no row or max_passes (0 = 16) passes have run.
        tips / bubbles / connections: the keyword arguments of clip_tips / pop_bubbles / remove_connections (None = their defaults), or
        False to skip that part.  On return the unitigs and the edges of the rows left are built.  -> {n_passes, n_rows_left, tips,
        bubbles, connections: the sums of the three calls' dicts}."""
        tp, bp, cp = self._tip_params_of(tips), self._bubble_params_of(bubbles), self._connection_params_of(connections)
        st = _SimplifyAllStats()
        self._ck(self._lib.dskgpu_simplify_all(self._h, *(C.byref(x) if x is not None else None for x in (tp, bp, cp)), max_passes, C.byref(st)))
        return {"n_passes": int(st.n_passes), "n_rows_left": int(st.n_rows_left), "tips": _stats_dict(st.tips), "bubbles": _stats_dict(st.bubbles),
                "connections": _stats_dict(st.connections)}

    # -- the bubbles of the compacted graph reported as variants (include/dskgpu.h: dskgpu_variants / _variants_table / _variants_stream)
    def variants(self, max_nodes: Optional[int] = None, max_diff: int = 4) -> dict:
        """Find the variants of the last result -- the pairs of sibling unitigs of the bubble rule -- and keep their records and their
        stream in the context; the result stays as it is.  max_nodes None = 2 * kmer_size.  -> the stats: n_variants, n_snps, n_multi,
        n_indels, n_complex, n_unitigs (the unitigs in a variant), stream_bytes, max_letters (the longest text compared)."""
        par, st = _VariantParams(max_nodes=2 * self.kmer_size if max_nodes is None else max_nodes, max_diff=max_diff), _VariantStats()
        self._ck(self._lib.dskgpu_variants(self._h, C.byref(par), C.byref(st)))
        self._variant_stats = {name: int(getattr(st, name)) for name, _ in _VariantStats._fields_}
        return dict(self._variant_stats)

    def variants_table(self, d_records: int) -> None:
        """d_records: 8 * n_variants u32 on the device <- A, B, from, to, lcp, lcs, n_mismatch, kind of every kept variant."""
        self._ck(self._lib.dskgpu_variants_table(self._h, C.c_void_p(d_records) if d_records else None))

    def variants_stream(self, d_offsets: int, d_bytes: int, capacity: int = 0) -> None:
        """d_offsets: 2 * n_variants + 1 u64 on the device <- the first byte of every line of the variant stream (the last: stream_bytes);
        d_bytes: capacity bytes <- text(A) '\\n' text(B) '\\n' of every kept variant; either may be 0."""
        self._ck(self._lib.dskgpu_variants_stream(self._h, C.c_void_p(d_offsets) if d_offsets else None, C.c_void_p(d_bytes) if d_bytes else None, capacity))

    def variants_tensor(self):
        """-> int64[n_variants, 8] (A, B, from, to, lcp, lcs, n_mismatch, kind), a CUDA tensor, of the variants the last variants() of this
        object kept (its stats size the tensor; when the library has dropped them since, the call raises DSKGPU_E_STATE)."""
        import torch
        n = (getattr(self, "_variant_stats", None) or {"n_variants": 0})["n_variants"]
        dev = torch.device("cuda", self.device)
        rec = torch.zeros((max(n, 1), 8), dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()              # the context's stream is not torch's: the zero fill is done before the copy writes
        self.variants_table(rec.data_ptr())
        return rec[:n].to(torch.int64) & 0xFFFFFFFF

    def variants_stream_tensor(self):
        """-> (int64[2 * n_variants + 1] line offsets, uint8[stream_bytes] the variant stream), CUDA tensors, of the kept variants."""
        import torch
        st = getattr(self, "_variant_stats", None) or {"n_variants": 0, "stream_bytes": 0}
        n, nb = st["n_variants"], st["stream_bytes"]
        dev = torch.device("cuda", self.device)
        off, text = torch.zeros(2 * n + 1, dtype=torch.int64, device=dev), torch.zeros(max(nb, 1), dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        self.variants_stream(off.data_ptr(), text.data_ptr(), nb)
        return off, text[:nb]

    def write_variants(self, path: str) -> dict:
        """The kept variants as FASTA, two records per variant:
        >v<i>|a|<KIND>|<u>+ from=<U> to=<U> L=<nodes> S=<abundance sum> lcp=<n> lcs=<n> n_mismatch=<n>
        and the same with |b| and the oriented unitig of the second branch, oriented unitigs in GFA style (17+ / 17-).
        -> dict(n_variants, n_snps, n_multi, n_indels, n_complex)."""
        rec = self.variants_tensor().cpu().numpy()
        off, text = (t.cpu().numpy() for t in self.variants_stream_tensor())
        offsets, ab_sum, _ = (t.cpu().numpy() for t in self.unitigs_table_tensor())
        nodes = np.diff(offsets.astype(np.int64)) - self.kmer_size
        raw = text.tobytes()

        def gfa(U):
            return "%d%s" % (int(U) >> 1, "-" if int(U) & 1 else "+")

        with open(path, "w") as f:
            for i, (A, B, frm, to, lcp, lcs, nm, kind) in enumerate(rec.tolist()):
                for j, (side, U) in enumerate((("a", A), ("b", B))):
                    f.write(">v%d|%s|%s|%s from=%s to=%s L=%d S=%d lcp=%d lcs=%d n_mismatch=%d\n" % (
                        i, side, VARIANT_KINDS[kind], gfa(U), gfa(frm), gfa(to), int(nodes[U >> 1]), int(ab_sum[U >> 1]), lcp, lcs, nm))
                    f.write(raw[int(off[2 * i + j]): int(off[2 * i + j + 1]) - 1].decode() + "\n")
        st = self._variant_stats
        return {name: st[name] for name in ("n_variants", "n_snps", "n_multi", "n_indels", "n_complex")}

    # -- the connected components of the compacted graph (include/dskgpu.h: dskgpu_components* / _graph_small_components / _drop_components)
    def components(self) -> dict:
        """Build the components of the last result's compacted graph (the edges, the compaction and the index too when they are not there)
        -> the stats: n_components, n_single, max_unitigs, max_rows, n_rounds (launches of the labelling)."""
        st = _ComponentStats()
        self._ck(self._lib.dskgpu_components(self._h, C.byref(st)))
        return _stats_dict(st)

    def components_labels(self, d_unitig_comp: int, d_row_comp: int) -> None:
        """d_unitig_comp: n_unitigs u32 on the device <- the component of every unitig; d_row_comp: n_rows u32 <- that of every row's unitig;
        either may be 0."""
        self._ck(self._lib.dskgpu_components_labels(self._h, C.c_void_p(d_unitig_comp) if d_unitig_comp else None, C.c_void_p(d_row_comp) if d_row_comp else None))

    def components_labels_tensor(self):
        """-> (int32[n_unitigs] component of every unitig, int32[n_rows] component of every row), CUDA tensors."""
        import torch
        nu = self.unitigs()["n_unitigs"]
        n = self.result_device()[2]
        dev = torch.device("cuda", self.device)
        ucomp, rcomp = torch.zeros(max(nu, 1), dtype=torch.int32, device=dev), torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()              # the context's stream is not torch's: the zero fill is done before the kernels write
        self.components_labels(ucomp.data_ptr(), rcomp.data_ptr())
        return ucomp[:nu], rcomp[:n]

    def components_table(self, d_first: int, d_unitigs: int, d_rows: int, d_ab_sum: int, d_edges: int) -> None:
        """d_first: n_components u32 (the smallest unitig of every component), d_unitigs / d_rows / d_ab_sum / d_edges: n_components u64 each,
        on the device; any may be 0."""
        self._ck(self._lib.dskgpu_components_table(self._h, *(C.c_void_p(p) if p else None for p in (d_first, d_unitigs, d_rows, d_ab_sum, d_edges))))

    def components_table_tensor(self):
        """-> (int32[n_c] first, int64[n_c] unitigs, int64[n_c] rows, int64[n_c] ab_sum, int64[n_c] edges), CUDA tensors."""
        import torch
        nc = self.components()["n_components"]
        dev = torch.device("cuda", self.device)
        first = torch.zeros(max(nc, 1), dtype=torch.int32, device=dev)
        cols = [torch.zeros(max(nc, 1), dtype=torch.int64, device=dev) for _ in range(4)]
        torch.cuda.current_stream(dev).synchronize()
        self.components_table(first.data_ptr(), *(c.data_ptr() for c in cols))
        return (first[:nc],) + tuple(c[:nc] for c in cols)

    def small_components(self, min_rows: int, max_abundance: int = 0, d_row_drop: int = 0, d_comp_small: int = 0) -> dict:
        """The small-component rule on the last result, which stays as it is: a component is small when it has fewer than min_rows rows and
        (max_abundance == 0 or its mean abundance is at most max_abundance).  d_row_drop: n_rows bytes on the device <- 1 = the row's
        component is small; d_comp_small: n_components bytes <- 1 = small; either may be 0.  -> n_small, n_unitigs_dropped, n_rows_dropped,
        n_rows_left."""
        par, st = _ComponentParams(min_rows=min_rows, max_abundance=max_abundance), _ComponentDropStats()
        self._ck(self._lib.dskgpu_graph_small_components(self._h, C.byref(par), C.c_void_p(d_row_drop) if d_row_drop else None,
                                                         C.c_void_p(d_comp_small) if d_comp_small else None, C.byref(st)))
        return _stats_dict(st)

    def small_components_tensor(self, min_rows: int, max_abundance: int = 0):
        """-> (uint8[n_rows] the row's component is small, uint8[n_components] small, the stats of small_components), CUDA tensors."""
        import torch
        nc = self.components()["n_components"]
        n = self.result_device()[2]
        dev = torch.device("cuda", self.device)
        row_drop, comp_small = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(nc, dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()              # the context's stream is not torch's: the zero fill is done before the kernels write
        st = self.small_components(min_rows, max_abundance, row_drop.data_ptr() if n else 0, comp_small.data_ptr() if nc else 0)
        return row_drop, comp_small, st

    def drop_components(self, min_rows: int, max_abundance: int = 0) -> dict:
        """Take the rows of the small components out of the result (one filter_rows; one application is final).  On return the unitigs, the
        edges and the components of the rows left are built.  -> n_small, n_unitigs_dropped, n_rows_dropped, n_rows_left."""
        par, st = _ComponentParams(min_rows=min_rows, max_abundance=max_abundance), _ComponentDropStats()
        self._ck(self._lib.dskgpu_drop_components(self._h, C.byref(par), C.byref(st)))
        return _stats_dict(st)

    # -- kernel-level entry points (parity tests)
    def k_encode(self, d_bytes: int, nbytes: int, d_packed: int, d_invalid: int) -> None:
        self._ck(self._lib.dskgpu_k_encode(self._h, C.c_void_p(d_bytes), nbytes, C.c_void_p(d_packed), C.c_void_p(d_invalid)))

    def k_enumerate(self, d_bytes: int, nbytes: int, d_kmers: int, d_valid: int) -> None:
        self._ck(self._lib.dskgpu_k_enumerate(self._h, C.c_void_p(d_bytes), nbytes, C.c_void_p(d_kmers), C.c_void_p(d_valid)))

    def k_minimizers(self, d_bytes: int, nbytes: int, d_minim: int, d_valid: int) -> None:
        self._ck(self._lib.dskgpu_k_minimizers(self._h, C.c_void_p(d_bytes), nbytes, C.c_void_p(d_minim), C.c_void_p(d_valid)))


class KmerGroup:
    """N ranks of one sharded count inside this process (include/dskgpu.h: dskgpu_group_*): what `dsk -nb-gpus N` runs.
    `rank(r)` is a KmerCounter view of rank r for feeding reads and reading that rank's rows."""

    def __init__(self, devices, kmer_size: int = 31, abundance_min: int = 2, abundance_max: int = 2147483647,
                 histo_max: int = 10000, nb_partitions: int = 0, timing: bool = False, sort: bool = True,
                 minimizer_size: int = 0, max_pass_mkeys: int = 0, mg_explicit: bool = False):
        self._lib = load_library()
        devices = list(devices)
        cfg = _make_config(kmer_size, abundance_min, abundance_max, histo_max, 0, nb_partitions, timing, sort, len(devices), 0,
                           minimizer_size, max_pass_mkeys, "sum", 0, False, mg_explicit)
        devs = (C.c_int32 * len(devices))(*devices)
        h = C.c_void_p()
        rc = self._lib.dskgpu_group_create(C.byref(cfg), devs, len(devices), C.byref(h))
        if rc != 0:
            raise DskGpuError(rc, self._lib.dskgpu_group_last_error(None).decode())
        self._h = h
        self.size = len(devices)
        self.kmer_size, self.histo_max = kmer_size, histo_max
        self.words = (kmer_size + 31) // 32
        self._ranks = [KmerCounter._borrowed(self._lib.dskgpu_group_ctx(self._h, r), kmer_size, histo_max, self.size, devices[r])
                       for r in range(self.size)]

    def _ck(self, rc: int) -> None:
        if rc != 0:
            raise DskGpuError(rc, self._lib.dskgpu_group_last_error(self._h).decode())

    def close(self) -> None:
        if getattr(self, "_h", None):
            for r in self._ranks:
                r._h = None
            self._lib.dskgpu_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def rank(self, r: int) -> KmerCounter:
        return self._ranks[r]

    def transport(self) -> str:
        return self._lib.dskgpu_group_transport(self._h).decode()

    def count(self) -> None:
        self._ck(self._lib.dskgpu_group_count(self._h))

    def exchanged_words(self) -> int:
        return int(self._lib.dskgpu_group_exchanged_words(self._h))

    def sliced_steps(self) -> int:
        """Steps of the last count whose exchange ran in slices (overlapped with the sender and the receiver's level 1)."""
        return int(self._lib.dskgpu_group_sliced_steps(self._h))

    def histogram(self) -> np.ndarray:
        out = np.zeros(self.histo_max + 1, dtype=np.uint64)
        self._ck(self._lib.dskgpu_group_histogram(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), self.histo_max + 1))
        return out

    def stats(self) -> dict:
        s = _Stats()
        self._ck(self._lib.dskgpu_group_get_stats(self._h, C.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in _Stats._fields_ if k != "reserved"}

    def num_partitions(self) -> int:
        return int(self._lib.dskgpu_group_num_partitions(self._h))

    def partition(self, p: int) -> Tuple[np.ndarray, np.ndarray]:
        n = int(self._lib.dskgpu_group_partition_size(self._h, p))
        kmers = np.zeros((n, self.words), dtype=np.uint64)
        ab = np.zeros(n, dtype=np.uint32)
        self._ck(self._lib.dskgpu_group_partition_copy(self._h, p, C.c_void_p(kmers.ctypes.data), C.c_void_p(ab.ctypes.data)))
        return kmers, ab


def sample_distances(shared, cross, min_sum) -> dict:
    """The pair matrices of colors_pairs (numpy arrays or tensors, [n_colors, n_colors]) -> {name: float64[n_colors, n_colors]}, the
    distances between the samples.  With N = diag(shared), T = diag(cross), a = shared, s = min_sum, U[i][j] = cross[i][j] / T[i] and
    V[i][j] = cross[j][i] / T[j]:
      jaccard 1 - a / (Ni + Nj - a); sorensen 1 - 2a / (Ni + Nj); ochiai 1 - a / sqrt(Ni Nj); kulczynski 1 - (a / Ni + a / Nj) / 2;
      bray_curtis 1 - 2s / (Ti + Tj); ruzicka 1 - s / (Ti + Tj - s);
      ab_jaccard 1 - UV / (U + V - UV); ab_ochiai 1 - sqrt(UV); ab_sorensen 1 - 2UV / (U + V).
    An entry whose denominator is zero (an empty sample) is NaN."""
    def f64(m):
        m = m.cpu().numpy() if hasattr(m, "cpu") else np.asarray(m)
        if m.dtype == np.int64:
            m = m.view(np.uint64)                                 # (a tensor holds the bit pattern of a u64)
        return m.astype(np.float64)

    a, x, s = f64(shared), f64(cross), f64(min_sum)
    if a.ndim != 2 or a.shape[0] != a.shape[1] or x.shape != a.shape or s.shape != a.shape:
        raise ValueError("sample_distances: three square matrices of one shape are needed")
    N, T = np.diag(a), np.diag(x)
    Ni, Nj, Ti, Tj = N[:, None], N[None, :], T[:, None], T[None, :]

    def over(num, den):
        out = np.full(a.shape, np.nan)
        np.divide(num, den, out=out, where=den != 0)
        return out

    U, V = over(x, Ti), over(x.T, Tj)
    UV = U * V
    return {
        "jaccard": 1.0 - over(a, Ni + Nj - a),
        "sorensen": 1.0 - over(2.0 * a, Ni + Nj),
        "ochiai": 1.0 - over(a, np.sqrt(Ni * Nj)),
        "kulczynski": 1.0 - (over(a, Ni) + over(a, Nj)) / 2.0,
        "bray_curtis": 1.0 - over(2.0 * s, Ti + Tj),
        "ruzicka": 1.0 - over(s, Ti + Tj - s),
        "ab_jaccard": 1.0 - over(UV, U + V - UV),
        "ab_ochiai": 1.0 - np.sqrt(UV),
        "ab_sorensen": 1.0 - over(2.0 * UV, U + V),
    }


def kmer_to_string(value: int, k: int) -> str:
    """Kmer<span>::ModelCanonical::toString (utils/dsk2ascii.cpp:104): MSB-first, A C T G = 0 1 2 3."""
    return "".join("ACTG"[(value >> (2 * (k - 1 - i))) & 3] for i in range(k))


def parse_ascii_rows(path_or_lines, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """`dsk2ascii`'s default text -- `<letters> <abundance>` per line, the inverse of kmer_to_string -- as (kmers uint64[n, words] LSW first,
    abundance uint32[n]).  path_or_lines: a file name or an iterable of lines.  A line of the wrong length, with other letters or with an
    abundance that is no positive 32-bit number raises ValueError naming the line (1-based)."""
    words = (k + 31) // 32
    code = {"A": 0, "C": 1, "T": 2, "G": 3}
    if isinstance(path_or_lines, (str, bytes, os.PathLike)):
        with open(path_or_lines, "r") as f:
            lines = f.read().splitlines()
    else:
        lines = [ln.decode() if isinstance(ln, bytes) else ln for ln in path_or_lines]
    kmers, ab = [], []
    for no, line in enumerate(lines, 1):
        line = line.rstrip("\r\n")
        if not line.strip():
            continue
        parts = line.split()
        if len(parts) != 2:
            raise ValueError("line %d: expected `<letters> <abundance>`, got %r" % (no, line))
        letters, count = parts
        if len(letters) != k:
            raise ValueError("line %d: %d letters, k is %d" % (no, len(letters), k))
        value = 0
        for ch in letters:
            if ch not in code:
                raise ValueError("line %d: letter %r is none of A, C, G, T" % (no, ch))
            value = (value << 2) | code[ch]
        if not count.isdigit() or not 1 <= int(count) <= 0xFFFFFFFF:
            raise ValueError("line %d: abundance %r is no number in 1 .. 2^32 - 1" % (no, count))
        kmers.append([(value >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(words)])
        ab.append(int(count))
    return np.array(kmers, dtype=np.uint64).reshape(-1, words), np.array(ab, dtype=np.uint32)
