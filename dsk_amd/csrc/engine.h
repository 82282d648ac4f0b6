// engine.h -- what the host translation units of libdskgpu share: the context (dskgpu_ctx) with its buffers and switches,
// the error macros, and the functions one of them calls in the other.  dskgpu.hip runs the count path and the rest of the C-ABI;
// reads.hip takes the reads in -- pushed bytes, raw file text, a read set on the device (dskgpu_push_reads .. _set_reads_device) -- and owns dskgpu_ctx::reads;
// banks.hip counts the banks of the reads one by one and merges them (dskgpu_next_bank, _set_banks, _histogram2d, the dskgpu_i_* steps of group.hip) and owns dskgpu_ctx::banks;
// sender.hip turns the 2-bit read stream into super-k-mer records -- for the multi-GPU exchange (dskgpu_mg_sample .. _mg_slices_finish) and for
// the record-based level 0 of a multi-pass count (rec_l0_*) -- and owns the two Sender states (dskgpu_ctx::sender, ::l0_sender);
// rowsort.hip orders the solid rows (order_rows) and owns the row sort's state (dskgpu_ctx::rs); query.hip answers lookups in the
// last result (dskgpu_query_*) and owns dskgpu_ctx::query; graph.hip answers the de Bruijn neighbourhood of k-mers from the same index
// (dskgpu_graph_*); unitigs.hip compacts the rows' graph into unitigs and links them (dskgpu_unitigs*, dskgpu_unitig_edges*) and owns dskgpu_ctx::unitigs;
// rowfilter.hip takes rows out of a result (dskgpu_filter_rows), drives the rounds of (a rule -> the filter of the rows it flags) and owns dskgpu_ctx::filtered;
// rules.hip finds and clips the tips, finds and pops the simple bubbles and finds and removes the erroneous connections of the compacted graph with those rounds
// (dskgpu_graph_tips, dskgpu_clip_tips, dskgpu_graph_bubbles, dskgpu_pop_bubbles, dskgpu_graph_connections, dskgpu_remove_connections) and runs the rules in turn (dskgpu_simplify, dskgpu_simplify_all);
// thread.hip threads reads through the compacted graph (dskgpu_thread_*) and owns dskgpu_ctx::threading;
// components.hip labels the connected components of the compacted graph and takes the small ones out (dskgpu_components*, dskgpu_graph_small_components,
// dskgpu_drop_components) and owns dskgpu_ctx::unitigs.cc;
// correct.hip corrects substitution errors in a read stream against the rows (dskgpu_correct_reads) and keeps nothing;
// variants.hip reports the bubbles as pairs of sequences (dskgpu_variants*) and owns dskgpu_ctx::variants;
// readsum.hip summarises the abundances of every read of a stream, marks the reads by a rule and takes reads out of a stream
// (dskgpu_read_summaries*, dskgpu_read_marks, dskgpu_select_reads) and owns dskgpu_ctx::readsum;
// colors.hip counts per row how often every sample (colour) of a read stream with bank boundaries holds it and reduces that matrix onto the
// unitigs (dskgpu_colors_*) and owns dskgpu_ctx::colors.  Private to the library.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dskgpu.h"
#include "layouts.h"

hipError_t placed_malloc(void** out, size_t bytes);      // (dskgpu.hip: DSKGPU_PLACE)
#define HIDDEN __attribute__((visibility("hidden")))      // keeps a name out of the library's dynamic symbols (nm -D): functions one unit calls in another, and the out-of-line copies the compiler emits of in-class release() members

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        // growing a buffer that exists: 6 % on top, so that a size that wobbles by a few per cent from pass to pass (slices from
        // sampled loads) does not free and allocate tens of GB again -- near a full HBM that took a second
        size_t want = ((p ? bytes + bytes / 16 : bytes) + 255) & ~size_t(255);
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        hipError_t e = placed_malloc(&p, want);
        if (e == hipSuccess) cap = want; else p = nullptr;
        return e;
    }
    // grow, keeping the first `keep` bytes (device-to-device copy on `stream`); returns 0 on success
    int ensure_keep(size_t bytes, size_t keep, hipStream_t stream) {
        if (bytes <= cap) return 0;
        void* np = nullptr;
        size_t want = ((std::max(bytes, cap + cap / 2) + 255) & ~size_t(255));
        if (hipMalloc(&np, want) != hipSuccess) return -1;
        if (keep && p) {
            if (hipMemcpyAsync(np, p, keep, hipMemcpyDeviceToDevice, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) { (void)hipFree(np); return -1; }
        }
        if (p) (void)hipFree(p);
        p = np; cap = want;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

enum Scalar { SC_NCH1 = 0, SC_MLEN1, SC_NCH2, SC_MLEN2, SC_OVERFLOW, SC_F, SC_SORTFLAG, SC_OVF2, SC_OVF1, SC_RSLEN, SC_RSWORK, SC_RSWORK2, SC_RSTIES, SC_EXT, SC_NCHAINED, SC_NCH_S, SC_MLEN_S, SC_WORK2, SC_COUNT = 24 };

struct Stage { const char* name; hipEvent_t ev; };

// Test / experiment switches (NOTEBOOK.md "Environment switches"): read ONCE from the environment when a context is
// created; none of them changes results.  The launch paths only look at this struct.
struct Tuning {
    bool no_opt1 = false, no_opt2 = false;      // DSKGPU_NO_OPT1 / _NO_OPT2: exact histogram + scan path at level 1 / at both levels
    bool no_aligned = false;                    // DSKGPU_NO_ALIGNED: plain write-out for key-array scatters
    u32 rs_heavy = 0;                           // DSKGPU_RS_HEAVY: rows of a first-digit bucket above which the row sort gives up (tests)
    u32 rs_bbits = 0;                           // DSKGPU_RS_BBITS: forced width of the row sort's second digit (8..10; tests)
    u32 rs_block_rows = 0;                      // DSKGPU_RS_BLOCK_ROWS: largest sub-bucket the hand-written row sort orders itself (tests: provoke its fallback)
    bool sk_exact = false, no_recsrc = false;   // DSKGPU_SK_EXACT, DSKGPU_NO_RECSRC (multi-GPU sender layout / receiver source)
    u32 opt_cap = 0;                            // DSKGPU_OPT_CAP: forced level-2 region size (keys)
    u64 opt_slice = 0;                          // DSKGPU_OPT_SLICE: forced level-1 slice size (keys)
    u64 sk_slice = 0, sk_minslice = 2000;       // DSKGPU_SK_SLICE, DSKGPU_SK_MINSLICE
    u32 table_maxload = 0;                      // DSKGPU_TABLE_MAXLOAD: distinct keys a count table may hold (forces the finer-partition retry)
    long long max_ext = -1;                     // DSKGPU_MAX_EXT: size of the extension-region pool of the level-2 scatter (tests: 0 = no chains)
    bool no_sample = false;                     // DSKGPU_NO_SAMPLE: level-1 slices from the mean load instead of the sampled per-bin loads
    bool no_heavy = false;                      // DSKGPU_NO_HEAVY: no k-mer is counted apart by the level-1 scatter
    bool verbose = false;                       // DSKGPU_VERBOSE: trace of the plan decisions on stderr
    bool no_level0 = false; u32 l0_passes = 0;  // DSKGPU_NO_LEVEL0: every pass of a multi-pass count re-generates its keys; DSKGPU_L0_PASSES=n: passes per level-0 sweep (tests)
    u64 rs_max_rows = 0;                        // DSKGPU_RS_MAX_ROWS: most rows the MSD row sort takes in one piece (tests: the group-wise path of huge row sets on a small input)
    u32 ps_maxc = 0;                            // DSKGPU_PS_MAXC: rows sharing a value bin that the partition-order sort still orders (tests: 1 provokes its fallback to the global order)
    bool sk_generic = false;                    // DSKGPU_SK_GENERIC: the sender kernels with k and m at run time even for k = 31 / 63 (tests: both forms write the same records)
    bool l0_keys = false;                       // DSKGPU_L0_KEYS: level 0 as key arrays (k_level0) even where the record-based one applies (experiments, tests)
    u32 mp_pass_mkeys = 0;                      // DSKGPU_MP_PASS_MKEYS: keys (millions) per pass of an input that needs several passes (default 1000)
    u64 rs_slab_rows = 0;                       // DSKGPU_RS_SLAB_ROWS: rows per slab of the row sort for >= 2^32 rows (tests: forces that path, with small slabs, on a small input)
    bool unitig_stages = false;                 // DSKGPU_UNITIG_STAGES: the build of the unitigs marks "unitig links" / "unitig ranking" / "unitig numbering" instead of "unitigs" (tools/bench_unitigs.py)
    bool cc_plain = false, cc_stages = false;   // DSKGPU_CC_PLAIN: the component table by one add per unitig and column instead of the wave-combined form; DSKGPU_CC_STAGES: the build of the components marks "component labelling" / "component numbering" / "component table" instead of "components" (tools/bench_components.py)
    bool correct_staged = false;                // DSKGPU_CORRECT_STAGED: the trials of dskgpu_correct_reads by the staged pair (one window of every alternative as a batch, then a wave per surviving candidate) instead of one thread per candidate, which is the default because it measured faster (profiles/read_correction.md; tests, tools/bench_correct.py)
    u32 pairs_reg_max = ~0u, pairs_grid = 0; bool pairs_no_skip = false;    // DSKGPU_PAIRS_GRID: blocks of a pair kernel at the most (unset: CP_GRID; tests: 2 makes every block walk several stretches of a small matrix); DSKGPU_PAIRS_REG_MAX: n_colors (0..8) up to which dskgpu_colors_pairs runs the one-thread-per-row kernel instead of the tiled one (unset: CP_REG_SWITCH of colors.h); DSKGPU_PAIRS_NO_SKIP: the tiled kernel does not step over all-zero rows (tests, tools/bench_color_pairs.py, profiles/color_pairs.md)
    u32 num_cu = 0;                             // DSKGPU_NUM_CU: the CU count every grid and plan is sized from (1..1024; unset, 0 or out of range: the device's own; tests: 1 and 3 make every block of a small input take several units of work, 32 and 304 are a CPX partition and a device whose count is no power of two)
    void read() {
        auto on =[](const char* n) { return getenv(n) != nullptr; };
        auto num = [](const char* n, u64 dflt) { const char* e = getenv(n); return e ? (u64)atoll(e) : dflt; };
        no_opt1 = on("DSKGPU_NO_OPT1"); no_opt2 = on("DSKGPU_NO_OPT2"); no_aligned = on("DSKGPU_NO_ALIGNED");
        sk_exact = on("DSKGPU_SK_EXACT");
        no_recsrc = on("DSKGPU_NO_RECSRC");
        opt_cap = (u32)num("DSKGPU_OPT_CAP", 0) & ~7u; opt_slice = num("DSKGPU_OPT_SLICE", 0) & ~7ull;
        sk_slice = num("DSKGPU_SK_SLICE", 0); sk_minslice = num("DSKGPU_SK_MINSLICE", 2000);
        table_maxload = (u32)num("DSKGPU_TABLE_MAXLOAD", 0);
        max_ext = getenv("DSKGPU_MAX_EXT") ? atoll(getenv("DSKGPU_MAX_EXT")) : -1;
        no_sample = on("DSKGPU_NO_SAMPLE"); no_heavy = on("DSKGPU_NO_HEAVY"); verbose = on("DSKGPU_VERBOSE"); no_level0 = on("DSKGPU_NO_LEVEL0"); l0_passes = (u32)num("DSKGPU_L0_PASSES", 0); mp_pass_mkeys = (u32)num("DSKGPU_MP_PASS_MKEYS", 0); rs_max_rows = num("DSKGPU_RS_MAX_ROWS", 0); l0_keys = on("DSKGPU_L0_KEYS"); sk_generic = on("DSKGPU_SK_GENERIC"); ps_maxc = (u32)num("DSKGPU_PS_MAXC", 0);
        rs_slab_rows = num("DSKGPU_RS_SLAB_ROWS", 0);
        unitig_stages = on("DSKGPU_UNITIG_STAGES");
        cc_plain = on("DSKGPU_CC_PLAIN"); cc_stages = on("DSKGPU_CC_STAGES");
        correct_staged = on("DSKGPU_CORRECT_STAGED");
        pairs_reg_max = (u32)num("DSKGPU_PAIRS_REG_MAX", pairs_reg_max); pairs_no_skip = on("DSKGPU_PAIRS_NO_SKIP"); pairs_grid = (u32)num("DSKGPU_PAIRS_GRID", 0);
        { const u64 n = num("DSKGPU_NUM_CU", 0); num_cu = n >= 1 && n <= 1024 ? (u32)n : 0u; }
        rs_block_rows = (u32)num("DSKGPU_RS_BLOCK_ROWS", 0); rs_bbits = (u32)num("DSKGPU_RS_BBITS", 0); rs_heavy = (u32)num("DSKGPU_RS_HEAVY", 0);
    }
};

// The solid rows of a pass where the count kernels left them (regions of `cap` rows, or exact ranges from fstart; soff = the scan of the
// per-sub-partition solid counts; keys still mixed) + the rows of the k-mers counted apart as a dense, un-mixed tail (W <= 2 only).  The
// row sort's first step and the partition-order pass read them there instead of a dense copy made by k_compact.  as<>(): the descriptor
// a kernel of that width takes (layouts.h), built at its launch.
struct SparseRows {
    int W = 0;                     // 0 = none; else 1, 2 or 4: the words of a key
    const void* keys = nullptr; const u32 *ab = nullptr, *soff = nullptr, *fstart = nullptr; u32 cap = 0, F = 0;
    u64 n_sparse = 0; u32 n_tail = 0; RowsIn tail_w{}; const u32* tail_ab = nullptr;
    template <class S> S as(u32 qpc = 0) const { return S{static_cast<decltype(S::keys)>(keys), ab, soff, fstart, cap, F, qpc}; }
    Rows2C tail2() const { return Rows2C{tail_w.w[1], tail_w.w[0], tail_ab}; }
};

// DSKGPU_F_PARTITION_ORDER for the passes of a multi-pass count: every pass orders its rows partition by partition straight into the job's
// row arrays (one k_part_sort launch instead of k_compact), the offsets of its partitions -- relative to the pass's first row, row_base of
// the job (run_pipeline sets `row_base` before the pass runs) -- go to part_off[off_index ..], one flag serves the whole job; at the end
// the offsets become 64-bit row numbers (RowSort::h_part_off64).  ok: every pass so far took part
struct PartPasses {
    struct Pass { u64 row_base; u32 nparts, off_index; };
    std::vector<Pass> passes; DevBuf part_off, flag; u32 off_used = 0; bool ok = false; u64 row_base = 0;
    std::vector<u32> h_off;
};

// The row sort's state between calls (order_rows below owns it; the partition accessors read its layout)
struct RowSort {
    DevBuf fix_list;               // multi-word row sort: [count | (first row, rows) x FIX_LIST_CAP] of the prefix runs above FIX_CAP rows
    DevBuf g[4];                   // the gathered rows of the listed sub-buckets, one buffer per round (sort_oversize)
    DevBuf del, lens;              // >= 2^32 rows: per (slab, bin) 64-bit output offsets; the slabs' matrix lengths
    std::vector<u64> h_del; std::vector<u32> h_lens, h_lin;
    DevBuf ovs;                    // [count | (offset, rows, bits left) x RS_OVS_CAP] of the sub-buckets listed for another round
    u32 flag = 0, listed = 0;      // host copies of SC_SORTFLAG ("could not finish in place") and of the listed count ovs[0]
    u64* hist_pin = nullptr; size_t hist_pin_n = 0;      // pinned landing of the end-of-step read-back: histogram + k_sort_back's two words
    // DSKGPU_F_PARTITION_ORDER (partsort.h): the rows ascending inside each output partition only.  part_mode: the last result is laid
    // out that way, h_part_off[p] = first row of partition p (n_parts + 1 entries, pinned; several passes: h_part_off64)
    bool part_mode = false; u32 n_parts = 0; u32* h_part_off = nullptr; size_t h_part_cap = 0; DevBuf part_off;
    std::vector<u64> h_part_off64;
    PartPasses mp;
    void release() {
        for (DevBuf* b : {&fix_list, &g[0], &g[1], &g[2], &g[3], &del, &lens, &ovs, &part_off, &mp.part_off, &mp.flag}) b->release();
        if (hist_pin) (void)hipHostFree(hist_pin);
        if (h_part_off) (void)hipHostFree(h_part_off);
        hist_pin = nullptr; h_part_off = nullptr;
    }
};

// Lookups in the last result (query.hip): one open-addressing hash table over the result rows, built on the first query after a count.
// A slot is (fingerprint << 32 | row number), all ones = empty; cap is a power of two >= 2 * rows.  packed / inval: the 2-bit form of the
// QUERIED stream (dskgpu_query_reads) -- buffers of the query's own, so that the context's reads and their kept encoding stay untouched.
// deg: the 25 x u64 degree counters of dskgpu_graph_adjacency (graph.hip), which probes the same table.
struct Query {
    DevBuf table, packed, inval, deg;
    u64 cap = 0;
    bool valid = false;            // the table indexes the current result (dskgpu_ctx::drop_result clears it)
    void release() { table.release(); packed.release(); inval.release(); deg.release(); cap = 0; valid = false; }
    void invalidate() { valid = false; }      // the rows changed under it (dskgpu_filter_rows): built again on the next use, in the memory it has
};

// The rows' de Bruijn graph compacted into unitigs (unitigs.hip), built on the first dskgpu_unitigs* call after a count: per row the unitig
// number and (position << 1 | orientation), per unitig the stream offset (n_unitigs + 1 of them), the abundance sum and the kind.
// The edges between the unitigs, built on the first dskgpu_unitig_edges* call on top of the compaction: per oriented unitig U = 2 u + t its
// last node (ends) and the CSR offset of its targets (e_offsets, 2 n_unitigs + 1 of them), per edge the oriented unitig it leads to.
// The connected components of that graph (components.hip), built on the first dskgpu_components* call on top of the edges and kept with them:
// per unitig its component, per component its smallest unitig (first) and the four columns of the table, cols[col * n_components + c] with
// col = unitigs, rows, ab_sum, edges.  4 bytes per unitig + 36 per component.
struct Components {
    DevBuf comp, first, cols;
    dskgpu_component_stats stats{};
    bool valid = false;            // they are those of the edges of the current result
    void release() { for (DevBuf* b : {&comp, &first, &cols}) b->release(); stats = dskgpu_component_stats{}; valid = false; }
    void invalidate() { stats = dskgpu_component_stats{}; valid = false; }
};

struct Unitigs {
    DevBuf unitig, pos, offsets, ab_sum, kind;
    DevBuf ends, e_offsets, e_targets;
    Components cc;                 // (they go wherever the edges go)
    dskgpu_unitig_stats stats{};
    dskgpu_unitig_edge_stats e_stats{};
    bool valid = false;            // they compact the current result (dskgpu_ctx::drop_result clears it)
    bool e_valid = false;          // ... and the edges are those of that compaction
    void release_edges() { for (DevBuf* b : {&ends, &e_offsets, &e_targets}) b->release(); e_stats = dskgpu_unitig_edge_stats{}; e_valid = false; cc.release(); }
    void release() { for (DevBuf* b : {&unitig, &pos, &offsets, &ab_sum, &kind}) b->release(); stats = dskgpu_unitig_stats{}; valid = false; release_edges(); }
    void invalidate() { stats = dskgpu_unitig_stats{}; e_stats = dskgpu_unitig_edge_stats{}; valid = false; e_valid = false; cc.invalidate(); }      // as Query::invalidate
};

// Reads threaded through the compacted graph (thread.hip), kept by dskgpu_thread_reads until the rows change: the walks as CSR offsets into
// steps (n_walks + 1 of them), the first and last stream position and (j(first), j(last)) of every walk, the oriented unitig of every step,
// and the read support of every unitig and every edge of the compaction the stream was threaded through (n_unitigs, n_edges: theirs).
struct Threading {
    DevBuf offsets, steps, first, last, ends, usup, esup;
    dskgpu_thread_stats stats{};
    u64 n_unitigs = 0, n_edges = 0;
    bool valid = false;            // a threading of the current result is kept (dskgpu_ctx::drop_result and dskgpu_filter_rows drop it)
    void release() { for (DevBuf* b : {&offsets, &steps, &first, &last, &ends, &usup, &esup}) b->release(); stats = dskgpu_thread_stats{}; n_unitigs = n_edges = 0; valid = false; }
};

// The bubbles of the compacted graph reported as variants (variants.hip), kept by dskgpu_variants until the rows change: the records (8 x u32
// per variant), the offsets of the 2 n_variants lines of the variant stream (+ 1) and the stream itself.  32 + 16 bytes per variant + the stream.
struct Variants {
    DevBuf rec, off, stream;
    dskgpu_variant_stats stats{};
    bool valid = false;            // the variants of the current result are kept (dskgpu_ctx::drop_result and dskgpu_filter_rows drop them)
    void release() { for (DevBuf* b : {&rec, &off, &stream}) b->release(); stats = dskgpu_variant_stats{}; valid = false; }
};

// The per-read summaries of a stream (readsum.hip), kept by dskgpu_read_summaries until the rows change: 32 bytes per record.
struct ReadSummaries {
    DevBuf table;
    dskgpu_read_summary_stats stats{};
    bool valid = false;            // a table of the current result is kept (dskgpu_ctx::drop_result and dskgpu_filter_rows drop it)
    void release() { table.release(); stats = dskgpu_read_summary_stats{}; valid = false; }
};

// The colour matrix of the rows (colors.hip), kept from dskgpu_colors_begin until the rows change: u32 C[n_rows][n_colors], row-major.
struct Colors {
    DevBuf C;
    u32 n_colors = 0;
    u64 n_rows = 0;                // the rows of the result it was begun for
    bool valid = false;            // a matrix of the current result is kept (dskgpu_ctx::drop_result and dskgpu_filter_rows drop it)
    void release() { C.release(); n_colors = 0; n_rows = 0; valid = false; }
};

// The rows that dskgpu_filter_rows kept (rowfilter.hip): two sets of row arrays, so that a filter of filtered rows reads one set and writes the
// other; cur = the set res_w / res_ab point into, -1 = the result is still the count's own.  part_off: DSKGPU_F_PARTITION_ORDER, the first
// kept row of every partition (n_parts + 1 entries) -- rows_partition_range reads them instead of the row sort's while cur >= 0.
// The rest is scratch: scan = the exclusive scan of the keep flags, rec = the record a round reads back ([REC_COUNTERS counters | new
// partition offsets]), off_in = the old partition offsets on the device; info / len / bits / keep = the tip rule's per-unitig and per-row
// bytes; the bubble rule uses len / bits / keep too and ends = the two ends of every candidate, one word per unitig; the
// connection rule uses info / len / bits / keep (rules.hip).
// Like the index and the compaction it is kept between calls (9 bytes per row + 14 per unitig of the largest call), so that a caller
// who drives the rounds pays no allocation per round, and goes with the result (dskgpu_ctx::drop_result).
struct Filtered {
    DevBuf w[2][4], ab[2];
    int cur = -1;
    std::vector<u64> part_off;
    DevBuf scan, tmp, rec, off_in, info, len, bits, keep, ends;
    void release() {
        for (int s = 0; s < 2; ++s) { for (int x = 0; x < 4; ++x) w[s][x].release(); ab[s].release(); }
        for (DevBuf* b : {&scan, &tmp, &rec, &off_in, &info, &len, &bits, &keep, &ends}) b->release();
        cur = -1; part_off.clear();
    }
};

// The super-k-mer sender's state (sender.hip): what k_sk_sample / k_sk_hist / k_sk_scatter are launched with and what they leave behind.
// A context has two: `sender`, the multi-GPU exchange's (G = world size; configured by dskgpu_create and dskgpu_mg_set_table), and
// `l0_sender`, the record-based level 0's of a multi-pass count (G = passes, a table and per-owner layout of its own: rec_l0_*) -- so a
// count never touches the owners or the table the caller's exchange works with.  k, m and R are the same in both (dskgpu_create).
struct Sender {
    SkParams sp{};
    std::vector<uint8_t> h_table;  // the repartition table in use (SK_BUCKETS owners; default: bucket scaled to G)
    bool table_dirty = true;       // h_table not yet copied to `table`
    DevBuf table, load;            // the table on the device; the sampled k-mer load of every minimizer bucket (k_sk_sample)
    DevBuf sent;                   // [k-mers sent per owner | sampled k-mers per owner | overflow flag of a sliced step]
    DevBuf lay;                    // level 0: [region base per owner: u64 x 64][slice per owner: u32 x 64] of a sweep
    DevBuf cb64;                   // exact layout: h_cb64 on the device (k_sk_scatter<false>)
    bool prepared = false;         // the send layout below is that of the current reads and ctx->packed / mat1 still hold what it was made from
    bool slices = false;           // the prepared send layout is slices from a sampled estimate (else exact offsets)
    bool exact = false;            // a slice overflowed on these reads: exact counts from now on
    u32 nslices = 0;               // dskgpu_mg_slices_prepare: slices of the prepared step (0 = none prepared)
    std::vector<u64> h_rstart;     // first RECORD of every owner in the send buffer (64-bit: no limit on a rank's shard)
    std::vector<u32> h_cells;      // records per (owner, chunk) as the sizing pass counted them
    std::vector<u64> h_cb64;       // exact layout: their exclusive scan (owner-major) = record index of every (owner, chunk) pair
    u64 h_sent[SK_MAX_OWNERS] = {0};      // k-mers inside the records the last scatter / sweep wrote for every owner
    u64 h_est[SK_MAX_OWNERS] = {0};       // sampled layout: estimated k-mers per owner (k_sk_hist on every 16th tile, scaled)
    void release() { for (DevBuf* b : {&table, &load, &sent, &lay, &cb64}) b->release(); table_dirty = true; prepared = false; nslices = 0; }
};

// The read stream a context owns (reads.hip): `own` holds the first `len` bytes of what was pushed.  pin / pin_ev / pin_used / pin_next: the two pinned staging
// buffers of the host-to-device copy, the event behind each one's last copy, and the slot the next piece takes.  dskgpu_push_raw: file text parsed on the device; the
// stream's length is on the device (RawState) until raw_finish reads it back -- raw_base / raw_ub: the stream's length before the raw pushes / an upper bound of it now
struct ReadStream {
    DevBuf own; u64 len = 0;
    void* pin[2] = {nullptr, nullptr}; hipEvent_t pin_ev[2] = {nullptr, nullptr}; bool pin_used[2] = {false, false}; int pin_next = 0;
    DevBuf raw_in, raw_blk, raw_boff, raw_bstate, raw_state;
    bool raw_pending = false; u64 raw_base = 0, raw_ub = 0;
    HIDDEN void release() {
        for (DevBuf* b : {&own, &raw_in, &raw_blk, &raw_boff, &raw_bstate, &raw_state}) b->release();
        len = 0; raw_pending = false;
        for (int i = 0; i < 2; ++i) { if (pin[i]) (void)hipHostFree(pin[i]); if (pin_ev[i]) (void)hipEventDestroy(pin_ev[i]); pin[i] = nullptr; pin_ev[i] = nullptr; pin_used[i] = false; }
    }
};

// state of a per-bank count in steps (banks.hip: banks_begin .. banks_finish)
struct BankJob { dskgpu_config cfg; const uint8_t* base; u64 total; std::vector<u64> ends; u64 nu, tot_kmers; u32 passes, retries; bool active = false; };

// Multi-bank mode (banks.hip: solidity kinds, 2-D histogram).  ends: the end offset of every declared bank in the read stream; u_w / u_val:
// the union of the per-bank rows and their (bank, abundance) values, s_w: the rows sorted (the sorted values borrow dskgpu_ctx::s_val);
// m_flag / m_pos / m_sum / gh2d: the merge's solidity flags, their scan, the abundance sums and the 2-D histogram, hist2d its host copy
struct Banks {
    BankJob job{};
    std::vector<u64> ends;
    DevBuf u_w[4], s_w[4], u_val, m_flag, m_pos, m_sum, gh2d;
    std::vector<u64> hist2d;
    void forget_ends() { ends.clear(); }                   // the reads are another read set
    void cut_ends(u64 stream_bytes) { while (!ends.empty() && ends.back() > stream_bytes) ends.pop_back(); }      // the stream was rewound
    void forget_hist2d() { hist2d.clear(); }               // a count without banks has none
    HIDDEN void release() { for (int x = 0; x < 4; ++x) { u_w[x].release(); s_w[x].release(); } for (DevBuf* b : {&u_val, &m_flag, &m_pos, &m_sum, &gh2d}) b->release(); }
};

struct dskgpu_ctx {
    dskgpu_config cfg{};
    Tuning tune;
    int W = 1;
    int words_out = 1;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cu = 256;
    std::string err;

    // input: the current reads, whoever owns the bytes (the caller, or `reads`)
    ReadStream reads;
    const uint8_t* d_reads = nullptr; u64 n_bytes = 0;
    Banks banks;

    DevBuf packed, inval;          // K1 output
    DevBuf bufA, bufB;             // partition ping-pong
    DevBuf mat1, mat2, sums, descs1, descs2, seg, fstart, nsolid, scalars, ghist, gstats, chain_next;
    RowSort rs;
    DevBuf smp_keys;               // records: the sample expanded to a key array (16 slots per candidate record, sentinel pads)
    DevBuf smp_mat, smp_descs, boff;   // sampled level-1 loads: chunk x bin matrix of the sample tiles, their descriptors; per-bin slice offsets
    DevBuf dbg, l0buf; DevBuf hv_lut, hv_collect, hv_buf; // heavy k-mers: bin -> collect slot, collected sample keys; [keys | counts | rows] of the k-mers counted apart
    std::vector<unsigned char> h_hv_lut; std::vector<u32> h_hv_cnt, h_hv_step; std::vector<u64> h_hv_coll, h_hv_keys;
    std::vector<ChunkDesc> h_descs_s, h_descs1, h_descs2; std::vector<u64> h_cbeg; std::vector<u32> h_boff; std::vector<u64> h_mom;
    DevBuf out_w[4], srt_w[4], acc_w[4];   // rows as struct-of-arrays: word i of every row in [i]
    DevBuf out_ab, srt_ab, srt_tmp, srt_idx, srt_idx2, srt_k, srt_k2, abund2, acc_ab;   // srt_k2: one record per row for the multi-word gather
    DevBuf s_val;                  // row sort: the sorted keys of a pass (scratch beside srt_k / srt_idx2); the bank merge borrows it for its sorted values, as it borrows srt_tmp and srt_idx
    // the count path's own buffers, those declared further down included (sk_*, cur_state, back_*, land): a new one goes into this list
    HIDDEN void release() {
        for (DevBuf* b : {&packed, &inval, &bufA, &bufB, &mat1, &mat2, &sums, &descs1, &descs2, &seg, &fstart, &nsolid, &scalars, &ghist, &gstats, &chain_next,
                          &smp_keys, &smp_mat, &smp_descs, &boff, &dbg, &l0buf, &hv_lut, &hv_collect, &hv_buf, &out_ab, &srt_ab, &srt_tmp, &srt_idx, &srt_idx2,
                          &srt_k, &srt_k2, &abund2, &acc_ab, &s_val, &sk_sums, &sk_cbase, &sk_keys, &cur_state, &back_dev}) b->release();
        for (int i = 0; i < 4; ++i) { out_w[i].release(); srt_w[i].release(); acc_w[i].release(); }
        if (back_host) (void)hipHostFree(back_host);
        if (land) (void)hipHostFree(land);
        back_host = land = nullptr;
    }
    u64 max_keys_per_pass = 0;     // 0 = as many as 32-bit offsets allow
    std::vector<u32> h_starts;     // explicit-key exchange: first key of every owner in the send buffer
    // the 2-bit form of the reads (packed / inval) between calls.  Both flags describe ctx->packed, which the count path writes and checks
    // (run_encode, encode_current) as much as the sender does: they stay here, not in Sender
    bool enc_keep = false;         // dskgpu_encode_reads: packed / inval hold the 2-bit form of the current reads and the ASCII bytes are gone (d_reads == nullptr)
    bool enc_fresh = false;        // packed / inval hold the encoding of the current reads, left by dskgpu_mg_sample for the sender's sizing pass of the same step
    // super-k-mer records (superkmer.h): who writes them ...
    bool sk_mode = false;          // 20 <= k <= 64 and no DSKGPU_F_MG_EXPLICIT: the exchange and a multi-pass level 0 use records (sender.sp.R words each)
    Sender sender, l0_sender;
    // ... and who reads them: the receiver (sk_sizes, expand_records, sk_count, the level-1 scatter with SRC 2)
    DevBuf sk_sums, sk_cbase, sk_keys;
    std::vector<u32> h_sk_sums; std::vector<u64> h_sk_cbase;
    // records handed to dskgpu_mg_count: the level-1 scatter reads them directly (SRC 2); expanded lazily for the exact path
    const u64* rec_src = nullptr; u64 rec_n = 0; u64 rec_nch = 0, rec_rpc = 0; bool rec_expanded = false;
    bool rec_sized = false;                  // per-chunk k-mer sums of the records are on the device (k_sk_count ran)
    u64 rec_hint = 0;                        // dskgpu_mg_count_sized: the caller's k-mer total of the records (0 = none)
    bool rec_hint_est = false;               // ... an estimate (sliced step): sizes the fast path only, never checked against the result
    std::vector<u64> rec_slice_end;          // dskgpu_mg_count_sliced: record index where every slice ends; empty = one piece
    dskgpu_slice_gate rec_gate = nullptr; void* rec_gate_user = nullptr; u32 rec_gated = 0;      // slices whose arrival the stream already waits for
    bool rec_gate_failed = false;            // a gate said its slice will never arrive: the count stops (DSKGPU_E_STATE)
    std::vector<u32> h_slice_chunk;          // first level-1 chunk of every slice (+ the end)
    DevBuf cur_state;                        // parked write cursors of the level-1 blocks between the launches of a sliced receive
    // what the counts of the current reads found out about them
    u64 last_rows = 0;             // solid rows of the last count of the current reads (0 = not counted yet): sizes what a multi-pass count keeps free for its rows
    bool rec_l0_off = false;       // these reads do not take the record-based level 0 (a slice of its sampled layout overflowed)
    u64* land = nullptr;                             // 64 KB of pinned host memory: where the small per-step read-backs land (landing())
    DevBuf back_dev; u64* back_host = nullptr;      // the count stage's read-back record (k_gather_back) and its pinned landing zone
    u32 h_back[3] = {0}; u64 h_stats[4] = {0}; u32 h_ovf1 = 0; u64 h_nvalid = 0; bool have_nvalid = false;      // read-back landings; the valid k-mer windows of the reads
    bool sentinel_ok = true;       // the all-ones key is not the mixed form of a canonical k-mer of this k (checked at create)
    bool opt1_off = false;         // same for the histogram-free level-1 scatter (block-owned slices)
    bool mw_v3_off = false;        // the top-word table of k_count2v3 met two k-mers it cannot tell apart on these reads: k_count_mw from now on
    bool opt2_off = false;         // the fixed-capacity level-2 scatter overflowed on these reads: use the exact path   // host landing zone of the async size read-back
    std::vector<const void*> big_lds_fns;   // kernels whose dynamic-LDS limit this context has raised (allow_big_lds)
    u32 h_sc[SC_COUNT] = {0};      // host mirror of the device scalars (kept alive across async copies)

    u32 job_passes = 1;            // passes of the running count as run_pipeline sees them (a pass of a record-based multi-pass count runs as "pass 0 of 1" inside run_one_pass)
    // the solid rows of a single pass handed to the row sort where the count kernel left them (pass_rows; W = 0: the rows are dense).  Four-word
    // rows: under DSKGPU_F_PARTITION_ORDER only -- k_part_sort4 is their one sparse reader; no k-mers counted apart, so no tail
    SparseRows sp_rows;
    SparseRows take_sparse_rows() { const SparseRows r = sp_rows; sp_rows = SparseRows{}; return r; }
    // multi-pass jobs: where a pass may put its dense rows straight away -- the job's accumulators, from row `rows` on (run_pipeline sets it
    // once they are sized; run_one_pass sets `took` when it did: the pass's rows are then already appended)
    struct RowSink { bool active = false, took = false; u32* ab = nullptr; u64* w[4] = {nullptr, nullptr, nullptr, nullptr}; u64 rows = 0, cap = 0; } sink;
    // results
    bool have_result = false;
    u64 n_rows = 0;
    const u64* res_w[4] = {nullptr, nullptr, nullptr, nullptr}; const u32* res_ab = nullptr;
    dskgpu_stats stats{};
    std::vector<u64> hist;
    Query query;
    Unitigs unitigs;
    Threading threading;
    Variants variants;
    ReadSummaries readsum;
    Colors colors;
    Filtered filtered;
    // a count starts, or its result is not to be read: the index of the old rows and their unitigs go with them, and so does their memory
    // -- up to 32 + 8 bytes per row that the count about to run may need (a no-op for a context that was never queried)
    // (dskgpu_destroy frees these owners through it: it has to release(), not invalidate())
    void drop_result() { have_result = false; query.release(); unitigs.release(); threading.release(); variants.release(); readsum.release(); colors.release(); filtered.release(); }
    // the read stream changed: what was learnt about the old reads -- their kept encoding apart (enc_keep: the caller's to clear) -- goes
    void reads_changed() { enc_fresh = false; sender.prepared = false; sender.exact = false; opt2_off = false; opt1_off = false; mw_v3_off = false; rec_l0_off = false; last_rows = 0; }

    // timing
    std::vector<Stage> marks;
    std::vector<hipEvent_t> ev_pool; size_t ev_used = 0;
    std::vector<const char*> st_names; std::vector<float> st_ms;

    void mark(const char* name) {
        if (!(cfg.flags & DSKGPU_F_TIMING)) return;
        if (ev_used == ev_pool.size()) { hipEvent_t e; (void)hipEventCreate(&e); ev_pool.push_back(e); }
        hipEvent_t e = ev_pool[ev_used++];
        (void)hipEventRecord(e, stream);
        marks.push_back({name, e});
    }
    void resolve_marks() {   // after a stream sync; appends to st_names/st_ms
        for (size_t i = 0; i + 1 < marks.size(); ++i) {
            float ms = 0; (void)hipEventElapsedTime(&ms, marks[i].ev, marks[i + 1].ev);
            // one entry per stage name: the passes of a multi-pass count (and the retries of a pass) add up
            size_t at = 0;
            while (at < st_names.size() && std::strcmp(st_names[at], marks[i + 1].name) != 0) ++at;
            if (at == st_names.size()) { st_names.push_back(marks[i + 1].name); st_ms.push_back(ms); } else st_ms[at] += ms;
        }
        marks.clear(); ev_used = 0;
    }
};

#define CK(expr)                                                                             \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            ctx->err = std::string(#expr) + ": " + hipGetErrorString(e_);                    \
            return (e_ == hipErrorOutOfMemory) ? DSKGPU_E_NOMEM : DSKGPU_E_DEVICE;           \
        }                                                                                    \
    } while (0)

#define CKL(what)                                                                            \
    do {                                                                                     \
        hipError_t e_ = hipGetLastError();                                                   \
        if (e_ != hipSuccess) {                                                              \
            ctx->err = std::string(what) + ": " + hipGetErrorString(e_);                     \
            return DSKGPU_E_DEVICE;                                                          \
        }                                                                                    \
    } while (0)

inline int fail(dskgpu_ctx* ctx, int code, const std::string& msg) { ctx->err = msg; return code; }
inline unsigned blocks(u64 items, u64 per_block) { return (unsigned)((items + per_block - 1) / per_block); }      // the grid of a kernel that takes per_block items per block

// dskgpu.hip
int encode_current(dskgpu_ctx* ctx, u64* nwords_out);    // the 2-bit form of the current reads in ctx->packed / inval: encoded now, or kept (dskgpu_encode_reads)
HIDDEN int count_reads(dskgpu_ctx* ctx);                     // count the context's current reads with its configuration (what dskgpu_count runs when there are no banks)
int encode_into(dskgpu_ctx* ctx, const uint8_t* d_bytes, u64 n, u64* packed, u32* inval);      // k_encode of n bytes into (n + 31) / 32 words of the caller's buffers
int run_scan(dskgpu_ctx* ctx, u32* a, const u32* d_len, u64 max_len);
int allow_big_lds(dskgpu_ctx* ctx, const void* fn, int bytes = 160 * 1024);      // (bytes: kernels with static LDS next to the dynamic block ask for what they use)

// reads.hip, banks.hip
int raw_finish(dskgpu_ctx* ctx, u64* lines);             // the raw pushes' result: the stream's length comes back from the device
#define RAW_SYNC(ctx) do { if ((ctx)->reads.raw_pending) { const int e_ = raw_finish(ctx, nullptr); if (e_) return e_; } } while (0)
HIDDEN bool per_bank_job(const dskgpu_ctx* ctx);         // the reads have several banks and the configuration needs them counted one by one
HIDDEN int run_banks(dskgpu_ctx* ctx);                   // ... that count: every bank through count_reads, then the merge

// sender.hip
#define REC_L0_NO 2001             // rec_l0_prepare / _sweep: this input does not take the record path (not an error)
struct RecL0 { u32 G = 0; u64 nch = 0; u32 slice[SK_MAX_OWNERS] = {0}; u64 region[SK_MAX_OWNERS] = {0}; };      // region[o]: records of owner o's region (nch * slice[o])
int rec_l0_prepare(dskgpu_ctx* ctx, Sender& s, u64 nwords, u32 G, RecL0* rl);      // table for G owners + the slice of every owner, both from samples
int rec_l0_sweep(dskgpu_ctx* ctx, Sender& s, const RecL0& rl, u32 olo, u32 ohi, u64 (&base_words)[SK_MAX_OWNERS]);      // the records of owners [olo, ohi) into ctx->l0buf
uint64_t sk_send_capacity_words(dskgpu_ctx* ctx);        // the exchange: words the send buffer must hold for the current reads (sizes the send layout if need be)
int sk_scatter(dskgpu_ctx* ctx, void* d_send, uint64_t capacity_words, uint64_t* send_words);      // ... and the records into it, grouped by owner

// rowsort.hip
int order_rows(dskgpu_ctx* ctx, u64 n, u32 npass, bool loaded = false);      // loaded: the rows of dskgpu_load_rows (equal values allowed, global order, no histogram read-back)
u64 rs_max_rows(const dskgpu_ctx* ctx);
int sort_index_multiword(dskgpu_ctx* ctx, const u64* const* rows, u64 n, int W);
u32 part_sort_nparts(const SparseRows& rows);
int launch_part_sort(dskgpu_ctx* ctx, const SparseRows& rows, RowsOut out, u32* out_ab, u32* d_part_off, u32* d_flag, u32* nparts_out);
u32 rows_partitions(const dskgpu_ctx* ctx);
void rows_partition_range(const dskgpu_ctx* ctx, u32 p, u64* b, u64* e);

// query.hip (QTable: query.h)
struct QTable;
int ensure_index(dskgpu_ctx* ctx);                       // the index of the current result: there already, or enqueued now; no result: DSKGPU_E_STATE
QTable query_table(const dskgpu_ctx* ctx);               // what a kernel takes to probe it
int query_ensure(dskgpu_ctx* ctx, DevBuf& b, size_t bytes, const char* what);
void query_begin(dskgpu_ctx* ctx);                       // stage marks of a call from "query start" on ...
int query_finish(dskgpu_ctx* ctx);                       // ... and the wait for the stream that resolves them

// unitigs.hip
int ensure_compaction(dskgpu_ctx* ctx, const char* who); // the compaction of the current result: there already, or built now (opens the call's stage marks)
int ensure_edges(dskgpu_ctx* ctx, const char* who);      // the edges of the current result's compaction: there already, or built now (opens the call's stage marks)

// rowfilter.hip: the machinery of a round that takes rows out, shared by the rules of rules.hip and by components.hip.  The record of a round
// (Filtered::rec) is [REC_COUNTERS counters of the rule, zeroed | one new offset per entry of old_off]; the last new offset is the kept
// total.  Counter REC_ROWS of every rule is the number of rows it flags
enum { REC_COUNTERS = 4, REC_ROWS = 3 };
int abandon(dskgpu_ctx* ctx, int rc);                    // a call gives up: wait for the stream, forget its stage marks, -> rc
int begin_record(dskgpu_ctx* ctx, bool with_offsets, std::vector<u64>& old_off);      // the record, its counters zeroed; with_offsets: old_off = the partitions' first rows and n_rows
int filter_scan(dskgpu_ctx* ctx, const unsigned char* keep, const std::vector<u64>& old_off);      // enqueue the scan of the keep flags and the new offsets into the record
int read_record(dskgpu_ctx* ctx, std::vector<u64>& h, u64 n_off);      // the round's ONE read-back: REC_COUNTERS + n_off words
int filter_apply(dskgpu_ctx* ctx, const unsigned char* keep, const u64* new_off, u64 n_off);      // the kept rows become the result
// per row, bit 1 of Filtered::bits of its unitig -> d_row_flag (may be null) and, with want_keep, its complement -> Filtered::keep
int flag_rows(dskgpu_ctx* ctx, unsigned char* d_row_flag, bool want_keep);
// a rule: enqueue one round on the current result, whose edges are there (n_rows > 0): the bits of every unitig into Filtered::bits, the
// counters into the record, then flag_rows(d_row_flag, want_keep).  params: the rule's parameter structure
typedef int (*RoundEnqueue)(dskgpu_ctx* ctx, const void* params, unsigned char* d_row_flag, bool want_keep);
// one round, no row changes: counters[REC_COUNTERS] (zero when there are no rows), the bits copied to d_unitig_bits (may be null)
int round_once(dskgpu_ctx* ctx, const char* who, const char* stage, RoundEnqueue enqueue, const void* params, void* d_row_flag, void* d_unitig_bits, u64* counters);
// rounds of (rule -> filter) until a round flags no row or max_rounds rounds have removed rows: counters[REC_COUNTERS] = the sums, *n_rounds
int rounds_run(dskgpu_ctx* ctx, const char* who, const char* stage, u64 max_rounds, RoundEnqueue enqueue, const void* params, u64* counters, u64* n_rounds);

// rules.hip
int bubble_candidates(dskgpu_ctx* ctx, u32 max_nodes);   // enqueue k_bubble_candidates on the current result, whose edges are there: Filtered::ends / ::len
