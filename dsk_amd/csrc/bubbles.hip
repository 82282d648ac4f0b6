// bubbles.hip -- the simple bubbles of the compacted de Bruijn graph found and popped on the device, and the rules in turn until the graph
// stops changing: dskgpu_graph_bubbles / dskgpu_pop_bubbles / dskgpu_simplify / dskgpu_simplify_all (include/dskgpu.h).  Host side of
// bubbles.h.  The bubble rule reads the tables of unitigs.hip (ensure_edges builds them) and nothing else; a round is the round of tips.hip
// (round_once / rounds_run of engine.h), with its record, keep flags, scan and compaction: the four counters of the rule and the new
// partition offsets are read back at once.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "bubbles.h"

static_assert(BS_COUNT == REC_COUNTERS && BS_ROWS == REC_ROWS, "the bubble rule's counters are the record's");

namespace {

unsigned blocks(u64 items, u64 per_block) { return (unsigned)((items + per_block - 1) / per_block); }

// enqueue one round of the rule on the current result, whose edges are there: bits per unitig (F.bits), the counters into the record,
// d_row_pop (may be null) and, with want_keep, the keep flags of the rows (F.keep).  n_rows > 0
int bubbles_enqueue(dskgpu_ctx* ctx, const void* params, unsigned char* d_row_pop, bool want_keep) {
    const dskgpu_bubble_params& p = *static_cast<const dskgpu_bubble_params*>(params);
    Filtered& F = ctx->filtered;
    const Unitigs& U = ctx->unitigs;
    const u64 nu = U.stats.n_unitigs;
    if (const int rc = bubble_candidates(ctx, p.max_nodes)) return rc;
    if (const int rc = query_ensure(ctx, F.bits, nu, "bubble bits")) return rc;
    hipLaunchKernelGGL(k_bubble_decide, dim3(blocks(nu, 256)), dim3(256), 0, ctx->stream, F.ends.as<u64>(), F.len.as<u32>(), U.ab_sum.as<u64>(), U.e_offsets.as<u64>(), U.e_targets.as<u32>(), nu,
                       U.e_stats.n_edges, p.max_diff, F.bits.as<unsigned char>(), F.rec.as<u64>());
    CKL("k_bubble_decide");
    return flag_rows(ctx, d_row_pop, want_keep);
}

int check_params(dskgpu_ctx* ctx, const dskgpu_bubble_params* p, const char* who, bool rounds) {
    if (!p) return fail(ctx, DSKGPU_E_ARG, std::string(who) + ": null params");
    if (p->max_nodes == 0 || p->max_nodes > B_MAX_NODES) return fail(ctx, DSKGPU_E_ARG, std::string(who) + ": max_nodes must be in 1..65535");
    if (rounds && p->max_rounds > 64) return fail(ctx, DSKGPU_E_ARG, std::string(who) + ": max_rounds must be in 0..64");
    return DSKGPU_OK;
}

void set_counters(dskgpu_bubble_stats& t, const u64* h) {
    t.n_candidates = h[BS_CAND]; t.n_in_bubbles = h[BS_IN_BUBBLES]; t.n_popped = h[BS_POPPED]; t.n_rows_popped = h[BS_ROWS];
}

// passes of (dskgpu_clip_tips, dskgpu_pop_bubbles, dskgpu_remove_connections), a null parameter set skipping its part, until a pass removes
// no row: dskgpu_simplify (no third part) and dskgpu_simplify_all.  s: the sums, whatever the return code
int simplify_passes(dskgpu_ctx* ctx, const char* who, const dskgpu_tip_params* tip_params, const dskgpu_bubble_params* bubble_params,
                    const dskgpu_connection_params* connection_params, uint32_t max_passes, dskgpu_simplify_all_stats& s) {
    s = dskgpu_simplify_all_stats{};
    if (max_passes > 16) return fail(ctx, DSKGPU_E_ARG, std::string(who) + ": max_passes must be in 0..16");
    if (tip_params && (tip_params->max_nodes == 0 || tip_params->max_nodes > B_MAX_NODES || tip_params->max_rounds > 64))
        return fail(ctx, DSKGPU_E_ARG, std::string(who) + ": tip_params: max_nodes must be in 1..65535 and max_rounds in 0..64");
    if (bubble_params) if (const int rc = check_params(ctx, bubble_params, (std::string(who) + ": bubble_params").c_str(), true)) return rc;
    if (connection_params) if (const int rc = connection_check_params(ctx, connection_params, (std::string(who) + ": connection_params").c_str(), true)) return rc;
    const u32 passes = max_passes ? max_passes : 16;
    int rc = DSKGPU_OK;
    for (u32 pass = 0; pass < passes && rc == DSKGPU_OK; ++pass) {
        dskgpu_tip_stats t{}; dskgpu_bubble_stats b{}; dskgpu_connection_stats c{};
        if (tip_params) rc = dskgpu_clip_tips(ctx, tip_params, &t);            // (an error in any part: what it did is in its stats, and in the sums)
        if (bubble_params && rc == DSKGPU_OK) rc = dskgpu_pop_bubbles(ctx, bubble_params, &b);
        if (connection_params && rc == DSKGPU_OK) rc = dskgpu_remove_connections(ctx, connection_params, &c);
        s.tips.n_candidates += t.n_candidates; s.tips.n_tips += t.n_tips; s.tips.n_outranked += t.n_outranked;
        s.tips.n_rows_clipped += t.n_rows_clipped; s.tips.n_rounds += t.n_rounds;
        s.bubbles.n_candidates += b.n_candidates; s.bubbles.n_in_bubbles += b.n_in_bubbles; s.bubbles.n_popped += b.n_popped;
        s.bubbles.n_rows_popped += b.n_rows_popped; s.bubbles.n_rounds += b.n_rounds;
        s.connections.n_candidates += c.n_candidates; s.connections.n_one_sided += c.n_one_sided; s.connections.n_removed += c.n_removed;
        s.connections.n_rows_removed += c.n_rows_removed; s.connections.n_rounds += c.n_rounds;
        if (t.n_rows_clipped + b.n_rows_popped + c.n_rows_removed == 0) break;
        ++s.n_passes;
    }
    s.n_rows_left = s.tips.n_rows_left = s.bubbles.n_rows_left = s.connections.n_rows_left = ctx->n_rows;
    return rc;
}

}  // namespace

// enqueue the candidates of the current result, whose edges are there: Filtered::ends and ::len of every unitig.  variants.hip starts from them too
int bubble_candidates(dskgpu_ctx* ctx, u32 max_nodes) {
    Filtered& F = ctx->filtered;
    const Unitigs& U = ctx->unitigs;
    const u64 nu = U.stats.n_unitigs;
    if (const int rc = query_ensure(ctx, F.ends, nu * 8, "bubble ends")) return rc;
    if (const int rc = query_ensure(ctx, F.len, nu * 4, "bubble lengths")) return rc;
    hipLaunchKernelGGL(k_bubble_candidates, dim3(blocks(nu, 256)), dim3(256), 0, ctx->stream, U.offsets.as<u64>(), U.kind.as<unsigned char>(), U.e_offsets.as<u64>(), U.e_targets.as<u32>(), nu,
                       U.e_stats.n_edges, (int)ctx->cfg.kmer_size, max_nodes, F.ends.as<u64>(), F.len.as<u32>());
    CKL("k_bubble_candidates");
    return DSKGPU_OK;
}

extern "C" {

int dskgpu_graph_bubbles(dskgpu_ctx* ctx, const dskgpu_bubble_params* params, void* d_row_pop, void* d_unitig_bits, dskgpu_bubble_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!d_row_pop && !d_unitig_bits && !stats) return fail(ctx, DSKGPU_E_ARG, "dskgpu_graph_bubbles: no output pointer");
    if (const int rc = check_params(ctx, params, "dskgpu_graph_bubbles", false)) return rc;
    u64 h[REC_COUNTERS];
    if (const int rc = round_once(ctx, "dskgpu_graph_bubbles", "bubbles", bubbles_enqueue, params, d_row_pop, d_unitig_bits, h)) return rc;
    dskgpu_bubble_stats t{};
    if (ctx->n_rows) { set_counters(t, h); t.n_rounds = 1; t.n_rows_left = ctx->n_rows - t.n_rows_popped; }
    if (stats) *stats = t;
    return DSKGPU_OK;
}

int dskgpu_pop_bubbles(dskgpu_ctx* ctx, const dskgpu_bubble_params* params, dskgpu_bubble_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (const int rc = check_params(ctx, params, "dskgpu_pop_bubbles", true)) return rc;
    u64 h[REC_COUNTERS], n_rounds;
    dskgpu_bubble_stats t{};
    const int rc = rounds_run(ctx, "dskgpu_pop_bubbles", "bubbles", params->max_rounds ? params->max_rounds : 64, bubbles_enqueue, params, h, &n_rounds);
    set_counters(t, h);
    t.n_rounds = n_rounds;
    t.n_rows_left = ctx->n_rows;
    if (stats) *stats = t;
    return rc;
}

int dskgpu_simplify(dskgpu_ctx* ctx, const dskgpu_tip_params* tip_params, const dskgpu_bubble_params* bubble_params, uint32_t max_passes, dskgpu_simplify_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!tip_params && !bubble_params) return fail(ctx, DSKGPU_E_ARG, "dskgpu_simplify: null tip_params and bubble_params");
    dskgpu_simplify_all_stats a;
    const int rc = simplify_passes(ctx, "dskgpu_simplify", tip_params, bubble_params, nullptr, max_passes, a);
    if (rc == DSKGPU_E_ARG) return rc;                                       // (nothing ran: stats stays as it is)
    dskgpu_simplify_stats s{};
    s.n_passes = a.n_passes; s.n_rows_left = a.n_rows_left; s.tips = a.tips; s.bubbles = a.bubbles;
    if (stats) *stats = s;
    return rc;
}

int dskgpu_simplify_all(dskgpu_ctx* ctx, const dskgpu_tip_params* tip_params, const dskgpu_bubble_params* bubble_params,
                        const dskgpu_connection_params* connection_params, uint32_t max_passes, dskgpu_simplify_all_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!tip_params && !bubble_params && !connection_params) return fail(ctx, DSKGPU_E_ARG, "dskgpu_simplify_all: null tip_params, bubble_params and connection_params");
    dskgpu_simplify_all_stats a;
    const int rc = simplify_passes(ctx, "dskgpu_simplify_all", tip_params, bubble_params, connection_params, max_passes, a);
    if (rc == DSKGPU_E_ARG) return rc;
    if (stats) *stats = a;
    return rc;
}

}  // extern "C"
