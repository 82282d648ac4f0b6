// bubbles.hip -- the simple bubbles of the compacted de Bruijn graph found and popped on the device, and tips and bubbles in turn until the
// graph stops changing: dskgpu_graph_bubbles / dskgpu_pop_bubbles / dskgpu_simplify (include/dskgpu.h).  Host side of bubbles.h.
// The bubble rule reads the tables of unitigs.hip (ensure_edges builds them) and nothing else; a round is the round of tips.hip, with its
// record, keep flags, scan and compaction (engine.h): the four counters of the rule and the new partition offsets are read back at once.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "bubbles.h"

static_assert(BS_COUNT == REC_COUNTERS, "the bubble rule's counters are the record's");

namespace {

unsigned blocks(u64 items, u64 per_block) { return (unsigned)((items + per_block - 1) / per_block); }

// enqueue one round of the rule on the current result, whose edges are there: bits per unitig (F.bits), the counters into the record,
// d_row_pop (may be null) and, with want_keep, the keep flags of the rows (F.keep).  n_rows > 0
int bubbles_enqueue(dskgpu_ctx* ctx, const dskgpu_bubble_params& p, unsigned char* d_row_pop, bool want_keep) {
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

void add_round(dskgpu_bubble_stats& t, const u64* h) {
    t.n_candidates += h[BS_CAND]; t.n_in_bubbles += h[BS_IN_BUBBLES]; t.n_popped += h[BS_POPPED]; t.n_rows_popped += h[BS_ROWS];
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
    if (const int rc = ensure_edges(ctx, "dskgpu_graph_bubbles")) return rc;
    dskgpu_bubble_stats t{};
    if (ctx->n_rows == 0) {
        if (const int rc = query_finish(ctx)) return rc;
        if (stats) *stats = t;
        return DSKGPU_OK;
    }
    std::vector<u64> old_off, h;
    if (const int rc = begin_record(ctx, false, old_off)) return abandon(ctx, rc);
    if (const int rc = bubbles_enqueue(ctx, *params, static_cast<unsigned char*>(d_row_pop), false)) return abandon(ctx, rc);
    if (d_unitig_bits) CK(hipMemcpyAsync(d_unitig_bits, ctx->filtered.bits.p, ctx->unitigs.stats.n_unitigs, hipMemcpyDeviceToDevice, ctx->stream));
    ctx->mark("bubbles");
    if (const int rc = read_record(ctx, h, 0)) return abandon(ctx, rc);
    if (const int rc = query_finish(ctx)) return rc;
    add_round(t, h.data());
    t.n_rounds = 1; t.n_rows_left = ctx->n_rows - t.n_rows_popped;
    if (stats) *stats = t;
    return DSKGPU_OK;
}

int dskgpu_pop_bubbles(dskgpu_ctx* ctx, const dskgpu_bubble_params* params, dskgpu_bubble_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (const int rc = check_params(ctx, params, "dskgpu_pop_bubbles", true)) return rc;
    const u64 max_rounds = params->max_rounds ? params->max_rounds : 64;
    dskgpu_bubble_stats t{};
    std::vector<u64> old_off, h;
    int rc = DSKGPU_OK;
    for (;;) {
        if ((rc = ensure_edges(ctx, "dskgpu_pop_bubbles"))) break;            // (of the final rows too: the graph is ready when the call returns)
        if (ctx->n_rows == 0 || t.n_rounds == max_rounds) { rc = query_finish(ctx); break; }
        const u64 n = ctx->n_rows;
        if ((rc = begin_record(ctx, true, old_off)) || (rc = bubbles_enqueue(ctx, *params, nullptr, true))) { abandon(ctx, rc); break; }
        ctx->mark("bubbles");
        const unsigned char* keep = ctx->filtered.keep.as<unsigned char>();
        if ((rc = filter_scan(ctx, keep, old_off)) || (rc = read_record(ctx, h, old_off.size()))) { abandon(ctx, rc); break; }
        if (h[BS_POPPED] == 0) { add_round(t, h.data()); rc = query_finish(ctx); break; }
        if (h[BS_ROWS] + h.back() != n) { rc = abandon(ctx, fail(ctx, DSKGPU_E_DEVICE, "dskgpu_pop_bubbles: the popped rows and the kept rows do not add up (internal error)")); break; }
        if ((rc = filter_apply(ctx, keep, h.data() + REC_COUNTERS, old_off.size()))) { abandon(ctx, rc); break; }
        ctx->mark("filter rows");
        add_round(t, h.data());
        ++t.n_rounds;
        if ((rc = query_finish(ctx))) break;
    }
    t.n_rows_left = ctx->n_rows;
    if (stats) *stats = t;
    return rc;
}

int dskgpu_simplify(dskgpu_ctx* ctx, const dskgpu_tip_params* tip_params, const dskgpu_bubble_params* bubble_params, uint32_t max_passes, dskgpu_simplify_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!tip_params && !bubble_params) return fail(ctx, DSKGPU_E_ARG, "dskgpu_simplify: null tip_params and bubble_params");
    if (max_passes > 16) return fail(ctx, DSKGPU_E_ARG, "dskgpu_simplify: max_passes must be in 0..16");
    if (tip_params && (tip_params->max_nodes == 0 || tip_params->max_nodes > B_MAX_NODES || tip_params->max_rounds > 64))
        return fail(ctx, DSKGPU_E_ARG, "dskgpu_simplify: tip_params: max_nodes must be in 1..65535 and max_rounds in 0..64");
    if (bubble_params) if (const int rc = check_params(ctx, bubble_params, "dskgpu_simplify: bubble_params", true)) return rc;
    const u32 passes = max_passes ? max_passes : 16;
    dskgpu_simplify_stats s{};
    int rc = DSKGPU_OK;
    for (u32 pass = 0; pass < passes && rc == DSKGPU_OK; ++pass) {
        dskgpu_tip_stats t{}; dskgpu_bubble_stats b{};
        if (tip_params) rc = dskgpu_clip_tips(ctx, tip_params, &t);            // (an error in either half: what it did is in its stats, and in the sums)
        if (bubble_params && rc == DSKGPU_OK) rc = dskgpu_pop_bubbles(ctx, bubble_params, &b);
        s.tips.n_candidates += t.n_candidates; s.tips.n_tips += t.n_tips; s.tips.n_outranked += t.n_outranked;
        s.tips.n_rows_clipped += t.n_rows_clipped; s.tips.n_rounds += t.n_rounds;
        s.bubbles.n_candidates += b.n_candidates; s.bubbles.n_in_bubbles += b.n_in_bubbles; s.bubbles.n_popped += b.n_popped;
        s.bubbles.n_rows_popped += b.n_rows_popped; s.bubbles.n_rounds += b.n_rounds;
        if (t.n_rows_clipped + b.n_rows_popped == 0) break;
        ++s.n_passes;
    }
    s.n_rows_left = s.tips.n_rows_left = s.bubbles.n_rows_left = ctx->n_rows;
    if (stats) *stats = s;
    return rc;
}

}  // extern "C"
