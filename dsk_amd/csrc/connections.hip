// connections.hip -- the erroneous connections of the compacted de Bruijn graph found and removed on the device: dskgpu_graph_connections /
// dskgpu_remove_connections (include/dskgpu.h; dskgpu_simplify_all is next to dskgpu_simplify in bubbles.hip).  Host side of connections.h.
// The rule reads the tables of unitigs.hip (ensure_edges builds them) and nothing else; a round is the round of tips.hip (round_once /
// rounds_run of engine.h), with its record, keep flags, scan and compaction.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "connections.h"

static_assert(CS_COUNT == REC_COUNTERS && CS_ROWS == REC_ROWS, "the connection rule's counters are the record's");

namespace {

unsigned blocks(u64 items, u64 per_block) { return (unsigned)((items + per_block - 1) / per_block); }

// enqueue one round of the rule on the current result, whose edges are there: bits per unitig (F.bits), the counters into the record,
// d_row_rem (may be null) and, with want_keep, the keep flags of the rows (F.keep).  n_rows > 0
int connections_enqueue(dskgpu_ctx* ctx, const void* params, unsigned char* d_row_rem, bool want_keep) {
    const dskgpu_connection_params& p = *static_cast<const dskgpu_connection_params*>(params);
    Filtered& F = ctx->filtered;
    const Unitigs& U = ctx->unitigs;
    const u64 nu = U.stats.n_unitigs;
    if (const int rc = query_ensure(ctx, F.info, nu, "connection candidates")) return rc;
    if (const int rc = query_ensure(ctx, F.len, nu * 4, "connection lengths")) return rc;
    if (const int rc = query_ensure(ctx, F.bits, nu, "connection bits")) return rc;
    const dim3 ugrid(blocks(nu, 256));
    hipLaunchKernelGGL(k_conn_candidates, ugrid, dim3(256), 0, ctx->stream, U.offsets.as<u64>(), U.kind.as<unsigned char>(), U.ab_sum.as<u64>(), U.e_offsets.as<u64>(),
                       U.e_targets.as<u32>(), nu, U.e_stats.n_edges, (int)ctx->cfg.kmer_size, p.max_nodes, p.max_abundance, F.info.as<unsigned char>(), F.len.as<u32>());
    CKL("k_conn_candidates");
    hipLaunchKernelGGL(k_conn_decide, ugrid, dim3(256), 0, ctx->stream, F.info.as<unsigned char>(), F.len.as<u32>(), U.ab_sum.as<u64>(), U.e_offsets.as<u64>(),
                       U.e_targets.as<u32>(), nu, U.e_stats.n_edges, p.min_ratio, F.bits.as<unsigned char>(), F.rec.as<u64>());
    CKL("k_conn_decide");
    return flag_rows(ctx, d_row_rem, want_keep);
}

void set_counters(dskgpu_connection_stats& t, const u64* h) {
    t.n_candidates = h[CS_CAND]; t.n_one_sided = h[CS_ONE_SIDED]; t.n_removed = h[CS_REMOVED]; t.n_rows_removed = h[CS_ROWS];
}

}  // namespace

int connection_check_params(dskgpu_ctx* ctx, const dskgpu_connection_params* p, const char* who, bool rounds) {
    if (!p) return fail(ctx, DSKGPU_E_ARG, std::string(who) + ": null params");
    if (p->max_nodes == 0 || p->max_nodes > C_MAX_NODES) return fail(ctx, DSKGPU_E_ARG, std::string(who) + ": max_nodes must be in 1..65535");
    if (p->min_ratio < C_MIN_RATIO || p->min_ratio > C_MAX_RATIO) return fail(ctx, DSKGPU_E_ARG, std::string(who) + ": min_ratio must be in 2..255");
    if (rounds && p->max_rounds > 64) return fail(ctx, DSKGPU_E_ARG, std::string(who) + ": max_rounds must be in 0..64");
    return DSKGPU_OK;
}

extern "C" {

int dskgpu_graph_connections(dskgpu_ctx* ctx, const dskgpu_connection_params* params, void* d_row_rem, void* d_unitig_bits, dskgpu_connection_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!d_row_rem && !d_unitig_bits && !stats) return fail(ctx, DSKGPU_E_ARG, "dskgpu_graph_connections: no output pointer");
    if (const int rc = connection_check_params(ctx, params, "dskgpu_graph_connections", false)) return rc;
    u64 h[REC_COUNTERS];
    if (const int rc = round_once(ctx, "dskgpu_graph_connections", "connections", connections_enqueue, params, d_row_rem, d_unitig_bits, h)) return rc;
    dskgpu_connection_stats t{};
    if (ctx->n_rows) { set_counters(t, h); t.n_rounds = 1; t.n_rows_left = ctx->n_rows - t.n_rows_removed; }
    if (stats) *stats = t;
    return DSKGPU_OK;
}

int dskgpu_remove_connections(dskgpu_ctx* ctx, const dskgpu_connection_params* params, dskgpu_connection_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (const int rc = connection_check_params(ctx, params, "dskgpu_remove_connections", true)) return rc;
    u64 h[REC_COUNTERS], n_rounds;
    dskgpu_connection_stats t{};
    const int rc = rounds_run(ctx, "dskgpu_remove_connections", "connections", params->max_rounds ? params->max_rounds : 64, connections_enqueue, params, h, &n_rounds);
    set_counters(t, h);
    t.n_rounds = n_rounds;
    t.n_rows_left = ctx->n_rows;
    if (stats) *stats = t;
    return rc;
}

}  // extern "C"
