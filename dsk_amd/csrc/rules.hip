// rules.hip -- the three rules that simplify the compacted de Bruijn graph on the device -- tips found and clipped, simple bubbles found
// and popped, erroneous connections found and removed -- and the rules in turn until the graph stops changing: dskgpu_graph_tips /
// dskgpu_clip_tips / dskgpu_graph_bubbles / dskgpu_pop_bubbles / dskgpu_graph_connections / dskgpu_remove_connections / dskgpu_simplify /
// dskgpu_simplify_all (include/dskgpu.h).  Host side of tips.h, bubbles.h and connections.h.  A rule reads the tables of unitigs.hip
// (ensure_edges builds them) and nothing else; its round is the round of rowfilter.hip (round_once / rounds_run of engine.h), with its
// record, keep flags, scan and compaction: the four counters of the rule and the new partition offsets are read back at once.
#include <hip/hip_runtime.h>
#include <cstddef>
#include <type_traits>

#include "engine.h"
#include "tips.h"
#include "bubbles.h"
#include "connections.h"

static_assert(R_COUNTERS == REC_COUNTERS && R_ROWS == REC_ROWS, "the rules' counters are the record's");

namespace {

// the stats of a rule as the entry points fill them: the three public structures have this layout, and only the names of the counters differ
struct RuleStats { u64 c[REC_COUNTERS], n_rounds, n_rows_left, reserved[2]; };
template <class S> constexpr bool is_rule_stats() {
    return sizeof(S) == sizeof(RuleStats) && offsetof(S, n_candidates) == offsetof(RuleStats, c) && offsetof(S, n_rounds) == offsetof(RuleStats, n_rounds) &&
           offsetof(S, n_rows_left) == offsetof(RuleStats, n_rows_left) && offsetof(S, reserved) == offsetof(RuleStats, reserved);
}
static_assert(is_rule_stats<dskgpu_tip_stats>() && offsetof(dskgpu_tip_stats, n_rows_clipped) == offsetof(RuleStats, c[REC_ROWS]), "dskgpu_tip_stats is a RuleStats");
static_assert(is_rule_stats<dskgpu_bubble_stats>() && offsetof(dskgpu_bubble_stats, n_rows_popped) == offsetof(RuleStats, c[REC_ROWS]), "dskgpu_bubble_stats is a RuleStats");
static_assert(is_rule_stats<dskgpu_connection_stats>() && offsetof(dskgpu_connection_stats, n_rows_removed) == offsetof(RuleStats, c[REC_ROWS]),
              "dskgpu_connection_stats is a RuleStats");

struct Rule { const char* stage; RoundEnqueue enqueue; };

// enqueue one round of a rule on the current result, whose edges are there: bits per unitig (F.bits), the counters into the record,
// d_row_flag (may be null) and, with want_keep, the keep flags of the rows (F.keep).  n_rows > 0
int tips_enqueue(dskgpu_ctx* ctx, const void* params, unsigned char* d_row_tip, bool want_keep) {
    const dskgpu_tip_params& p = *static_cast<const dskgpu_tip_params*>(params);
    Filtered& F = ctx->filtered;
    const Unitigs& U = ctx->unitigs;
    const u64 nu = U.stats.n_unitigs;
    if (const int rc = query_ensure(ctx, F.info, nu, "tip candidates")) return rc;
    if (const int rc = query_ensure(ctx, F.len, nu * 4, "tip lengths")) return rc;
    if (const int rc = query_ensure(ctx, F.bits, nu, "tip bits")) return rc;
    const dim3 ugrid(blocks(nu, 256));
    hipLaunchKernelGGL(k_tip_candidates, ugrid, dim3(256), 0, ctx->stream, U.offsets.as<u64>(), U.kind.as<unsigned char>(), U.ab_sum.as<u64>(), U.e_offsets.as<u64>(), nu,
                       (int)ctx->cfg.kmer_size, p.max_nodes, p.max_abundance, F.info.as<unsigned char>(), F.len.as<u32>());
    CKL("k_tip_candidates");
    hipLaunchKernelGGL(k_tip_decide, ugrid, dim3(256), 0, ctx->stream, F.info.as<unsigned char>(), F.len.as<u32>(), U.ab_sum.as<u64>(), U.e_offsets.as<u64>(),
                       U.e_targets.as<u32>(), nu, U.e_stats.n_edges, F.bits.as<unsigned char>(), F.rec.as<u64>());
    CKL("k_tip_decide");
    return flag_rows(ctx, d_row_tip, want_keep);
}

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

const Rule TIPS{"tips", tips_enqueue}, BUBBLES{"bubbles", bubbles_enqueue}, CONNECTIONS{"connections", connections_enqueue};

// what is wrong with the parameters of a rule, as the tail of the error text, or null.  rounds: max_rounds counts (the calls that run rounds)
template <class P>
const char* params_fault(const P* p, bool rounds) {
    if (!p) return "null params";
    if (p->max_nodes == 0 || p->max_nodes > R_MAX_NODES) return "max_nodes must be in 1..65535";
    if constexpr (std::is_same<P, dskgpu_connection_params>::value)
        if (p->min_ratio < C_MIN_RATIO || p->min_ratio > C_MAX_RATIO) return "min_ratio must be in 2..255";
    if (rounds && p->max_rounds > 64) return "max_rounds must be in 0..64";
    return nullptr;
}

// the parameter check of every rule: DSKGPU_E_ARG and its text, or DSKGPU_OK
template <class P>
int check_params(dskgpu_ctx* ctx, const P* p, const std::string& who, bool rounds) {
    const char* fault = params_fault(p, rounds);
    return fault ? fail(ctx, DSKGPU_E_ARG, who + ": " + fault) : DSKGPU_OK;
}

// dskgpu_graph_tips and its kin: one round, no row changes.  stats: the rule's public structure, may be null
template <class P, class S>
int rule_once(dskgpu_ctx* ctx, const char* who, const Rule& rule, const P* params, void* d_row_flag, void* d_unitig_bits, S* stats) {
    static_assert(is_rule_stats<S>(), "S is one of the three stats structures");
    if (!ctx) return DSKGPU_E_ARG;
    if (!d_row_flag && !d_unitig_bits && !stats) return fail(ctx, DSKGPU_E_ARG, std::string(who) + ": no output pointer");
    if (const int rc = check_params(ctx, params, who, false)) return rc;
    RuleStats t{};
    if (const int rc = round_once(ctx, who, rule.stage, rule.enqueue, params, d_row_flag, d_unitig_bits, t.c)) return rc;
    if (ctx->n_rows) { t.n_rounds = 1; t.n_rows_left = ctx->n_rows - t.c[REC_ROWS]; }
    if (stats) std::memcpy(stats, &t, sizeof(t));
    return DSKGPU_OK;
}

// dskgpu_clip_tips and its kin: rounds until one takes nothing out.  stats: what was done, whatever the return code
template <class P, class S>
int rule_rounds(dskgpu_ctx* ctx, const char* who, const Rule& rule, const P* params, S* stats) {
    static_assert(is_rule_stats<S>(), "S is one of the three stats structures");
    if (!ctx) return DSKGPU_E_ARG;
    if (const int rc = check_params(ctx, params, who, true)) return rc;
    RuleStats t{};
    const int rc = rounds_run(ctx, who, rule.stage, params->max_rounds ? params->max_rounds : 64, rule.enqueue, params, t.c, &t.n_rounds);
    t.n_rows_left = ctx->n_rows;
    if (stats) std::memcpy(stats, &t, sizeof(t));
    return rc;
}

// sum += part: the four counters and the rounds
template <class S>
void add_stats(S& sum, const S& part) {
    RuleStats a, b;
    std::memcpy(&a, &sum, sizeof(a)); std::memcpy(&b, &part, sizeof(b));
    for (int i = 0; i < REC_COUNTERS; ++i) a.c[i] += b.c[i];
    a.n_rounds += b.n_rounds;
    std::memcpy(&sum, &a, sizeof(a));
}

// passes of (dskgpu_clip_tips, dskgpu_pop_bubbles, dskgpu_remove_connections), a null parameter set skipping its part, until a pass removes
// no row: dskgpu_simplify (no third part) and dskgpu_simplify_all.  s: the sums, whatever the return code
int simplify_passes(dskgpu_ctx* ctx, const std::string& who, const dskgpu_tip_params* tip_params, const dskgpu_bubble_params* bubble_params,
                    const dskgpu_connection_params* connection_params, uint32_t max_passes, dskgpu_simplify_all_stats& s) {
    s = dskgpu_simplify_all_stats{};
    if (max_passes > 16) return fail(ctx, DSKGPU_E_ARG, who + ": max_passes must be in 0..16");
    if (tip_params && params_fault(tip_params, true))                         // (one text for whatever is wrong with them)
        return fail(ctx, DSKGPU_E_ARG, who + ": tip_params: max_nodes must be in 1..65535 and max_rounds in 0..64");
    if (bubble_params) if (const int rc = check_params(ctx, bubble_params, who + ": bubble_params", true)) return rc;
    if (connection_params) if (const int rc = check_params(ctx, connection_params, who + ": connection_params", true)) return rc;
    const u32 passes = max_passes ? max_passes : 16;
    int rc = DSKGPU_OK;
    for (u32 pass = 0; pass < passes && rc == DSKGPU_OK; ++pass) {
        dskgpu_tip_stats t{}; dskgpu_bubble_stats b{}; dskgpu_connection_stats c{};
        if (tip_params) rc = dskgpu_clip_tips(ctx, tip_params, &t);            // (an error in any part: what it did is in its stats, and in the sums)
        if (bubble_params && rc == DSKGPU_OK) rc = dskgpu_pop_bubbles(ctx, bubble_params, &b);
        if (connection_params && rc == DSKGPU_OK) rc = dskgpu_remove_connections(ctx, connection_params, &c);
        add_stats(s.tips, t); add_stats(s.bubbles, b); add_stats(s.connections, c);
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

int dskgpu_graph_tips(dskgpu_ctx* ctx, const dskgpu_tip_params* params, void* d_row_tip, void* d_unitig_tip, dskgpu_tip_stats* stats) {
    return rule_once(ctx, "dskgpu_graph_tips", TIPS, params, d_row_tip, d_unitig_tip, stats);
}

int dskgpu_clip_tips(dskgpu_ctx* ctx, const dskgpu_tip_params* params, dskgpu_tip_stats* stats) {
    return rule_rounds(ctx, "dskgpu_clip_tips", TIPS, params, stats);
}

int dskgpu_graph_bubbles(dskgpu_ctx* ctx, const dskgpu_bubble_params* params, void* d_row_pop, void* d_unitig_bits, dskgpu_bubble_stats* stats) {
    return rule_once(ctx, "dskgpu_graph_bubbles", BUBBLES, params, d_row_pop, d_unitig_bits, stats);
}

int dskgpu_pop_bubbles(dskgpu_ctx* ctx, const dskgpu_bubble_params* params, dskgpu_bubble_stats* stats) {
    return rule_rounds(ctx, "dskgpu_pop_bubbles", BUBBLES, params, stats);
}

int dskgpu_graph_connections(dskgpu_ctx* ctx, const dskgpu_connection_params* params, void* d_row_rem, void* d_unitig_bits, dskgpu_connection_stats* stats) {
    return rule_once(ctx, "dskgpu_graph_connections", CONNECTIONS, params, d_row_rem, d_unitig_bits, stats);
}

int dskgpu_remove_connections(dskgpu_ctx* ctx, const dskgpu_connection_params* params, dskgpu_connection_stats* stats) {
    return rule_rounds(ctx, "dskgpu_remove_connections", CONNECTIONS, params, stats);
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
