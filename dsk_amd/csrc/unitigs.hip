// unitigs.hip -- the rows' de Bruijn graph compacted into unitigs: dskgpu_unitigs / _rows / _table / _stream, and the edges between the
// unitigs: dskgpu_unitig_edges / _edges_table (include/dskgpu.h).  Host side
// of unitigs.h; owns dskgpu_ctx::unitigs.  Probes the lookup index of query.hip (ensure_index builds it on first use) and reads the result
// (res_w / res_ab / n_rows); nothing else of the context.  What is kept after the build is 8 bytes per row and 17 per unitig; the
// links, the ranking words and the scan live only while build() runs.  The edges add 12 bytes per oriented unitig and 4 per edge; their
// target slots and degrees live only while build_edges() runs.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include "engine.h"
#include "unitigs.h"

namespace {

RowsIn result_rows(const dskgpu_ctx* ctx) {
    RowsIn rows;
    for (int x = 0; x < 4; ++x) rows.w[x] = ctx->res_w[x];
    return rows;
}

template <int W>
void launch_links(dskgpu_ctx* ctx, unsigned char* adj, u32* nxt, u64* P) {
    const u64 n = ctx->n_rows;
    const int k = (int)ctx->cfg.kmer_size;
    hipLaunchKernelGGL(k_graph_rows<W>, dim3(blocks(n, 256ull * GBatch<W>::R)), dim3(256), 0, ctx->stream, result_rows(ctx), n, k, query_table(ctx), adj, (u64*)nullptr);
    ctx->mark("graph");
    hipLaunchKernelGGL(k_unitig_links<W>, dim3(blocks(n, 256ull * UBatch<W>::R)), dim3(256), 0, ctx->stream, result_rows(ctx), n, k, query_table(ctx), adj, nxt, P);
}

// the build's scratch: freed when build() returns, whatever way
struct Scratch {
    DevBuf adj, nxt, P, Q, val, scan, tmp, cnt;
    ~Scratch() { for (DevBuf* b : {&adj, &nxt, &P, &Q, &val, &scan, &tmp, &cnt}) b->release(); }
};

int read_back(dskgpu_ctx* ctx, void* dst, const void* src, size_t bytes) {
    CK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return DSKGPU_OK;
}

// rounds of `launch` until one reports nothing new in its counter (the next free one of cnt[]); at most U_ROUNDS
template <class Launch>
int run_phase(dskgpu_ctx* ctx, u32* d_cnt, u32& used, u64& rounds, const char* what, Launch launch) {
    for (int round = 0; round < U_ROUNDS; ++round) {
        launch(d_cnt + used);
        CKL(what);
        u32 h = 0;
        if (const int rc = read_back(ctx, &h, d_cnt + used, sizeof(h))) return rc;
        ++used; ++rounds;
        if (h == 0) return DSKGPU_OK;
    }
    return fail(ctx, DSKGPU_E_DEVICE, std::string("dskgpu_unitigs: ") + what + " has not finished after 33 rounds");
}

int build(dskgpu_ctx* ctx) {
    Unitigs& U = ctx->unitigs;
    const u64 n = ctx->n_rows, n_nodes = 2 * n;
    const int k = (int)ctx->cfg.kmer_size;
    U.stats = dskgpu_unitig_stats{};
    if (n == 0) {
        if (const int rc = query_ensure(ctx, U.offsets, 8, "unitig offsets")) return rc;
        CK(hipMemsetAsync(U.offsets.p, 0, 8, ctx->stream));
        ctx->mark(ctx->tune.unitig_stages ? "unitig numbering" : "unitigs");
        return DSKGPU_OK;
    }
    Scratch S;
    constexpr u32 N_CNT = 3 * U_ROUNDS + 3;                                        // one counter per round of the three phases + the nodes left (twice)
    if (const int rc = query_ensure(ctx, S.adj, n, "unitig adjacency")) return rc;
    if (const int rc = query_ensure(ctx, S.nxt, n_nodes * 4, "unitig links")) return rc;
    if (const int rc = query_ensure(ctx, S.P, n_nodes * 8, "unitig ranks")) return rc;
    if (const int rc = query_ensure(ctx, S.cnt, N_CNT * 4 + US_COUNT * 8, "unitig counters")) return rc;
    CK(hipMemsetAsync(S.cnt.p, 0, N_CNT * 4 + US_COUNT * 8, ctx->stream));
    u32* d_cnt = S.cnt.as<u32>();
    u64* d_stat = reinterpret_cast<u64*>(d_cnt + N_CNT);                            // (N_CNT is even: 8-byte aligned)
    static_assert(N_CNT % 2 == 0, "the statistics follow the counters as 64-bit words");
    u32* nxt = S.nxt.as<u32>(); u64* P = S.P.as<u64>();

    if (ctx->W == 1) launch_links<1>(ctx, S.adj.as<unsigned char>(), nxt, P);
    else if (ctx->W == 2) launch_links<2>(ctx, S.adj.as<unsigned char>(), nxt, P);
    else launch_links<4>(ctx, S.adj.as<unsigned char>(), nxt, P);
    CKL("k_unitig_links");
    if (ctx->tune.unitig_stages) ctx->mark("unitig links");

    // chains: rank towards the head
    u32 used = 0; u64 rounds = 0;
    const unsigned jump_grid = blocks(n_nodes, 256ull * U_JUMP), node_grid = blocks(n_nodes, 256);
    auto jump = [&](u32* c) { hipLaunchKernelGGL(k_unitig_jump, dim3(jump_grid), dim3(256), 0, ctx->stream, P, n_nodes, c); };
    if (const int rc = run_phase(ctx, d_cnt, used, rounds, "the ranking of the chains", jump)) return rc;

    // what is left lies on cycles: none in most inputs, so the nodes left are counted first and Q is only made when there are some
    u32 left = 0;
    hipLaunchKernelGGL(k_unitig_cyc_init, dim3(node_grid), dim3(256), 0, ctx->stream, P, nxt, n_nodes, (u64*)nullptr, d_cnt + used);
    CKL("k_unitig_cyc_init");
    if (const int rc = read_back(ctx, &left, d_cnt + used, sizeof(left))) return rc;
    ++used;
    if (left) {
        if (const int rc = query_ensure(ctx, S.Q, n_nodes * 8, "unitig cycles")) return rc;
        u64* Q = S.Q.as<u64>();
        hipLaunchKernelGGL(k_unitig_cyc_init, dim3(node_grid), dim3(256), 0, ctx->stream, P, nxt, n_nodes, Q, d_cnt + used);
        CKL("k_unitig_cyc_init");
        ++used;
        auto cyc_min = [&](u32* c) { hipLaunchKernelGGL(k_unitig_cyc_min, dim3(jump_grid), dim3(256), 0, ctx->stream, Q, n_nodes, c); };
        if (const int rc = run_phase(ctx, d_cnt, used, rounds, "the minimum of the cycles", cyc_min)) return rc;
        hipLaunchKernelGGL(k_unitig_cyc_cut, dim3(node_grid), dim3(256), 0, ctx->stream, P, Q, nxt, n_nodes);
        CKL("k_unitig_cyc_cut");
        if (const int rc = run_phase(ctx, d_cnt, used, rounds, "the ranking of the cycles", jump)) return rc;
        S.Q.release();
    }
    if (ctx->tune.unitig_stages) ctx->mark("unitig ranking");

    // first nodes -> unitig numbers and the nodes before each
    if (const int rc = query_ensure(ctx, S.val, n * 8, "unitig firsts")) return rc;
    u64* val = S.val.as<u64>();
    const unsigned row_grid = blocks(n, 256);
    hipLaunchKernelGGL(k_unitig_first, dim3(row_grid), dim3(256), 0, ctx->stream, P, nxt, n, val, d_stat);
    CKL("k_unitig_first");
    if (const int rc = query_ensure(ctx, S.scan, n * 8, "unitig scan")) return rc;
    u64* scan = S.scan.as<u64>();
    size_t tmp_bytes = 0;
    CK(rocprim::exclusive_scan(nullptr, tmp_bytes, val, scan, 0ull, (size_t)n, rocprim::plus<u64>(), ctx->stream));      // LIBRARY SCAN (rocprim): plumbing, one pass over 8 bytes per row
    if (const int rc = query_ensure(ctx, S.tmp, tmp_bytes ? tmp_bytes : 8, "unitig scan")) return rc;
    CK(rocprim::exclusive_scan(S.tmp.p, tmp_bytes, val, scan, 0ull, (size_t)n, rocprim::plus<u64>(), ctx->stream));
    u64 last[2] = {0, 0}, h_stat[US_COUNT] = {0};
    CK(hipMemcpyAsync(&last[0], scan + (n - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(&last[1], val + (n - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
    if (const int rc = read_back(ctx, h_stat, d_stat, sizeof(h_stat))) return rc;
    const u64 total = last[0] + last[1], n_unitigs = total >> 32;
    if ((total & 0xFFFFFFFFull) != n || n_unitigs == 0 || n_unitigs > n)
        return fail(ctx, DSKGPU_E_DEVICE, "dskgpu_unitigs: the unitigs do not add up to the rows (internal error)");

    if (const int rc = query_ensure(ctx, U.unitig, n * 4, "unitig numbers")) return rc;
    if (const int rc = query_ensure(ctx, U.pos, n * 4, "unitig positions")) return rc;
    if (const int rc = query_ensure(ctx, U.offsets, (n_unitigs + 1) * 8, "unitig offsets")) return rc;
    if (const int rc = query_ensure(ctx, U.ab_sum, n_unitigs * 8, "unitig abundance sums")) return rc;
    if (const int rc = query_ensure(ctx, U.kind, n_unitigs, "unitig kinds")) return rc;
    CK(hipMemsetAsync(U.ab_sum.p, 0, n_unitigs * 8, ctx->stream));
    hipLaunchKernelGGL(k_unitig_number, dim3(row_grid), dim3(256), 0, ctx->stream, P, scan, ctx->res_ab, n, k, n_unitigs, U.unitig.as<u32>(), U.pos.as<u32>(),
                       U.offsets.as<u64>(), U.ab_sum.as<u64>(), U.kind.as<unsigned char>());
    CKL("k_unitig_number");
    ctx->mark(ctx->tune.unitig_stages ? "unitig numbering" : "unitigs");
    CK(hipStreamSynchronize(ctx->stream));                                          // the scratch goes when this returns
    U.stats.n_unitigs = n_unitigs; U.stats.n_cycles = h_stat[US_CYCLES]; U.stats.n_single = h_stat[US_SINGLE]; U.stats.max_nodes = h_stat[US_MAX];
    U.stats.stream_bytes = n + n_unitigs * (u64)k; U.stats.n_rounds = rounds;
    return DSKGPU_OK;
}

// the compaction of the current result: there already, or built now.  Opens the call's stage marks.
int ensure_unitigs(dskgpu_ctx* ctx, const char* who) {
    if (ctx->cfg.world_size > 1)
        return fail(ctx, DSKGPU_E_STATE, std::string(who) + ": a rank holds only the k-mers it owns; the unitigs of its rows are not the group's (world_size > 1)");
    CK(hipSetDevice(ctx->cfg.device));
    query_begin(ctx);
    if (ctx->have_result && ctx->n_rows > 0x7FFFFFFFull)
        return fail(ctx, DSKGPU_E_STATE, "the result has more than 2^31 - 1 rows: the unitigs number 2 * rows oriented nodes in 32 bits");
    const bool had_index = ctx->query.valid;
    if (const int rc = ensure_index(ctx)) return rc;
    if (!had_index) ctx->mark("query index");
    if (ctx->unitigs.valid) return DSKGPU_OK;
    const int rc = build(ctx);
    if (rc != DSKGPU_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        ctx->unitigs.release(); ctx->marks.clear(); ctx->ev_used = 0;
        return rc;
    }
    ctx->unitigs.valid = true;
    return DSKGPU_OK;
}

int finish(dskgpu_ctx* ctx) {
    const int rc = query_finish(ctx);
    if (rc != DSKGPU_OK) ctx->unitigs.release();
    return rc;
}

template <int W>
void launch_edges(dskgpu_ctx* ctx, u32* slots, u64* deg, u64* stat) {
    const Unitigs& U = ctx->unitigs;
    hipLaunchKernelGGL(k_unitig_edges<W>, dim3(blocks(2 * U.stats.n_unitigs, 256ull * UEBatch<W>::R)), dim3(256), 0, ctx->stream, result_rows(ctx), ctx->n_rows,
                       (int)ctx->cfg.kmer_size, query_table(ctx), U.unitig.as<u32>(), U.ends.as<u32>(), U.stats.n_unitigs, slots, deg, stat);
}

// the scratch of the edges: freed when build_edges() returns, whatever way
struct EdgeScratch {
    DevBuf slots, deg, tmp, stat;
    ~EdgeScratch() { for (DevBuf* b : {&slots, &deg, &tmp, &stat}) b->release(); }
};

int build_edges(dskgpu_ctx* ctx) {
    Unitigs& U = ctx->unitigs;
    const u64 n = ctx->n_rows, nu = U.stats.n_unitigs, n_or = 2 * nu;
    U.e_stats = dskgpu_unitig_edge_stats{};
    if (const int rc = query_ensure(ctx, U.e_offsets, (n_or + 1) * 8, "unitig edge offsets")) return rc;
    if (n == 0) {
        CK(hipMemsetAsync(U.e_offsets.p, 0, 8, ctx->stream));
        ctx->mark("unitig edges");
        return DSKGPU_OK;
    }
    EdgeScratch S;
    if (const int rc = query_ensure(ctx, U.ends, n_or * 4, "unitig ends")) return rc;
    if (const int rc = query_ensure(ctx, S.slots, n_or * 16, "unitig edge slots")) return rc;
    if (const int rc = query_ensure(ctx, S.deg, (n_or + 1) * 8, "unitig degrees")) return rc;
    if (const int rc = query_ensure(ctx, S.stat, UE_COUNT * 8, "unitig edge counters")) return rc;
    CK(hipMemsetAsync(U.ends.p, 0xFF, n_or * 4, ctx->stream));
    CK(hipMemsetAsync(S.deg.as<u64>() + n_or, 0, 8, ctx->stream));                   // the scan's last input: offsets[n_or] = n_edges
    CK(hipMemsetAsync(S.stat.p, 0, UE_COUNT * 8, ctx->stream));
    hipLaunchKernelGGL(k_unitig_ends, dim3(blocks(n, 256)), dim3(256), 0, ctx->stream, U.unitig.as<u32>(), U.pos.as<u32>(), U.offsets.as<u64>(), n,
                       (int)ctx->cfg.kmer_size, nu, U.ends.as<u32>());
    CKL("k_unitig_ends");
    u64* deg = S.deg.as<u64>(); u64* stat = S.stat.as<u64>();
    if (ctx->W == 1) launch_edges<1>(ctx, S.slots.as<u32>(), deg, stat);
    else if (ctx->W == 2) launch_edges<2>(ctx, S.slots.as<u32>(), deg, stat);
    else launch_edges<4>(ctx, S.slots.as<u32>(), deg, stat);
    CKL("k_unitig_edges");
    u64* off = U.e_offsets.as<u64>();
    size_t tmp_bytes = 0;
    CK(rocprim::exclusive_scan(nullptr, tmp_bytes, deg, off, 0ull, (size_t)(n_or + 1), rocprim::plus<u64>(), ctx->stream));      // LIBRARY SCAN (rocprim): plumbing, 8 bytes per oriented unitig
    if (const int rc = query_ensure(ctx, S.tmp, tmp_bytes ? tmp_bytes : 8, "unitig edge scan")) return rc;
    CK(rocprim::exclusive_scan(S.tmp.p, tmp_bytes, deg, off, 0ull, (size_t)(n_or + 1), rocprim::plus<u64>(), ctx->stream));
    u64 total = 0, h_stat[UE_COUNT] = {0};
    CK(hipMemcpyAsync(&total, off + n_or, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (const int rc = read_back(ctx, h_stat, stat, sizeof(h_stat))) return rc;
    if (h_stat[UE_BROKEN] || total != h_stat[UE_EDGES] || total > 4 * n_or || h_stat[UE_MAXDEG] > 4)
        return fail(ctx, DSKGPU_E_DEVICE, "dskgpu_unitig_edges: an edge does not lead to the end of a unitig, or the degrees do not add up (internal error)");
    if (const int rc = query_ensure(ctx, U.e_targets, total ? total * 4 : 4, "unitig edge targets")) return rc;
    hipLaunchKernelGGL(k_unitig_edge_fill, dim3(blocks(n_or, 256)), dim3(256), 0, ctx->stream, S.slots.as<u32>(), off, n_or, total, U.e_targets.as<u32>());
    CKL("k_unitig_edge_fill");
    ctx->mark("unitig edges");
    CK(hipStreamSynchronize(ctx->stream));                                          // the scratch goes when this returns
    U.e_stats.n_edges = total; U.e_stats.n_self = h_stat[UE_SELF]; U.e_stats.n_dead_ends = h_stat[UE_DEAD]; U.e_stats.max_degree = h_stat[UE_MAXDEG];
    return DSKGPU_OK;
}

}  // namespace

// the compaction alone, for a caller outside this file that needs no edges (colors.hip)
int ensure_compaction(dskgpu_ctx* ctx, const char* who) { return ensure_unitigs(ctx, who); }

// the edges of the current result's compaction: there already, or built now (the compaction and the index below them too).  rowfilter.hip calls it.
int ensure_edges(dskgpu_ctx* ctx, const char* who) {
    if (const int rc = ensure_unitigs(ctx, who)) return rc;
    if (ctx->unitigs.e_valid) return DSKGPU_OK;
    const int rc = build_edges(ctx);
    if (rc != DSKGPU_OK) {                                                          // the compaction stays: it is whole
        (void)hipStreamSynchronize(ctx->stream);
        ctx->unitigs.release_edges(); ctx->marks.clear(); ctx->ev_used = 0;
        return rc;
    }
    ctx->unitigs.e_valid = true;
    return DSKGPU_OK;
}

extern "C" {

int dskgpu_unitigs(dskgpu_ctx* ctx, dskgpu_unitig_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (const int rc = ensure_unitigs(ctx, "dskgpu_unitigs")) return rc;
    if (const int rc = finish(ctx)) return rc;
    if (stats) *stats = ctx->unitigs.stats;
    return DSKGPU_OK;
}

int dskgpu_unitigs_rows(dskgpu_ctx* ctx, void* d_unitig, void* d_pos) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!d_unitig && !d_pos) return fail(ctx, DSKGPU_E_ARG, "dskgpu_unitigs_rows: neither d_unitig nor d_pos");
    if (const int rc = ensure_unitigs(ctx, "dskgpu_unitigs_rows")) return rc;
    const Unitigs& U = ctx->unitigs;
    const u64 n = ctx->n_rows;
    if (n && d_unitig) CK(hipMemcpyAsync(d_unitig, U.unitig.p, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if (n && d_pos) CK(hipMemcpyAsync(d_pos, U.pos.p, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return finish(ctx);
}

int dskgpu_unitigs_table(dskgpu_ctx* ctx, void* d_offsets, void* d_ab_sum, void* d_kind) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!d_offsets && !d_ab_sum && !d_kind) return fail(ctx, DSKGPU_E_ARG, "dskgpu_unitigs_table: no output pointer");
    if (const int rc = ensure_unitigs(ctx, "dskgpu_unitigs_table")) return rc;
    const Unitigs& U = ctx->unitigs;
    const u64 nu = U.stats.n_unitigs;
    if (d_offsets) CK(hipMemcpyAsync(d_offsets, U.offsets.p, (nu + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (nu && d_ab_sum) CK(hipMemcpyAsync(d_ab_sum, U.ab_sum.p, nu * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (nu && d_kind) CK(hipMemcpyAsync(d_kind, U.kind.p, nu, hipMemcpyDeviceToDevice, ctx->stream));
    return finish(ctx);
}

int dskgpu_unitigs_stream(dskgpu_ctx* ctx, void* d_bytes, uint64_t capacity) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!d_bytes) return fail(ctx, DSKGPU_E_ARG, "dskgpu_unitigs_stream: null pointer");
    if (const int rc = ensure_unitigs(ctx, "dskgpu_unitigs_stream")) return rc;
    const Unitigs& U = ctx->unitigs;
    if (capacity < U.stats.stream_bytes) {
        (void)finish(ctx);
        return fail(ctx, DSKGPU_E_ARG, "dskgpu_unitigs_stream: capacity " + std::to_string(capacity) + " < stream_bytes " + std::to_string(U.stats.stream_bytes));
    }
    const u64 n = ctx->n_rows;
    if (n) {
        const int k = (int)ctx->cfg.kmer_size;
        const dim3 grid(blocks(n, 256));
        unsigned char* out = static_cast<unsigned char*>(d_bytes);
        if (ctx->W == 1) hipLaunchKernelGGL(k_unitig_stream<1>, grid, dim3(256), 0, ctx->stream, result_rows(ctx), n, k, U.unitig.as<u32>(), U.pos.as<u32>(), U.offsets.as<u64>(), U.stats.n_unitigs, out);
        else if (ctx->W == 2) hipLaunchKernelGGL(k_unitig_stream<2>, grid, dim3(256), 0, ctx->stream, result_rows(ctx), n, k, U.unitig.as<u32>(), U.pos.as<u32>(), U.offsets.as<u64>(), U.stats.n_unitigs, out);
        else hipLaunchKernelGGL(k_unitig_stream<4>, grid, dim3(256), 0, ctx->stream, result_rows(ctx), n, k, U.unitig.as<u32>(), U.pos.as<u32>(), U.offsets.as<u64>(), U.stats.n_unitigs, out);
        CKL("k_unitig_stream");
    }
    ctx->mark("unitig stream");
    return finish(ctx);
}

int dskgpu_unitig_edges(dskgpu_ctx* ctx, dskgpu_unitig_edge_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (const int rc = ensure_edges(ctx, "dskgpu_unitig_edges")) return rc;
    if (const int rc = finish(ctx)) return rc;
    if (stats) *stats = ctx->unitigs.e_stats;
    return DSKGPU_OK;
}

int dskgpu_unitig_edges_table(dskgpu_ctx* ctx, void* d_offsets, void* d_targets, void* d_ends) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!d_offsets && !d_targets && !d_ends) return fail(ctx, DSKGPU_E_ARG, "dskgpu_unitig_edges_table: no output pointer");
    if (const int rc = ensure_edges(ctx, "dskgpu_unitig_edges_table")) return rc;
    const Unitigs& U = ctx->unitigs;
    const u64 n_or = 2 * U.stats.n_unitigs, ne = U.e_stats.n_edges;
    if (d_offsets) CK(hipMemcpyAsync(d_offsets, U.e_offsets.p, (n_or + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (ne && d_targets) CK(hipMemcpyAsync(d_targets, U.e_targets.p, ne * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if (n_or && d_ends) CK(hipMemcpyAsync(d_ends, U.ends.p, n_or * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return finish(ctx);
}

}  // extern "C"
