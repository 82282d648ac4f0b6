// graph.hip -- the de Bruijn neighbourhood of k-mers in the last result: dskgpu_graph_adjacency / dskgpu_graph_neighbors
// (include/dskgpu.h).  Host side of graph.h.  Probes the lookup index of query.hip (ensure_index builds it on first use) and owns
// nothing but the 25 degree counters in dskgpu_ctx::query; reads the result (res_w / n_rows) and nothing else of the context.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "graph.h"

namespace {

template <int W>
void launch_rows(dskgpu_ctx* ctx, unsigned char* d_adj, u64* d_deg) {
    const u64 per_block = 256ull * GBatch<W>::R;
    const unsigned grid = (unsigned)((ctx->n_rows + per_block - 1) / per_block);      // (n_rows <= Q_MAX_ROWS: ensure_index)
    RowsIn rows;
    for (int x = 0; x < 4; ++x) rows.w[x] = ctx->res_w[x];
    hipLaunchKernelGGL(k_graph_rows<W>, dim3(grid), dim3(256), 0, ctx->stream, rows, ctx->n_rows, (int)ctx->cfg.kmer_size, query_table(ctx), d_adj, d_deg);
}

template <int W>
void launch_neighbors(dskgpu_ctx* ctx, const u64* keys, u64 n, unsigned char* d_adj) {
    const u64 per_block = 256ull * GBatch<W>::R;
    const unsigned grid = (unsigned)((n + per_block - 1) / per_block);
    hipLaunchKernelGGL(k_graph_neighbors<W>, dim3(grid), dim3(256), 0, ctx->stream, keys, n, ctx->words_out, (int)ctx->cfg.kmer_size, query_table(ctx), d_adj);
}

}  // namespace

extern "C" {

int dskgpu_graph_adjacency(dskgpu_ctx* ctx, void* d_adj, uint64_t* degrees) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!d_adj && !degrees) return fail(ctx, DSKGPU_E_ARG, "dskgpu_graph_adjacency: neither d_adj nor degrees");
    CK(hipSetDevice(ctx->cfg.device));
    query_begin(ctx);
    if (const int rc = ensure_index(ctx)) return rc;
    ctx->mark("query index");
    u64 h_deg[G_DEG_CELLS] = {0};
    if (ctx->n_rows) {
        u64* d_deg = nullptr;
        if (degrees) {
            if (const int rc = query_ensure(ctx, ctx->query.deg, sizeof(h_deg), "degree table")) return rc;
            d_deg = ctx->query.deg.as<u64>();
            CK(hipMemsetAsync(d_deg, 0, sizeof(h_deg), ctx->stream));
        }
        unsigned char* out = static_cast<unsigned char*>(d_adj);
        if (ctx->W == 1) launch_rows<1>(ctx, out, d_deg); else if (ctx->W == 2) launch_rows<2>(ctx, out, d_deg); else launch_rows<4>(ctx, out, d_deg);
        CKL("k_graph_rows");
        ctx->mark("graph");
        if (degrees) CK(hipMemcpyAsync(h_deg, d_deg, sizeof(h_deg), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (const int rc = query_finish(ctx)) return rc;
    if (degrees) std::memcpy(degrees, h_deg, sizeof(h_deg));
    return DSKGPU_OK;
}

int dskgpu_graph_neighbors(dskgpu_ctx* ctx, const void* d_kmers, uint64_t n, void* d_adj) {
    if (!ctx) return DSKGPU_E_ARG;
    if (n == 0) return DSKGPU_OK;
    if (!d_kmers || !d_adj) return fail(ctx, DSKGPU_E_ARG, "dskgpu_graph_neighbors: null pointer");
    if (n > (0x7FFFFFFFull << 8)) return fail(ctx, DSKGPU_E_ARG, "dskgpu_graph_neighbors: more values than one launch takes; split the call");
    CK(hipSetDevice(ctx->cfg.device));
    query_begin(ctx);
    if (const int rc = ensure_index(ctx)) return rc;
    ctx->mark("query index");
    const u64* keys = static_cast<const u64*>(d_kmers); unsigned char* out = static_cast<unsigned char*>(d_adj);
    if (ctx->W == 1) launch_neighbors<1>(ctx, keys, n, out); else if (ctx->W == 2) launch_neighbors<2>(ctx, keys, n, out); else launch_neighbors<4>(ctx, keys, n, out);
    CKL("k_graph_neighbors");
    ctx->mark("graph");
    return query_finish(ctx);
}

}  // extern "C"
