// thread.hip -- reads threaded through the compacted de Bruijn graph: dskgpu_thread_place / _reads / _walks / _support
// (include/dskgpu.h).  Host side of thread.h; owns dskgpu_ctx::threading.  Reads the lookup index, the compaction and the edges
// (ensure_edges builds what is missing) and the result's rows; nothing else of the context.  dskgpu_thread_place encodes the stream into
// the query's two buffers (as dskgpu_query_reads does); dskgpu_thread_reads into scratch of its own, which goes with the placements
// (8 bytes per stream byte) and the block sums when the call returns.  What is kept is the tables of the walks and the two supports.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include "engine.h"
#include "thread.h"

namespace {

constexpr u64 LAUNCH_BLOCKS = 1ull << 30;        // blocks of one launch; a longer stream takes several

TGraph thread_graph(const dskgpu_ctx* ctx) {
    const Unitigs& U = ctx->unitigs;
    return TGraph{U.unitig.as<u32>(), U.pos.as<u32>(), U.offsets.as<u64>(), ctx->n_rows, U.stats.n_unitigs, (int)ctx->cfg.kmer_size};
}

template <int W>
void launch_place(dskgpu_ctx* ctx, const u64* packed, const u32* inval, u64 nwords, u64 nbytes, u32* out_u, u32* out_j, u64* stat) {
    constexpr int TPW = 32 / QBatch<W>::N;
    const u64 nblocks = (nwords * TPW + 255) / 256;
    const bool aligned = ((reinterpret_cast<uintptr_t>(out_u) | reinterpret_cast<uintptr_t>(out_j)) & 15) == 0;
    for (u64 b0 = 0; b0 < nblocks; b0 += LAUNCH_BLOCKS) {
        const unsigned grid = (unsigned)std::min<u64>(LAUNCH_BLOCKS, nblocks - b0);
        if (aligned)
            hipLaunchKernelGGL((k_thread_place<W, true>), dim3(grid), dim3(256), 0, ctx->stream, packed, inval, nwords, nbytes, b0 * 256, query_table(ctx),
                               thread_graph(ctx), out_u, out_j, stat);
        else
            hipLaunchKernelGGL((k_thread_place<W, false>), dim3(grid), dim3(256), 0, ctx->stream, packed, inval, nwords, nbytes, b0 * 256, query_table(ctx),
                               thread_graph(ctx), out_u, out_j, stat);
    }
}

// encode the stream into (packed, inval) and place every position
int place(dskgpu_ctx* ctx, DevBuf& packed, DevBuf& inval, const void* d_bytes, u64 nbytes, u32* out_u, u32* out_j, u64* stat) {
    const u64 nwords = (nbytes + 31) / 32;
    if (const int rc = query_ensure(ctx, packed, (nwords + 1) * 8, "encode buffer")) return rc;
    if (const int rc = query_ensure(ctx, inval, (nwords + 1) * 4, "encode buffer")) return rc;
    if (const int rc = encode_into(ctx, static_cast<const uint8_t*>(d_bytes), nbytes, packed.as<u64>(), inval.as<u32>())) return rc;
    if (ctx->W == 1) launch_place<1>(ctx, packed.as<u64>(), inval.as<u32>(), nwords, nbytes, out_u, out_j, stat);
    else if (ctx->W == 2) launch_place<2>(ctx, packed.as<u64>(), inval.as<u32>(), nwords, nbytes, out_u, out_j, stat);
    else launch_place<4>(ctx, packed.as<u64>(), inval.as<u32>(), nwords, nbytes, out_u, out_j, stat);
    CKL("k_thread_place");
    ctx->mark("thread place");
    return DSKGPU_OK;
}

// the per-position scratch of dskgpu_thread_reads: freed when build() returns, whatever way
struct Scratch {
    DevBuf packed, inval, U, J, heads, nsteps, nplaced, hbase, sbase, pbase, tmp, stat;
    ~Scratch() { for (DevBuf* b : {&packed, &inval, &U, &J, &heads, &nsteps, &nplaced, &hbase, &sbase, &pbase, &tmp, &stat}) b->release(); }
};

int scan64(dskgpu_ctx* ctx, DevBuf& tmp, u64* in, u64* out, u64 n) {
    size_t tmp_bytes = 0;
    CK(rocprim::exclusive_scan(nullptr, tmp_bytes, in, out, 0ull, (size_t)n, rocprim::plus<u64>(), ctx->stream));      // LIBRARY SCAN (rocprim): plumbing, 8 bytes per 1024 positions
    if (const int rc = query_ensure(ctx, tmp, tmp_bytes ? tmp_bytes : 8, "walk scan")) return rc;
    CK(rocprim::exclusive_scan(tmp.p, tmp_bytes, in, out, 0ull, (size_t)n, rocprim::plus<u64>(), ctx->stream));
    return DSKGPU_OK;
}

int build(dskgpu_ctx* ctx, const void* d_bytes, u64 nbytes) {
    Threading& T = ctx->threading;
    const Unitigs& G = ctx->unitigs;
    const u64 nu = G.stats.n_unitigs, ne = G.e_stats.n_edges;
    Scratch S;
    const u64 padded = (nbytes + T_PER + 3) & ~3ull;
    if (const int rc = query_ensure(ctx, S.U, padded * 4, "placements")) return rc;
    if (const int rc = query_ensure(ctx, S.J, padded * 4, "placements")) return rc;
    if (const int rc = query_ensure(ctx, S.stat, TS_COUNT * 8, "thread counters")) return rc;
    CK(hipMemsetAsync(S.stat.p, 0, TS_COUNT * 8, ctx->stream));
    u64* stat = S.stat.as<u64>();
    u32 *U = S.U.as<u32>(), *J = S.J.as<u32>();
    if (const int rc = place(ctx, S.packed, S.inval, d_bytes, nbytes, U, J, stat)) return rc;

    const u64 nblocks = (nbytes + T_BLOCK - 1) / T_BLOCK;
    for (DevBuf* b : {&S.heads, &S.nsteps, &S.nplaced, &S.hbase, &S.sbase, &S.pbase})
        if (const int rc = query_ensure(ctx, *b, (nblocks + 1) * 8, "walk block sums")) return rc;
    u64 *heads = S.heads.as<u64>(), *nsteps = S.nsteps.as<u64>(), *nplaced = S.nplaced.as<u64>(), *hbase = S.hbase.as<u64>(), *sbase = S.sbase.as<u64>(), *pbase = S.pbase.as<u64>();
    CK(hipMemsetAsync(heads + nblocks, 0, 8, ctx->stream));                          // the scans' last input: base[nblocks] = the total
    CK(hipMemsetAsync(nsteps + nblocks, 0, 8, ctx->stream));
    CK(hipMemsetAsync(nplaced + nblocks, 0, 8, ctx->stream));
    for (u64 b0 = 0; b0 < nblocks; b0 += LAUNCH_BLOCKS)
        hipLaunchKernelGGL(k_thread_count, dim3((unsigned)std::min<u64>(LAUNCH_BLOCKS, nblocks - b0)), dim3(256), 0, ctx->stream, U, J, nbytes, b0, heads, nsteps, nplaced);
    CKL("k_thread_count");
    if (const int rc = scan64(ctx, S.tmp, heads, hbase, nblocks + 1)) return rc;
    if (const int rc = scan64(ctx, S.tmp, nsteps, sbase, nblocks + 1)) return rc;
    if (const int rc = scan64(ctx, S.tmp, nplaced, pbase, nblocks + 1)) return rc;
    u64 totals[3] = {0, 0, 0};
    CK(hipMemcpyAsync(&totals[0], hbase + nblocks, 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(&totals[1], sbase + nblocks, 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(&totals[2], pbase + nblocks, 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    const u64 n_walks = totals[0], n_steps = totals[1];
    if (n_walks > n_steps || n_steps > nbytes)
        return fail(ctx, DSKGPU_E_DEVICE, "dskgpu_thread_reads: the walks and the steps do not add up (internal error)");

    if (const int rc = query_ensure(ctx, T.offsets, (n_walks + 1) * 8, "walk offsets")) return rc;
    if (const int rc = query_ensure(ctx, T.steps, (n_steps + 1) * 4, "walk steps")) return rc;
    if (const int rc = query_ensure(ctx, T.first, (n_walks + 1) * 8, "walk firsts")) return rc;
    if (const int rc = query_ensure(ctx, T.last, (n_walks + 1) * 8, "walk lasts")) return rc;
    if (const int rc = query_ensure(ctx, T.ends, (n_walks + 1) * 8, "walk ends")) return rc;
    if (const int rc = query_ensure(ctx, T.usup, (nu + 1) * 8, "unitig support")) return rc;
    if (const int rc = query_ensure(ctx, T.esup, (ne + 1) * 8, "edge support")) return rc;
    CK(hipMemsetAsync(T.usup.p, 0, (nu + 1) * 8, ctx->stream));
    CK(hipMemsetAsync(T.esup.p, 0, (ne + 1) * 8, ctx->stream));
    CK(hipMemsetAsync(T.offsets.p, 0, 8, ctx->stream));                              // (no walk: offsets[0] = 0 whatever the kernel does)
    const TEdges E{G.e_offsets.as<u64>(), G.e_targets.as<u32>(), 2 * nu, ne};
    const TWalks Wk{T.offsets.as<u64>(), T.first.as<u64>(), T.last.as<u64>(), T.steps.as<u32>(), T.ends.as<u32>(), n_walks, n_steps};
    for (u64 b0 = 0; b0 < nblocks; b0 += LAUNCH_BLOCKS)
        hipLaunchKernelGGL(k_thread_emit, dim3((unsigned)std::min<u64>(LAUNCH_BLOCKS, nblocks - b0)), dim3(256), 0, ctx->stream, U, J, nbytes, b0, hbase, sbase, E, nu, Wk,
                           T.usup.as<u64>(), T.esup.as<u64>(), stat);
    CKL("k_thread_emit");
    if (n_walks) {
        const unsigned grid = (unsigned)std::min<u64>((n_walks + 255) / 256, (u64)ctx->num_cu * 8);
        hipLaunchKernelGGL(k_thread_maxsteps, dim3(grid), dim3(256), 0, ctx->stream, T.offsets.as<u64>(), n_walks, stat);
        CKL("k_thread_maxsteps");
    }
    ctx->mark("thread walks");
    u64 h_stat[TS_COUNT] = {0};
    CK(hipMemcpyAsync(h_stat, stat, sizeof(h_stat), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));                                          // the scratch goes when this returns
    if (h_stat[TS_BROKEN])
        return fail(ctx, DSKGPU_E_DEVICE, "dskgpu_thread_reads: a read steps from one unitig to another over no edge of the graph (internal error)");
    T.stats.n_valid = h_stat[TS_VALID]; T.stats.n_placed = totals[2]; T.stats.n_walks = n_walks; T.stats.n_steps = n_steps;
    T.stats.max_steps = h_stat[TS_MAXSTEPS];
    T.n_unitigs = nu; T.n_edges = ne;
    return DSKGPU_OK;
}

}  // namespace

extern "C" {

int dskgpu_thread_place(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, void* d_unitig, void* d_off) {
    if (!ctx) return DSKGPU_E_ARG;
    if (nbytes == 0) return DSKGPU_OK;
    if (!d_bytes) return fail(ctx, DSKGPU_E_ARG, "dskgpu_thread_place: null pointer");
    if (!d_unitig && !d_off) return fail(ctx, DSKGPU_E_ARG, "dskgpu_thread_place: neither d_unitig nor d_off");
    if (const int rc = ensure_edges(ctx, "dskgpu_thread_place")) return rc;
    Query& q = ctx->query;
    if (const int rc = place(ctx, q.packed, q.inval, d_bytes, nbytes, static_cast<u32*>(d_unitig), static_cast<u32*>(d_off), nullptr)) return abandon(ctx, rc);
    return query_finish(ctx);
}

int dskgpu_thread_reads(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, dskgpu_thread_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (nbytes && !d_bytes) return fail(ctx, DSKGPU_E_ARG, "dskgpu_thread_reads: null pointer");
    if (ctx->cfg.world_size > 1)
        return fail(ctx, DSKGPU_E_STATE, "dskgpu_thread_reads: a rank holds only the k-mers it owns; the unitigs of its rows are not the group's (world_size > 1)");
    if (!ctx->have_result) return fail(ctx, DSKGPU_E_STATE, "no result to thread reads through: count first");
    CK(hipSetDevice(ctx->cfg.device));
    Threading& T = ctx->threading;
    T.release();
    if (nbytes == 0) {
        if (const int rc = query_ensure(ctx, T.offsets, 8, "walk offsets")) return rc;
        CK(hipMemsetAsync(T.offsets.p, 0, 8, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        T.valid = true;
        if (stats) *stats = T.stats;
        return DSKGPU_OK;
    }
    if (const int rc = ensure_edges(ctx, "dskgpu_thread_reads")) return rc;
    int rc = build(ctx, d_bytes, nbytes);
    if (rc == DSKGPU_OK) rc = query_finish(ctx); else rc = abandon(ctx, rc);
    if (rc != DSKGPU_OK) { T.release(); return rc; }
    T.valid = true;
    if (stats) *stats = T.stats;
    return DSKGPU_OK;
}

int dskgpu_thread_walks(dskgpu_ctx* ctx, void* d_offsets, void* d_steps, void* d_first, void* d_last, void* d_ends) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!d_offsets && !d_steps && !d_first && !d_last && !d_ends) return fail(ctx, DSKGPU_E_ARG, "dskgpu_thread_walks: no output pointer");
    const Threading& T = ctx->threading;
    if (!T.valid) return fail(ctx, DSKGPU_E_STATE, "dskgpu_thread_walks: no threading is kept: dskgpu_thread_reads first");
    CK(hipSetDevice(ctx->cfg.device));
    const u64 nw = T.stats.n_walks, ns = T.stats.n_steps;
    if (d_offsets) CK(hipMemcpyAsync(d_offsets, T.offsets.p, (nw + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (ns && d_steps) CK(hipMemcpyAsync(d_steps, T.steps.p, ns * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if (nw && d_first) CK(hipMemcpyAsync(d_first, T.first.p, nw * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (nw && d_last) CK(hipMemcpyAsync(d_last, T.last.p, nw * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (nw && d_ends) CK(hipMemcpyAsync(d_ends, T.ends.p, nw * 8, hipMemcpyDeviceToDevice, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return DSKGPU_OK;
}

int dskgpu_thread_support(dskgpu_ctx* ctx, void* d_unitig_support, void* d_edge_support) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!d_unitig_support && !d_edge_support) return fail(ctx, DSKGPU_E_ARG, "dskgpu_thread_support: neither d_unitig_support nor d_edge_support");
    const Threading& T = ctx->threading;
    if (!T.valid) return fail(ctx, DSKGPU_E_STATE, "dskgpu_thread_support: no threading is kept: dskgpu_thread_reads first");
    CK(hipSetDevice(ctx->cfg.device));
    if (T.n_unitigs && d_unitig_support) CK(hipMemcpyAsync(d_unitig_support, T.usup.p, T.n_unitigs * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (T.n_edges && d_edge_support) CK(hipMemcpyAsync(d_edge_support, T.esup.p, T.n_edges * 8, hipMemcpyDeviceToDevice, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return DSKGPU_OK;
}

}  // extern "C"
