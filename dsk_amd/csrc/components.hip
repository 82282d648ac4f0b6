// components.hip -- the connected components of the compacted de Bruijn graph on the device, and the small ones taken out of the result:
// dskgpu_components / _components_labels / _components_table / dskgpu_graph_small_components / dskgpu_drop_components (include/dskgpu.h).
// Host side of components.h; owns dskgpu_ctx::unitigs.cc.  The build reads the tables of unitigs.hip (ensure_edges builds them) and nothing
// else, and reads back two small records: the number of components, which sizes the table, and its counters.  The components go wherever
// the edges go (Unitigs::release_edges / ::invalidate).  Removing the small ones is the round of rowfilter.hip with its record, keep flags, scan
// and compaction (engine.h) -- one round: whole components go, so no adjacency byte of a kept row changes.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "engine.h"
#include "components.h"

static_assert(CR_COUNT == REC_COUNTERS, "the small-component counters are the record's");

namespace {

// the scratch of the build (12 bytes per unitig + the scan's): freed when build() returns, whatever way
struct Scratch {
    DevBuf parent, label, rank, tmp, stat;
    ~Scratch() { for (DevBuf* b : {&parent, &label, &rank, &tmp, &stat}) b->release(); }
};

int build(dskgpu_ctx* ctx) {
    Unitigs& U = ctx->unitigs;
    Components& X = U.cc;
    const u64 nu = U.stats.n_unitigs;
    X.stats = dskgpu_component_stats{};
    if (nu == 0) { ctx->mark("components"); return DSKGPU_OK; }
    Scratch S;
    if (const int rc = query_ensure(ctx, X.comp, nu * 4, "component labels")) return rc;
    if (const int rc = query_ensure(ctx, S.parent, nu * 4, "component parents")) return rc;
    if (const int rc = query_ensure(ctx, S.label, nu * 4, "component roots")) return rc;
    if (const int rc = query_ensure(ctx, S.rank, nu * 4, "component ranks")) return rc;
    if (const int rc = query_ensure(ctx, S.stat, CM_COUNT * 8, "component counters")) return rc;
    u32 *parent = S.parent.as<u32>(), *label = S.label.as<u32>(), *rank = S.rank.as<u32>(); u64* stat = S.stat.as<u64>();
    const dim3 ugrid(blocks(nu, 256));
    CK(hipMemsetAsync(stat, 0, CM_COUNT * 8, ctx->stream));
    // 1. the labelling: three launches whatever the graph
    hipLaunchKernelGGL(k_cc_init, ugrid, dim3(256), 0, ctx->stream, parent, nu);
    CKL("k_cc_init");
    hipLaunchKernelGGL(k_cc_hook, ugrid, dim3(256), 0, ctx->stream, U.e_offsets.as<u64>(), U.e_targets.as<u32>(), nu, U.e_stats.n_edges, parent, stat);
    CKL("k_cc_hook");
    hipLaunchKernelGGL(k_cc_flatten, ugrid, dim3(256), 0, ctx->stream, parent, nu, label, stat);
    CKL("k_cc_flatten");
    if (ctx->tune.cc_stages) ctx->mark("component labelling");
    // 2. the numbering
    auto flags = rocprim::make_transform_iterator(rocprim::counting_iterator<u32>(0u), CRootFlag{label});
    size_t tmp_bytes = 0;
    CK(rocprim::exclusive_scan(nullptr, tmp_bytes, flags, rank, 0u, (size_t)nu, rocprim::plus<u32>(), ctx->stream));      // LIBRARY SCAN (rocprim): plumbing, 4 bytes per unitig
    if (const int rc = query_ensure(ctx, S.tmp, tmp_bytes ? tmp_bytes : 8, "component scan")) return rc;
    CK(rocprim::exclusive_scan(S.tmp.p, tmp_bytes, flags, rank, 0u, (size_t)nu, rocprim::plus<u32>(), ctx->stream));
    u32 h_last[2] = {0, 0}; u64 h_stat[CM_COUNT] = {0};
    CK(hipMemcpyAsync(&h_last[0], rank + (nu - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(&h_last[1], label + (nu - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(h_stat, stat, sizeof(h_stat), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    const u64 n_c = (u64)h_last[0] + ((u64)h_last[1] == nu - 1 ? 1 : 0);
    if (h_stat[CM_BROKEN] || n_c == 0 || n_c > nu)
        return fail(ctx, DSKGPU_E_DEVICE, "dskgpu_components: the union-find did not settle, or a root is missing (internal error)");
    if (const int rc = query_ensure(ctx, X.first, n_c * 4, "component table")) return rc;
    if (const int rc = query_ensure(ctx, X.cols, CC_COUNT * n_c * 8, "component table")) return rc;
    hipLaunchKernelGGL(k_cc_number, ugrid, dim3(256), 0, ctx->stream, label, rank, nu, n_c, X.comp.as<u32>(), X.first.as<u32>());
    CKL("k_cc_number");
    if (ctx->tune.cc_stages) ctx->mark("component numbering");
    // 3. the table
    u64* cols = X.cols.as<u64>();
    CK(hipMemsetAsync(cols, 0, CC_COUNT * n_c * 8, ctx->stream));
    const dim3 tgrid(blocks(nu, CC_BLOCK));
    const int k = (int)ctx->cfg.kmer_size;
    if (ctx->tune.cc_plain)
        hipLaunchKernelGGL(k_cc_table<false>, tgrid, dim3(CC_BLOCK), 0, ctx->stream, X.comp.as<u32>(), U.offsets.as<u64>(), U.ab_sum.as<u64>(), U.e_offsets.as<u64>(), nu, k, n_c, cols);
    else
        hipLaunchKernelGGL(k_cc_table<true>, tgrid, dim3(CC_BLOCK), 0, ctx->stream, X.comp.as<u32>(), U.offsets.as<u64>(), U.ab_sum.as<u64>(), U.e_offsets.as<u64>(), nu, k, n_c, cols);
    CKL("k_cc_table");
    hipLaunchKernelGGL(k_cc_stats, dim3(blocks(n_c, 256)), dim3(256), 0, ctx->stream, cols, n_c, stat);
    CKL("k_cc_stats");
    ctx->mark(ctx->tune.cc_stages ? "component table" : "components");
    CK(hipMemcpyAsync(h_stat, stat, sizeof(h_stat), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));                                          // the scratch goes when this returns
    X.stats.n_components = n_c; X.stats.n_single = h_stat[CM_SINGLE]; X.stats.max_unitigs = h_stat[CM_MAXU]; X.stats.max_rows = h_stat[CM_MAXR];
    X.stats.n_rounds = 3;
    return DSKGPU_OK;
}

// the components of the current result's compaction: there already, or built now (the edges, the compaction and the index below them too).
// Opens the call's stage marks
int ensure_components(dskgpu_ctx* ctx, const char* who) {
    if (const int rc = ensure_edges(ctx, who)) return rc;
    Components& X = ctx->unitigs.cc;
    if (X.valid) return DSKGPU_OK;
    const int rc = build(ctx);
    if (rc != DSKGPU_OK) {                                                          // the edges stay: they are whole
        (void)hipStreamSynchronize(ctx->stream);
        X.release(); ctx->marks.clear(); ctx->ev_used = 0;
        return rc;
    }
    X.valid = true;
    return DSKGPU_OK;
}

int check_params(dskgpu_ctx* ctx, const dskgpu_component_params* p, const char* who) {
    if (!p) return fail(ctx, DSKGPU_E_ARG, std::string(who) + ": null params");
    if (p->min_rows == 0) return fail(ctx, DSKGPU_E_ARG, std::string(who) + ": min_rows must be at least 1");
    return DSKGPU_OK;
}

// enqueue the rule on the components, which are there: the flag of every component (Filtered::bits), the counters into the record, d_row_drop
// (may be null) and, with want_keep, the keep flags of the rows (Filtered::keep).  n_rows > 0
int small_enqueue(dskgpu_ctx* ctx, const dskgpu_component_params& p, unsigned char* d_row_drop, bool want_keep) {
    Filtered& F = ctx->filtered;
    const Unitigs& U = ctx->unitigs;
    const Components& X = U.cc;
    const u64 n = ctx->n_rows, n_c = X.stats.n_components;
    if (const int rc = query_ensure(ctx, F.bits, n_c, "small components")) return rc;
    if (want_keep) if (const int rc = query_ensure(ctx, F.keep, n, "keep flags")) return rc;
    hipLaunchKernelGGL(k_cc_small, dim3(blocks(n_c, 256)), dim3(256), 0, ctx->stream, X.cols.as<u64>(), n_c, p.min_rows, p.max_abundance, F.bits.as<unsigned char>(), F.rec.as<u64>());
    CKL("k_cc_small");
    if (d_row_drop || want_keep) {
        hipLaunchKernelGGL(k_cc_rows<true>, dim3(blocks(n, 256 * 16)), dim3(256), 0, ctx->stream, U.unitig.as<u32>(), X.comp.as<u32>(), F.bits.as<unsigned char>(), n,
                           U.stats.n_unitigs, n_c, (u32*)nullptr, d_row_drop, want_keep ? F.keep.as<unsigned char>() : (unsigned char*)nullptr);
        CKL("k_cc_rows");
    }
    return DSKGPU_OK;
}

void set_drop(dskgpu_component_drop_stats& t, const u64* h) { t.n_small = h[CR_SMALL]; t.n_unitigs_dropped = h[CR_UNITIGS]; t.n_rows_dropped = h[CR_ROWS]; }

}  // namespace

extern "C" {

int dskgpu_components(dskgpu_ctx* ctx, dskgpu_component_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (const int rc = ensure_components(ctx, "dskgpu_components")) return rc;
    if (const int rc = query_finish(ctx)) return rc;
    if (stats) *stats = ctx->unitigs.cc.stats;
    return DSKGPU_OK;
}

int dskgpu_components_labels(dskgpu_ctx* ctx, void* d_unitig_comp, void* d_row_comp) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!d_unitig_comp && !d_row_comp) return fail(ctx, DSKGPU_E_ARG, "dskgpu_components_labels: neither d_unitig_comp nor d_row_comp");
    if (const int rc = ensure_components(ctx, "dskgpu_components_labels")) return rc;
    const Unitigs& U = ctx->unitigs;
    const u64 n = ctx->n_rows, nu = U.stats.n_unitigs;
    if (nu && d_unitig_comp) CK(hipMemcpyAsync(d_unitig_comp, U.cc.comp.p, nu * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if (n && d_row_comp) {
        hipLaunchKernelGGL(k_cc_rows<false>, dim3(blocks(n, 256 * 4)), dim3(256), 0, ctx->stream, U.unitig.as<u32>(), U.cc.comp.as<u32>(), (const unsigned char*)nullptr, n, nu,
                           U.cc.stats.n_components, static_cast<u32*>(d_row_comp), (unsigned char*)nullptr, (unsigned char*)nullptr);
        CKL("k_cc_rows");
        ctx->mark("component rows");
    }
    return query_finish(ctx);
}

int dskgpu_components_table(dskgpu_ctx* ctx, void* d_first, void* d_unitigs, void* d_rows, void* d_ab_sum, void* d_edges) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!d_first && !d_unitigs && !d_rows && !d_ab_sum && !d_edges) return fail(ctx, DSKGPU_E_ARG, "dskgpu_components_table: no output pointer");
    if (const int rc = ensure_components(ctx, "dskgpu_components_table")) return rc;
    const Components& X = ctx->unitigs.cc;
    const u64 n_c = X.stats.n_components;
    if (n_c) {
        const u64* cols = X.cols.as<u64>();
        void* out[CC_COUNT] = {d_unitigs, d_rows, d_ab_sum, d_edges};
        if (d_first) CK(hipMemcpyAsync(d_first, X.first.p, n_c * 4, hipMemcpyDeviceToDevice, ctx->stream));
        for (int col = 0; col < CC_COUNT; ++col)
            if (out[col]) CK(hipMemcpyAsync(out[col], cols + col * n_c, n_c * 8, hipMemcpyDeviceToDevice, ctx->stream));
    }
    return query_finish(ctx);
}

int dskgpu_graph_small_components(dskgpu_ctx* ctx, const dskgpu_component_params* params, void* d_row_drop, void* d_comp_small, dskgpu_component_drop_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!d_row_drop && !d_comp_small && !stats) return fail(ctx, DSKGPU_E_ARG, "dskgpu_graph_small_components: no output pointer");
    if (const int rc = check_params(ctx, params, "dskgpu_graph_small_components")) return rc;
    if (const int rc = ensure_components(ctx, "dskgpu_graph_small_components")) return rc;
    dskgpu_component_drop_stats t{};
    if (ctx->n_rows == 0) {
        if (const int rc = query_finish(ctx)) return rc;
        if (stats) *stats = t;
        return DSKGPU_OK;
    }
    std::vector<u64> old_off, h;
    if (const int rc = begin_record(ctx, false, old_off)) return abandon(ctx, rc);
    if (const int rc = small_enqueue(ctx, *params, static_cast<unsigned char*>(d_row_drop), false)) return abandon(ctx, rc);
    if (d_comp_small) CK(hipMemcpyAsync(d_comp_small, ctx->filtered.bits.p, ctx->unitigs.cc.stats.n_components, hipMemcpyDeviceToDevice, ctx->stream));
    ctx->mark("small components");
    if (const int rc = read_record(ctx, h, 0)) return abandon(ctx, rc);
    if (const int rc = query_finish(ctx)) return rc;
    set_drop(t, h.data());
    t.n_rows_left = ctx->n_rows - t.n_rows_dropped;
    if (stats) *stats = t;
    return DSKGPU_OK;
}

int dskgpu_drop_components(dskgpu_ctx* ctx, const dskgpu_component_params* params, dskgpu_component_drop_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (const int rc = check_params(ctx, params, "dskgpu_drop_components")) return rc;
    dskgpu_component_drop_stats t{};
    std::vector<u64> old_off, h;
    int rc = ensure_components(ctx, "dskgpu_drop_components");
    if (rc == DSKGPU_OK && ctx->n_rows == 0) rc = query_finish(ctx);
    else if (rc == DSKGPU_OK) {
        const u64 n = ctx->n_rows;
        do {
            if ((rc = begin_record(ctx, true, old_off)) || (rc = small_enqueue(ctx, *params, nullptr, true))) { abandon(ctx, rc); break; }
            ctx->mark("small components");
            const unsigned char* keep = ctx->filtered.keep.as<unsigned char>();
            if ((rc = filter_scan(ctx, keep, old_off)) || (rc = read_record(ctx, h, old_off.size()))) { abandon(ctx, rc); break; }
            if (h[CR_SMALL] == 0) { rc = query_finish(ctx); break; }            // nothing is small: nothing is filtered, nothing invalidated
            if (h[CR_ROWS] + h.back() != n) { rc = abandon(ctx, fail(ctx, DSKGPU_E_DEVICE, "dskgpu_drop_components: the small components' rows and the kept rows do not add up (internal error)")); break; }
            if ((rc = filter_apply(ctx, keep, h.data() + REC_COUNTERS, old_off.size()))) { abandon(ctx, rc); break; }
            ctx->mark("filter rows");
            set_drop(t, h.data());
            if ((rc = query_finish(ctx))) break;
            if ((rc = ensure_components(ctx, "dskgpu_drop_components"))) break;   // of the final rows: the graph is ready when the call returns
            rc = query_finish(ctx);
        } while (false);
    }
    t.n_rows_left = ctx->n_rows;
    if (stats) *stats = t;
    return rc;
}

}  // extern "C"
