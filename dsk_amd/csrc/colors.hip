// colors.hip -- sample colours for rows, unitigs and variants: dskgpu_colors_begin / _colors_add / _colors_rows / _colors_unitigs, and the
// samples compared with each other: dskgpu_colors_pairs / _colors_load / _colors_marks (include/dskgpu.h).  Host side of colors.h; owns
// dskgpu_ctx::colors.  dskgpu_colors_add reads the lookup index (ensure_index builds it) and the result's rows and encodes the stream into
// scratch of its own, which goes when the call returns; dskgpu_colors_unitigs reads the compaction (ensure_compaction builds it); the pair
// matrices and the marks read the matrix alone.  What is kept is the matrix.  Nothing else of the context is touched.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "colors.h"

namespace {

constexpr u64 LAUNCH_BLOCKS = 1ull << 30;        // blocks of one launch; a longer stream takes several

struct Scratch {
    DevBuf packed, inval, stat;
    ~Scratch() { for (DevBuf* b : {&packed, &inval, &stat}) b->release(); }
};

template <int W>
void launch_reads(dskgpu_ctx* ctx, const Scratch& S, u64 nwords, u64 nbytes, const ColBanks& B) {
    constexpr int TPW = 32 / QBatch<W>::N;
    const Colors& K = ctx->colors;
    const u64 nblocks = (nwords * TPW + 255) / 256;
    for (u64 b0 = 0; b0 < nblocks; b0 += LAUNCH_BLOCKS) {
        const unsigned grid = (unsigned)std::min<u64>(LAUNCH_BLOCKS, nblocks - b0);
        hipLaunchKernelGGL(k_color_reads<W>, dim3(grid), dim3(256), 0, ctx->stream, (const u64*)S.packed.as<u64>(), (const u32*)S.inval.as<u32>(), nwords, nbytes, b0 * 256,
                           (int)ctx->cfg.kmer_size, query_table(ctx), B, K.n_rows, K.n_colors, K.C.as<u32>(), S.stat.as<u64>());
    }
}

int add_stream(dskgpu_ctx* ctx, const void* d_bytes, u64 nbytes, const ColBanks& B, dskgpu_color_stats* out) {
    Scratch S;
    const u64 nwords = (nbytes + 31) / 32;
    if (const int rc = query_ensure(ctx, S.packed, (nwords + 1) * 8, "encode buffer")) return rc;
    if (const int rc = query_ensure(ctx, S.inval, (nwords + 1) * 4, "encode buffer")) return rc;
    if (const int rc = query_ensure(ctx, S.stat, COL_ST_COUNT * 8, "colour counters")) return rc;
    CK(hipMemsetAsync(S.stat.p, 0, COL_ST_COUNT * 8, ctx->stream));
    if (const int rc = encode_into(ctx, static_cast<const uint8_t*>(d_bytes), nbytes, S.packed.as<u64>(), S.inval.as<u32>())) return rc;
    if (ctx->W == 1) launch_reads<1>(ctx, S, nwords, nbytes, B); else if (ctx->W == 2) launch_reads<2>(ctx, S, nwords, nbytes, B); else launch_reads<4>(ctx, S, nwords, nbytes, B);
    CKL("k_color_reads");
    ctx->mark("colors");
    u64 h[COL_ST_COUNT] = {0};
    CK(hipMemcpyAsync(h, S.stat.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));                                           // the scratch goes when this returns
    out->n_valid = h[COL_ST_VALID]; out->n_placed = h[COL_ST_PLACED];
    return DSKGPU_OK;
}

u64 pairs_grid(const dskgpu_ctx* ctx) { return ctx->tune.pairs_grid ? std::min<u64>(ctx->tune.pairs_grid, CP_GRID) : CP_GRID; }      // (never more than CP_GRID: the row counts of a thread are u32)

template <int NC>
void launch_pairs_reg(dskgpu_ctx* ctx, bool full, u32 min_count, const unsigned char* select, const ColPairOut& out) {
    const Colors& K = ctx->colors;
    const dim3 grid((unsigned)std::min<u64>((K.n_rows + CP_BLOCK - 1) / CP_BLOCK, pairs_grid(ctx)));
    if (full) hipLaunchKernelGGL((k_color_pairs_reg<NC, true>), grid, dim3(CP_BLOCK), 0, ctx->stream, (const u32*)K.C.as<u32>(), K.n_rows, min_count, select, out);
    else hipLaunchKernelGGL((k_color_pairs_reg<NC, false>), grid, dim3(CP_BLOCK), 0, ctx->stream, (const u32*)K.C.as<u32>(), K.n_rows, min_count, select, out);
}

// the pair kernel of the matrix's width: k_color_pairs_reg up to the switch point, k_color_pairs_tile above it
void launch_pairs(dskgpu_ctx* ctx, bool full, u32 min_count, const unsigned char* select, const ColPairOut& out) {
    const Colors& K = ctx->colors;
    const u32 reg_max = ctx->tune.pairs_reg_max == ~0u ? CP_REG_SWITCH : std::min<u32>(ctx->tune.pairs_reg_max, CP_REG_MAX);
    if (K.n_colors <= reg_max) {
        switch (K.n_colors) {
            case 1: launch_pairs_reg<1>(ctx, full, min_count, select, out); break;
            case 2: launch_pairs_reg<2>(ctx, full, min_count, select, out); break;
            case 3: launch_pairs_reg<3>(ctx, full, min_count, select, out); break;
            case 4: launch_pairs_reg<4>(ctx, full, min_count, select, out); break;
            case 5: launch_pairs_reg<5>(ctx, full, min_count, select, out); break;
            case 6: launch_pairs_reg<6>(ctx, full, min_count, select, out); break;
            case 7: launch_pairs_reg<7>(ctx, full, min_count, select, out); break;
            default: launch_pairs_reg<8>(ctx, full, min_count, select, out); break;
        }
        return;
    }
    const dim3 grid((unsigned)std::min<u64>((K.n_rows + CP_TILE_ROWS - 1) / CP_TILE_ROWS, pairs_grid(ctx)));
    const u32 no_skip = ctx->tune.pairs_no_skip ? 1u : 0u;
    if (full) hipLaunchKernelGGL(k_color_pairs_tile<true>, grid, dim3(CP_BLOCK), 0, ctx->stream, (const u32*)K.C.as<u32>(), K.n_rows, K.n_colors, min_count, select, no_skip, out);
    else hipLaunchKernelGGL(k_color_pairs_tile<false>, grid, dim3(CP_BLOCK), 0, ctx->stream, (const u32*)K.C.as<u32>(), K.n_rows, K.n_colors, min_count, select, no_skip, out);
}

}  // namespace

extern "C" {

int dskgpu_colors_begin(dskgpu_ctx* ctx, uint32_t n_colors) {
    if (!ctx) return DSKGPU_E_ARG;
    if (n_colors == 0 || n_colors > COL_MAX) return fail(ctx, DSKGPU_E_ARG, "dskgpu_colors_begin: n_colors must be in 1..64");
    if (!ctx->have_result) return fail(ctx, DSKGPU_E_STATE, "no result to colour: count first");
    CK(hipSetDevice(ctx->cfg.device));
    Colors& K = ctx->colors;
    K.valid = false;
    const u64 cells = ctx->n_rows * (u64)n_colors;
    if (const int rc = query_ensure(ctx, K.C, cells ? cells * 4 : 16, "colour matrix")) { K.release(); return rc; }
    CK(hipMemsetAsync(K.C.p, 0, cells ? cells * 4 : 16, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    K.n_colors = n_colors; K.n_rows = ctx->n_rows; K.valid = true;
    return DSKGPU_OK;
}

int dskgpu_colors_add(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, const uint64_t* end_offsets, uint32_t n_banks, uint32_t first_color,
                      dskgpu_color_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (nbytes && (!d_bytes || !end_offsets)) return fail(ctx, DSKGPU_E_ARG, "dskgpu_colors_add: null pointer");
    if (nbytes && n_banks == 0) return fail(ctx, DSKGPU_E_ARG, "dskgpu_colors_add: no bank for a stream of " + std::to_string(nbytes) + " bytes");
    if (n_banks > COL_MAX) return fail(ctx, DSKGPU_E_ARG, "dskgpu_colors_add: more than 64 banks");
    ColBanks B{};
    B.n = end_offsets ? n_banks : 0; B.first = first_color;
    for (u32 b = 0; b < B.n; ++b) {
        B.end[b] = end_offsets[b];
        if (B.end[b] > nbytes || (b && B.end[b] < B.end[b - 1])) return fail(ctx, DSKGPU_E_ARG, "dskgpu_colors_add: the bank ends must not decrease and must not pass nbytes");
    }
    const Colors& K = ctx->colors;
    if (!ctx->have_result) return fail(ctx, DSKGPU_E_STATE, "no result to colour: count first");
    if (!K.valid) return fail(ctx, DSKGPU_E_STATE, "dskgpu_colors_add: no matrix is kept: dskgpu_colors_begin first");
    if ((u64)first_color + n_banks > K.n_colors)
        return fail(ctx, DSKGPU_E_ARG, "dskgpu_colors_add: first_color + n_banks is " + std::to_string((u64)first_color + n_banks) + ", the matrix has " + std::to_string(K.n_colors) + " colours");
    dskgpu_color_stats out{};
    if (nbytes == 0) { if (stats) *stats = out; return DSKGPU_OK; }                  // (nothing is done: all-zero stats)
    out.n_rows = K.n_rows; out.n_colors = K.n_colors;
    CK(hipSetDevice(ctx->cfg.device));
    query_begin(ctx);
    const bool had_index = ctx->query.valid;
    if (const int rc = ensure_index(ctx)) return abandon(ctx, rc);
    if (!had_index) ctx->mark("query index");
    int rc = add_stream(ctx, d_bytes, nbytes, B, &out);
    if (rc == DSKGPU_OK) rc = query_finish(ctx); else rc = abandon(ctx, rc);
    if (rc != DSKGPU_OK) return rc;
    if (stats) *stats = out;
    return DSKGPU_OK;
}

int dskgpu_colors_rows(dskgpu_ctx* ctx, uint32_t min_count, void* d_counts, void* d_mask) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!d_counts && !d_mask) return fail(ctx, DSKGPU_E_ARG, "dskgpu_colors_rows: neither d_counts nor d_mask");
    if (min_count == 0) return fail(ctx, DSKGPU_E_ARG, "dskgpu_colors_rows: min_count must be at least 1");
    const Colors& K = ctx->colors;
    if (!K.valid) return fail(ctx, DSKGPU_E_STATE, "dskgpu_colors_rows: no matrix is kept: dskgpu_colors_begin first");
    CK(hipSetDevice(ctx->cfg.device));
    if (K.n_rows) {
        const bool vec = K.n_colors % 4 == 0 && (reinterpret_cast<uintptr_t>(d_counts) & 15) == 0;
        const dim3 grid(blocks(K.n_rows, 256));
        if (vec) hipLaunchKernelGGL(k_color_mask<true>, grid, dim3(256), 0, ctx->stream, (const u32*)K.C.as<u32>(), K.n_rows, K.n_colors, min_count, static_cast<u32*>(d_counts), static_cast<u64*>(d_mask));
        else hipLaunchKernelGGL(k_color_mask<false>, grid, dim3(256), 0, ctx->stream, (const u32*)K.C.as<u32>(), K.n_rows, K.n_colors, min_count, static_cast<u32*>(d_counts), static_cast<u64*>(d_mask));
        CKL("k_color_mask");
    }
    CK(hipStreamSynchronize(ctx->stream));
    return DSKGPU_OK;
}

int dskgpu_colors_unitigs(dskgpu_ctx* ctx, uint32_t min_count, void* d_sum, void* d_all, void* d_any) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!d_sum && !d_all && !d_any) return fail(ctx, DSKGPU_E_ARG, "dskgpu_colors_unitigs: no output pointer");
    if (min_count == 0) return fail(ctx, DSKGPU_E_ARG, "dskgpu_colors_unitigs: min_count must be at least 1");
    if (!ctx->colors.valid) return fail(ctx, DSKGPU_E_STATE, "dskgpu_colors_unitigs: no matrix is kept: dskgpu_colors_begin first");
    if (const int rc = ensure_compaction(ctx, "dskgpu_colors_unitigs")) return rc;
    const Colors& K = ctx->colors;
    const Unitigs& U = ctx->unitigs;
    const u64 nu = U.stats.n_unitigs, n = K.n_rows;
    u64 *sum = static_cast<u64*>(d_sum), *all = static_cast<u64*>(d_all), *any = static_cast<u64*>(d_any);
    int rc = DSKGPU_OK;
    auto enqueue = [&]() -> int {
        if (nu == 0 || n == 0) return DSKGPU_OK;
        if (sum) CK(hipMemsetAsync(sum, 0, nu * K.n_colors * 8, ctx->stream));
        if (any) CK(hipMemsetAsync(any, 0, nu * 8, ctx->stream));
        if (all) {
            hipLaunchKernelGGL(k_color_fill64, dim3(blocks(nu, 256)), dim3(256), 0, ctx->stream, all, nu, K.n_colors == 64 ? ~0ull : (1ull << K.n_colors) - 1ull);
            CKL("k_color_fill64");
        }
        hipLaunchKernelGGL(k_color_unitigs, dim3(blocks(n, 256)), dim3(256), 0, ctx->stream, (const u32*)K.C.as<u32>(), (const u32*)U.unitig.as<u32>(), n, nu, K.n_colors, min_count,
                           sum, all, any);
        CKL("k_color_unitigs");
        return DSKGPU_OK;
    };
    rc = enqueue();
    if (rc != DSKGPU_OK) return abandon(ctx, rc);
    ctx->mark("color unitigs");
    return query_finish(ctx);
}

int dskgpu_colors_pairs(dskgpu_ctx* ctx, uint32_t min_count, const void* d_select, void* d_shared, void* d_cross, void* d_min_sum, dskgpu_color_pair_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!d_shared && !d_cross && !d_min_sum) return fail(ctx, DSKGPU_E_ARG, "dskgpu_colors_pairs: no output pointer");
    if (min_count == 0) return fail(ctx, DSKGPU_E_ARG, "dskgpu_colors_pairs: min_count must be at least 1");
    const Colors& K = ctx->colors;
    if (!K.valid) return fail(ctx, DSKGPU_E_STATE, "dskgpu_colors_pairs: no matrix is kept: dskgpu_colors_begin or dskgpu_colors_load first");
    CK(hipSetDevice(ctx->cfg.device));
    dskgpu_color_pair_stats out{};
    const size_t bytes = (size_t)K.n_colors * K.n_colors * 8;
    Scratch S;
    query_begin(ctx);
    auto enqueue = [&]() -> int {
        for (void* p : {d_shared, d_cross, d_min_sum}) if (p) CK(hipMemsetAsync(p, 0, bytes, ctx->stream));
        if (K.n_rows == 0) return DSKGPU_OK;
        if (const int rc = query_ensure(ctx, S.stat, CP_ST_COUNT * 8, "colour counters")) return rc;
        CK(hipMemsetAsync(S.stat.p, 0, CP_ST_COUNT * 8, ctx->stream));
        const ColPairOut o{static_cast<u64*>(d_shared), static_cast<u64*>(d_cross), static_cast<u64*>(d_min_sum), S.stat.as<u64>()};
        launch_pairs(ctx, d_cross || d_min_sum, min_count, static_cast<const unsigned char*>(d_select), o);
        CKL("k_color_pairs");
        ctx->mark("color pairs");
        u64 h[CP_ST_COUNT] = {0};
        CK(hipMemcpyAsync(h, S.stat.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));                                       // the scratch goes when this returns
        out.n_rows = K.n_rows; out.n_colors = K.n_colors; out.n_selected = h[CP_ST_SELECTED]; out.n_present = h[CP_ST_PRESENT];
        return DSKGPU_OK;
    };
    if (const int rc = enqueue()) return abandon(ctx, rc);
    if (const int rc = query_finish(ctx)) return rc;
    if (stats) *stats = out;
    return DSKGPU_OK;
}

int dskgpu_colors_load(dskgpu_ctx* ctx, const void* d_counts, uint32_t n_colors) {
    if (!ctx) return DSKGPU_E_ARG;
    if (n_colors == 0 || n_colors > COL_MAX) return fail(ctx, DSKGPU_E_ARG, "dskgpu_colors_load: n_colors must be in 1..64");
    if (!ctx->have_result) return fail(ctx, DSKGPU_E_STATE, "no result to colour: count first");
    if (ctx->n_rows && !d_counts) return fail(ctx, DSKGPU_E_ARG, "dskgpu_colors_load: null d_counts");
    CK(hipSetDevice(ctx->cfg.device));
    Colors& K = ctx->colors;
    K.valid = false;
    const u64 cells = ctx->n_rows * (u64)n_colors;
    if (const int rc = query_ensure(ctx, K.C, cells ? cells * 4 : 16, "colour matrix")) { K.release(); return rc; }
    query_begin(ctx);
    auto enqueue = [&]() -> int {
        if (cells) CK(hipMemcpyAsync(K.C.p, d_counts, cells * 4, hipMemcpyDeviceToDevice, ctx->stream));
        else CK(hipMemsetAsync(K.C.p, 0, 16, ctx->stream));
        return DSKGPU_OK;
    };
    if (const int rc = enqueue()) { K.release(); return abandon(ctx, rc); }
    ctx->mark("color load");
    if (const int rc = query_finish(ctx)) { K.release(); return rc; }
    K.n_colors = n_colors; K.n_rows = ctx->n_rows; K.valid = true;
    return DSKGPU_OK;
}

int dskgpu_colors_marks(dskgpu_ctx* ctx, const dskgpu_color_rule* rule, void* d_keep, dskgpu_color_mark_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!rule) return fail(ctx, DSKGPU_E_ARG, "dskgpu_colors_marks: null rule");
    if (rule->flags & ~DSKGPU_COLORS_INVERT) return fail(ctx, DSKGPU_E_ARG, "dskgpu_colors_marks: unknown flag bits");
    if (rule->min_count == 0) return fail(ctx, DSKGPU_E_ARG, "dskgpu_colors_marks: min_count must be at least 1");
    const Colors& K = ctx->colors;
    if (!K.valid) return fail(ctx, DSKGPU_E_STATE, "dskgpu_colors_marks: no matrix is kept: dskgpu_colors_begin or dskgpu_colors_load first");
    if (K.n_colors < 64 && ((rule->need_all | rule->need_none) >> K.n_colors))
        return fail(ctx, DSKGPU_E_ARG, "dskgpu_colors_marks: need_all or need_none names a colour at or above n_colors = " + std::to_string(K.n_colors));
    if (K.n_rows && !d_keep) return fail(ctx, DSKGPU_E_ARG, "dskgpu_colors_marks: null d_keep");
    CK(hipSetDevice(ctx->cfg.device));
    dskgpu_color_mark_stats out{};
    if (K.n_rows) {
        Scratch S;
        query_begin(ctx);
        auto enqueue = [&]() -> int {
            if (const int rc = query_ensure(ctx, S.stat, COL_ST_COUNT * 8, "colour counters")) return rc;
            CK(hipMemsetAsync(S.stat.p, 0, COL_ST_COUNT * 8, ctx->stream));
            const ColRule R{rule->need_all, rule->need_none, rule->min_count, rule->min_present, rule->max_present, rule->flags & DSKGPU_COLORS_INVERT};
            hipLaunchKernelGGL(k_color_marks, dim3(blocks(K.n_rows, 256)), dim3(256), 0, ctx->stream, (const u32*)K.C.as<u32>(), K.n_rows, K.n_colors, R, static_cast<unsigned char*>(d_keep),
                               S.stat.as<u64>());
            CKL("k_color_marks");
            ctx->mark("color marks");
            u64 h[COL_ST_COUNT] = {0};
            CK(hipMemcpyAsync(h, S.stat.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
            CK(hipStreamSynchronize(ctx->stream));                                   // the scratch goes when this returns
            out.n_rows = K.n_rows; out.n_kept = h[0];
            return DSKGPU_OK;
        };
        if (const int rc = enqueue()) return abandon(ctx, rc);
        if (const int rc = query_finish(ctx)) return rc;
    }
    if (stats) *stats = out;
    return DSKGPU_OK;
}

}  // extern "C"
