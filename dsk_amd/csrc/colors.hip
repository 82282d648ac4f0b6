// colors.hip -- sample colours for rows, unitigs and variants: dskgpu_colors_begin / _colors_add / _colors_rows / _colors_unitigs
// (include/dskgpu.h).  Host side of colors.h; owns dskgpu_ctx::colors.  dskgpu_colors_add reads the lookup index (ensure_index builds it)
// and the result's rows and encodes the stream into scratch of its own, which goes when the call returns; dskgpu_colors_unitigs reads the
// compaction (ensure_compaction builds it).  What is kept is the matrix.  Nothing else of the context is touched.
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

}  // extern "C"
