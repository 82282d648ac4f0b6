// variants.hip -- the bubbles of the compacted de Bruijn graph reported as variants: dskgpu_variants / _variants_table / _variants_stream
// (include/dskgpu.h).  Host side of variants.h; owns dskgpu_ctx::variants.  Reads the tables of unitigs.hip (ensure_edges builds them), the
// result's rows and, as scratch, the candidate tables of the bubble rule (Filtered::ends / ::len, written by k_bubble_candidates); nothing
// else of the context.  Two small read-backs: the number of variants, then the letters, the stream bytes and the counters.  What is kept is
// the records, the line offsets and the variant stream; the flags, the scans and the letters of the flagged unitigs go when the call returns.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include "engine.h"
#include "variants.h"

namespace {

// the scratch of dskgpu_variants: freed when build() returns, whatever way
// (per_unitig: one allocation for what is sized by the unitigs -- [cnt | base | tlen | toff: n_unitigs + 1 words each | stat | flag])
struct Scratch {
    DevBuf per_unitig, vlen, letters, tmp;
    ~Scratch() { for (DevBuf* b : {&per_unitig, &vlen, &letters, &tmp}) b->release(); }
};

int scan64(dskgpu_ctx* ctx, DevBuf& tmp, u64* in, u64* out, u64 n) {
    size_t tmp_bytes = 0;
    CK(rocprim::exclusive_scan(nullptr, tmp_bytes, in, out, 0ull, (size_t)n, rocprim::plus<u64>(), ctx->stream));      // LIBRARY SCAN (rocprim): plumbing, 8 bytes per unitig / per line
    if (const int rc = query_ensure(ctx, tmp, tmp_bytes ? tmp_bytes : 8, "variant scan")) return rc;
    CK(rocprim::exclusive_scan(tmp.p, tmp_bytes, in, out, 0ull, (size_t)n, rocprim::plus<u64>(), ctx->stream));
    return DSKGPU_OK;
}

template <int W>
void launch_letters(dskgpu_ctx* ctx, const unsigned char* flag, const u64* toff, u64 n_letters, unsigned char* letters) {
    const Unitigs& U = ctx->unitigs;
    RowsIn rows;
    for (int x = 0; x < 4; ++x) rows.w[x] = ctx->res_w[x];
    hipLaunchKernelGGL(k_variant_letters<W>, dim3(blocks(ctx->n_rows, 256)), dim3(256), 0, ctx->stream, rows, ctx->n_rows, (int)ctx->cfg.kmer_size, U.unitig.as<u32>(),
                       U.pos.as<u32>(), flag, toff, U.stats.n_unitigs, n_letters, letters);
}

// no variant: the stats are all zero and the one offset is 0
int keep_none(dskgpu_ctx* ctx) {
    Variants& V = ctx->variants;
    if (const int rc = query_ensure(ctx, V.off, 8, "variant offsets")) return rc;
    CK(hipMemsetAsync(V.off.p, 0, 8, ctx->stream));
    return DSKGPU_OK;
}

// the variants of the current result, whose edges are there, into ctx->variants.  n_rows > 0
int build(dskgpu_ctx* ctx, const dskgpu_variant_params& p) {
    Variants& V = ctx->variants;
    Filtered& F = ctx->filtered;
    const Unitigs& U = ctx->unitigs;
    const u64 nu = U.stats.n_unitigs, ne = U.e_stats.n_edges;
    const int k = (int)ctx->cfg.kmer_size;
    Scratch S;
    if (const int rc = bubble_candidates(ctx, p.max_nodes)) return rc;
    if (const int rc = query_ensure(ctx, S.per_unitig, (4 * (nu + 1) + VS_COUNT) * 8 + nu, "variant scratch")) return rc;
    u64 *cnt = S.per_unitig.as<u64>(), *base = cnt + (nu + 1), *tlen = base + (nu + 1), *toff = tlen + (nu + 1), *stat = toff + (nu + 1);
    unsigned char* flag = reinterpret_cast<unsigned char*>(stat + VS_COUNT);
    CK(hipMemsetAsync(stat, 0, VS_COUNT * 8 + nu, ctx->stream));                     // the counters and, behind them, the flags
    CK(hipMemsetAsync(cnt + nu, 0, 8, ctx->stream));                                 // the scan's last input: base[nu] = n_variants
    const dim3 ugrid(blocks(nu, 256));
    const u64 *ends = F.ends.as<u64>(), *e_off = U.e_offsets.as<u64>();
    const u32 *len = F.len.as<u32>(), *e_tgt = U.e_targets.as<u32>();
    hipLaunchKernelGGL(k_variant_pairs<false>, ugrid, dim3(256), 0, ctx->stream, ends, len, e_off, e_tgt, nu, ne, p.max_diff, k, cnt, (const u64*)nullptr, 0ull,
                       (uint4*)nullptr, (u64*)nullptr, (unsigned char*)nullptr);
    CKL("k_variant_pairs");
    if (const int rc = scan64(ctx, S.tmp, cnt, base, nu + 1)) return rc;
    u64 nv = 0;
    CK(hipMemcpyAsync(&nv, base + nu, 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    if (nv > 4 * nu) return fail(ctx, DSKGPU_E_DEVICE, "dskgpu_variants: more variants than four per unitig (internal error)");
    if (nv == 0) return keep_none(ctx);

    if (const int rc = query_ensure(ctx, V.rec, nv * 32, "variant records")) return rc;
    if (const int rc = query_ensure(ctx, V.off, (2 * nv + 1) * 8, "variant offsets")) return rc;
    if (const int rc = query_ensure(ctx, S.vlen, (2 * nv + 1) * 8, "variant line lengths")) return rc;
    CK(hipMemsetAsync(S.vlen.as<u64>() + 2 * nv, 0, 8, ctx->stream));                // the scan's last input: off[2 nv] = stream_bytes
    uint4* rec = V.rec.as<uint4>();
    hipLaunchKernelGGL(k_variant_pairs<true>, ugrid, dim3(256), 0, ctx->stream, ends, len, e_off, e_tgt, nu, ne, p.max_diff, k, (u64*)nullptr, base, nv, rec,
                       S.vlen.as<u64>(), flag);
    CKL("k_variant_pairs");
    hipLaunchKernelGGL(k_variant_tlen, dim3(blocks(nu + 1, 256)), dim3(256), 0, ctx->stream, flag, len, nu, k, tlen, stat);
    CKL("k_variant_tlen");
    if (const int rc = scan64(ctx, S.tmp, tlen, toff, nu + 1)) return rc;
    if (const int rc = scan64(ctx, S.tmp, S.vlen.as<u64>(), V.off.as<u64>(), 2 * nv + 1)) return rc;
    u64 n_letters = 0, stream_bytes = 0;
    CK(hipMemcpyAsync(&n_letters, toff + nu, 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(&stream_bytes, V.off.as<u64>() + 2 * nv, 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    const u64 max_letters = (u64)k + p.max_nodes - 1;
    if (n_letters == 0 || n_letters > 2 * nv * max_letters || stream_bytes < 4 * nv || stream_bytes > 2 * nv * (max_letters + 1))
        return fail(ctx, DSKGPU_E_DEVICE, "dskgpu_variants: the texts of the variants do not add up (internal error)");

    if (const int rc = query_ensure(ctx, S.letters, n_letters, "variant letters")) return rc;
    if (const int rc = query_ensure(ctx, V.stream, stream_bytes, "variant stream")) return rc;
    unsigned char* letters = S.letters.as<unsigned char>();
    if (ctx->W == 1) launch_letters<1>(ctx, flag, toff, n_letters, letters);
    else if (ctx->W == 2) launch_letters<2>(ctx, flag, toff, n_letters, letters);
    else launch_letters<4>(ctx, flag, toff, n_letters, letters);
    CKL("k_variant_letters");
    const unsigned cgrid = (unsigned)std::min<u64>(blocks(nv, 4), (u64)ctx->num_cu * 8);      // (few blocks: each ends with two atomics on the same words)
    const u32 per_wave = (u32)((nv + 4ull * cgrid - 1) / (4ull * cgrid));
    hipLaunchKernelGGL(k_variant_compare, dim3(cgrid), dim3(256), 0, ctx->stream, rec, toff, letters, V.off.as<u64>(), nv, per_wave, nu, n_letters, stream_bytes,
                       (u32)max_letters, V.stream.as<unsigned char>(), stat);
    CKL("k_variant_compare");
    ctx->mark("variants");
    u64 h[VS_COUNT] = {0};
    CK(hipMemcpyAsync(h, stat, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));                                          // the scratch goes when this returns
    if (h[VS_BAD] || h[VS_SNP] + h[VS_MULTI] + h[VS_INDEL] + h[VS_COMPLEX] != nv)
        return fail(ctx, DSKGPU_E_DEVICE, "dskgpu_variants: a variant names no flagged unitig, or its two texts are equal (internal error)");
    V.stats.n_variants = nv; V.stats.n_snps = h[VS_SNP]; V.stats.n_multi = h[VS_MULTI]; V.stats.n_indels = h[VS_INDEL]; V.stats.n_complex = h[VS_COMPLEX];
    V.stats.n_unitigs = h[VS_UNITIGS]; V.stats.stream_bytes = stream_bytes; V.stats.max_letters = h[VS_MAXLEN];
    return DSKGPU_OK;
}

}  // namespace

extern "C" {

int dskgpu_variants(dskgpu_ctx* ctx, const dskgpu_variant_params* params, dskgpu_variant_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!params) return fail(ctx, DSKGPU_E_ARG, "dskgpu_variants: null params");
    if (params->max_nodes == 0 || params->max_nodes > R_MAX_NODES) return fail(ctx, DSKGPU_E_ARG, "dskgpu_variants: max_nodes must be in 1..65535");
    if (const int rc = ensure_edges(ctx, "dskgpu_variants")) return rc;
    Variants& V = ctx->variants;
    V.release();
    int rc = ctx->n_rows == 0 ? keep_none(ctx) : build(ctx, *params);
    if (rc == DSKGPU_OK && V.stats.n_variants == 0) ctx->mark("variants");      // (build() marks where the kernels end)
    if (rc == DSKGPU_OK) rc = query_finish(ctx); else rc = abandon(ctx, rc);
    if (rc != DSKGPU_OK) { V.release(); return rc; }
    V.valid = true;
    if (stats) *stats = V.stats;
    return DSKGPU_OK;
}

int dskgpu_variants_table(dskgpu_ctx* ctx, void* d_records) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!d_records) return fail(ctx, DSKGPU_E_ARG, "dskgpu_variants_table: null pointer");
    const Variants& V = ctx->variants;
    if (!V.valid) return fail(ctx, DSKGPU_E_STATE, "dskgpu_variants_table: no variants are kept: dskgpu_variants first");
    CK(hipSetDevice(ctx->cfg.device));
    if (V.stats.n_variants) CK(hipMemcpyAsync(d_records, V.rec.p, V.stats.n_variants * 32, hipMemcpyDeviceToDevice, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return DSKGPU_OK;
}

int dskgpu_variants_stream(dskgpu_ctx* ctx, void* d_offsets, void* d_bytes, uint64_t capacity) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!d_offsets && !d_bytes) return fail(ctx, DSKGPU_E_ARG, "dskgpu_variants_stream: neither d_offsets nor d_bytes");
    const Variants& V = ctx->variants;
    if (!V.valid) return fail(ctx, DSKGPU_E_STATE, "dskgpu_variants_stream: no variants are kept: dskgpu_variants first");
    if (d_bytes && capacity < V.stats.stream_bytes)
        return fail(ctx, DSKGPU_E_ARG, "dskgpu_variants_stream: capacity " + std::to_string(capacity) + " < stream_bytes " + std::to_string(V.stats.stream_bytes));
    CK(hipSetDevice(ctx->cfg.device));
    if (d_offsets) CK(hipMemcpyAsync(d_offsets, V.off.p, (2 * V.stats.n_variants + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (d_bytes && V.stats.stream_bytes) CK(hipMemcpyAsync(d_bytes, V.stream.p, V.stats.stream_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return DSKGPU_OK;
}

}  // extern "C"
