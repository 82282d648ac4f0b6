// correct.hip -- substitution errors in reads corrected against the last result: dskgpu_correct_reads (include/dskgpu.h).  Host side of
// correct.h.  Reads the lookup index (ensure_index builds it) and the result's rows; nothing else of the context, and it keeps nothing:
// the stream is encoded into scratch of its own, which goes -- with the state bytes, the block sums and the candidate list -- when the
// call returns.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include "engine.h"
#include "correct.h"

namespace {

struct Scratch {
    DevBuf packed, inval, state, bsum, bbase, tmp, gaps, alive, stat;
    ~Scratch() { for (DevBuf* b : {&packed, &inval, &state, &bsum, &bbase, &tmp, &gaps, &alive, &stat}) b->release(); }
};

template <int W>
void launch_state(dskgpu_ctx* ctx, const Scratch& S, u64 nwords, u64 nbytes, u32 tmin) {
    constexpr int TPW = 32 / QBatch<W>::N;
    const unsigned grid = (unsigned)((nwords * TPW + 255) / 256);
    hipLaunchKernelGGL(k_correct_state<W>, dim3(grid), dim3(256), 0, ctx->stream, S.packed.as<u64>(), S.inval.as<u32>(), nwords, nbytes, (int)ctx->cfg.kmer_size,
                       query_table(ctx), tmin, S.state.as<unsigned char>(), S.stat.as<u64>());
}

template <int W>
void launch_trials(dskgpu_ctx* ctx, const Scratch& S, const CTrial& P) {
    u64* stat = S.stat.as<u64>();
    if (!ctx->tune.correct_staged) {                                                 // the default: it measured faster (profiles/read_correction.md)
        hipLaunchKernelGGL(k_correct_plain<W>, dim3((unsigned)((P.n_cand + 255) / 256)), dim3(256), 0, ctx->stream, P, stat);
        return;
    }
    const u64 per_block = 256ull * CBatch<W>::CAND;
    hipLaunchKernelGGL(k_correct_first<W>, dim3((unsigned)((P.n_cand + per_block - 1) / per_block)), dim3(256), 0, ctx->stream, P, S.alive.as<unsigned char>(), stat);
    const unsigned grid = (unsigned)std::min<u64>((P.n_cand + 3) / 4, (u64)ctx->num_cu * 16);
    hipLaunchKernelGGL(k_correct_rest<W>, dim3(grid), dim3(256), 0, ctx->stream, P, S.alive.as<unsigned char>(), stat);
}

int correct(dskgpu_ctx* ctx, const void* d_bytes, u64 nbytes, u32 tmin, void* d_out, void* d_state, u64 (&h_stat)[CS_COUNT]) {
    Scratch S;
    const int k = (int)ctx->cfg.kmer_size;
    const u64 nwords = (nbytes + 31) / 32;
    if (const int rc = query_ensure(ctx, S.packed, (nwords + 1) * 8, "encode buffer")) return rc;
    if (const int rc = query_ensure(ctx, S.inval, (nwords + 1) * 4, "encode buffer")) return rc;
    if (const int rc = query_ensure(ctx, S.state, nwords * 32, "correction states")) return rc;
    if (const int rc = query_ensure(ctx, S.stat, CS_COUNT * 8, "correction counters")) return rc;
    CK(hipMemsetAsync(S.stat.p, 0, CS_COUNT * 8, ctx->stream));
    if (const int rc = encode_into(ctx, static_cast<const uint8_t*>(d_bytes), nbytes, S.packed.as<u64>(), S.inval.as<u32>())) return rc;
    if (ctx->W == 1) launch_state<1>(ctx, S, nwords, nbytes, tmin); else if (ctx->W == 2) launch_state<2>(ctx, S, nwords, nbytes, tmin); else launch_state<4>(ctx, S, nwords, nbytes, tmin);
    CKL("k_correct_state");
    if (d_state) CK(hipMemcpyAsync(d_state, S.state.p, nbytes, hipMemcpyDeviceToDevice, ctx->stream));
    ctx->mark("correct states");

    // the shaped gaps: count per block, scan, one read-back of the total, emit
    const u64 nblocks = (nbytes + C_BLOCK - 1) / C_BLOCK;
    if (const int rc = query_ensure(ctx, S.bsum, (nblocks + 1) * 8, "gap block sums")) return rc;
    if (const int rc = query_ensure(ctx, S.bbase, (nblocks + 1) * 8, "gap block sums")) return rc;
    const unsigned char* state = S.state.as<unsigned char>();
    u64 *bsum = S.bsum.as<u64>(), *bbase = S.bbase.as<u64>(), *stat = S.stat.as<u64>();
    CK(hipMemsetAsync(bsum + nblocks, 0, 8, ctx->stream));                           // the scan's last input: bbase[nblocks] = the total
    hipLaunchKernelGGL(k_correct_gaps<false>, dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, state, nbytes, k, bsum, (const u64*)nullptr, (CGap*)nullptr, 0ull, stat);
    CKL("k_correct_gaps");
    size_t tmp_bytes = 0;
    CK(rocprim::exclusive_scan(nullptr, tmp_bytes, bsum, bbase, 0ull, (size_t)(nblocks + 1), rocprim::plus<u64>(), ctx->stream));      // LIBRARY SCAN (rocprim): plumbing, 8 bytes per 4096 positions
    if (const int rc = query_ensure(ctx, S.tmp, tmp_bytes ? tmp_bytes : 8, "gap scan")) return rc;
    CK(rocprim::exclusive_scan(S.tmp.p, tmp_bytes, bsum, bbase, 0ull, (size_t)(nblocks + 1), rocprim::plus<u64>(), ctx->stream));
    u64 n_cand = 0;
    CK(hipMemcpyAsync(&n_cand, bbase + nblocks, 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    if (n_cand > nbytes) return fail(ctx, DSKGPU_E_DEVICE, "dskgpu_correct_reads: more candidates than bytes (internal error)");
    if (n_cand) {
        if (const int rc = query_ensure(ctx, S.gaps, n_cand * sizeof(CGap), "candidate list")) return rc;
        if (ctx->tune.correct_staged)
            if (const int rc = query_ensure(ctx, S.alive, n_cand, "candidate list")) return rc;
        hipLaunchKernelGGL(k_correct_gaps<true>, dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, state, nbytes, k, (u64*)nullptr, (const u64*)bbase, S.gaps.as<CGap>(), n_cand, stat);
        CKL("k_correct_gaps");
    }
    ctx->mark("correct gaps");

    // the copy of the input is ordered before the kernels that write the corrected bytes; in place there is nothing to copy
    if (d_out && d_out != d_bytes) CK(hipMemcpyAsync(d_out, d_bytes, nbytes, hipMemcpyDeviceToDevice, ctx->stream));
    if (n_cand) {
        const CTrial P{S.packed.as<u64>(), query_table(ctx), k, tmin, static_cast<const unsigned char*>(d_bytes), static_cast<unsigned char*>(d_out), S.gaps.as<CGap>(), n_cand};
        if (ctx->W == 1) launch_trials<1>(ctx, S, P); else if (ctx->W == 2) launch_trials<2>(ctx, S, P); else launch_trials<4>(ctx, S, P);
        CKL("k_correct_try");
    }
    ctx->mark("correct trials");
    CK(hipMemcpyAsync(h_stat, stat, sizeof(h_stat), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));                                           // the scratch goes when this returns
    return DSKGPU_OK;
}

}  // namespace

extern "C" {

int dskgpu_correct_reads(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, const dskgpu_correct_params* params, void* d_out, void* d_state,
                         dskgpu_correct_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (nbytes && !d_bytes) return fail(ctx, DSKGPU_E_ARG, "dskgpu_correct_reads: null pointer");
    if (params && (params->flags || params->reserved[0] || params->reserved[1] || params->reserved[2]))
        return fail(ctx, DSKGPU_E_ARG, "dskgpu_correct_reads: flags and reserved words must be 0");
    if (nbytes > (0x7FFFFFFFull << 11)) return fail(ctx, DSKGPU_E_ARG, "dskgpu_correct_reads: a longer stream than one launch takes; split the call");
    if (ctx->cfg.world_size > 1)
        return fail(ctx, DSKGPU_E_STATE, "dskgpu_correct_reads: a rank holds only the k-mers it owns; its rows are not the trusted set (world_size > 1)");
    if (!ctx->have_result) return fail(ctx, DSKGPU_E_STATE, "no result to correct reads against: count first");
    dskgpu_correct_stats out{};
    if (nbytes == 0) { if (stats) *stats = out; return DSKGPU_OK; }
    CK(hipSetDevice(ctx->cfg.device));
    query_begin(ctx);
    if (const int rc = ensure_index(ctx)) return abandon(ctx, rc);
    ctx->mark("query index");
    const u32 tmin = params && params->trust_min > 1 ? params->trust_min : 1u;       // (0 and 1: any row)
    u64 h[CS_COUNT] = {0};
    if (const int rc = correct(ctx, d_bytes, nbytes, tmin, d_out, d_state, h)) return abandon(ctx, rc);
    if (const int rc = query_finish(ctx)) return rc;
    out.n_valid = h[CS_VALID]; out.n_trusted = h[CS_TRUSTED]; out.n_gaps = h[CS_GAPS]; out.n_interior = h[CS_INTERIOR]; out.n_head = h[CS_HEAD];
    out.n_tail = h[CS_TAIL]; out.n_skipped = h[CS_SKIPPED]; out.n_corrected = h[CS_CORRECTED]; out.n_ambiguous = h[CS_AMBIGUOUS]; out.n_unfixable = h[CS_UNFIXABLE];
    if (stats) *stats = out;
    return DSKGPU_OK;
}

}  // extern "C"
