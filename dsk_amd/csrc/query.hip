// query.hip -- lookups in the last result: dskgpu_query_prepare / _kmers / _reads (include/dskgpu.h).  Host side of query.h; owns
// dskgpu_ctx::query.  Reads the result (res_w / res_ab / n_rows) and nothing else of the context: the queried stream is encoded into
// the query's own two buffers, never into ctx->packed / ctx->inval, so the reads of the context and their kept 2-bit form stay as
// they are.  The count path drops the index wherever it drops the result (dskgpu_ctx::drop_result).  graph.hip probes the same index:
// ensure_index, query_table and the begin / finish pair are declared in engine.h.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "query.h"

// allocation of a query buffer: out of memory is an answer (DSKGPU_E_NOMEM), not a broken context -- the error is taken off the
// runtime's "last error" so that the next launch check does not report it again
int query_ensure(dskgpu_ctx* ctx, DevBuf& b, size_t bytes, const char* what) {
    const hipError_t e = b.ensure(bytes);
    if (e == hipSuccess) return DSKGPU_OK;
    (void)hipGetLastError();
    ctx->err = std::string("query ") + what + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? DSKGPU_E_NOMEM : DSKGPU_E_DEVICE;
}

QTable query_table(const dskgpu_ctx* ctx) {
    QTable T;
    T.slots = ctx->query.table.as<u64>(); T.mask = ctx->query.cap - 1;
    for (int x = 0; x < 4; ++x) T.rows.w[x] = ctx->res_w[x];
    T.ab = ctx->res_ab;
    return T;
}

// the index of the current result: there already, or built now (enqueued on the context's stream; the kernel boundary orders it
// before the lookups that follow on the same stream)
int ensure_index(dskgpu_ctx* ctx) {
    if (!ctx->have_result) return fail(ctx, DSKGPU_E_STATE, "no result to query: count first");
    Query& q = ctx->query;
    if (q.valid) return DSKGPU_OK;
    const u64 n = ctx->n_rows;
    if (n > Q_MAX_ROWS) return fail(ctx, DSKGPU_E_STATE, "the result has more than 2^32 - 2 rows: the lookup index holds 32-bit row numbers");
    u64 cap = Q_MIN_CAP;
    while (cap < 2 * n) cap <<= 1;
    if (const int rc = query_ensure(ctx, q.table, cap * 8, "index")) return rc;
    q.cap = cap;
    CK(hipMemsetAsync(q.table.p, 0xFF, cap * 8, ctx->stream));
    if (n) {
        RowsIn rows;
        for (int x = 0; x < 4; ++x) rows.w[x] = ctx->res_w[x];
        const unsigned grid = (unsigned)std::min<u64>((n + 255) / 256, (u64)ctx->num_cu * 32);
        if (ctx->W == 1) hipLaunchKernelGGL(k_query_build<1>, dim3(grid), dim3(256), 0, ctx->stream, rows, n, q.table.as<u64>(), cap - 1);
        else if (ctx->W == 2) hipLaunchKernelGGL(k_query_build<2>, dim3(grid), dim3(256), 0, ctx->stream, rows, n, q.table.as<u64>(), cap - 1);
        else hipLaunchKernelGGL(k_query_build<4>, dim3(grid), dim3(256), 0, ctx->stream, rows, n, q.table.as<u64>(), cap - 1);
        CKL("k_query_build");
    }
    q.valid = true;
    return DSKGPU_OK;
}

void query_begin(dskgpu_ctx* ctx) { ctx->marks.clear(); ctx->ev_used = 0; ctx->mark("query start"); }

// wait for the stream; a failure leaves no half-built index behind
int query_finish(dskgpu_ctx* ctx) {
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->query.valid = false; ctx->marks.clear(); ctx->ev_used = 0; ctx->err = std::string("query: ") + hipGetErrorString(e); return DSKGPU_E_DEVICE; }
    ctx->resolve_marks();
    return DSKGPU_OK;
}

namespace {

template <int W>
void launch_reads(dskgpu_ctx* ctx, u64 nwords, u64 nbytes, u32* out) {
    constexpr int TPW = 32 / QBatch<W>::N;
    const unsigned grid = (unsigned)((nwords * TPW + 255) / 256);
    const Query& q = ctx->query;
    if ((reinterpret_cast<uintptr_t>(out) & 15) == 0)
        hipLaunchKernelGGL((k_query_reads<W, true>), dim3(grid), dim3(256), 0, ctx->stream, q.packed.as<u64>(), q.inval.as<u32>(), nwords, nbytes,
                           (int)ctx->cfg.kmer_size, query_table(ctx), out);
    else
        hipLaunchKernelGGL((k_query_reads<W, false>), dim3(grid), dim3(256), 0, ctx->stream, q.packed.as<u64>(), q.inval.as<u32>(), nwords, nbytes,
                           (int)ctx->cfg.kmer_size, query_table(ctx), out);
}

template <int W>
void launch_kmers(dskgpu_ctx* ctx, const u64* keys, u64 n, u32* out) {
    const u64 per_block = 256ull * QBatch<W>::N;
    const unsigned grid = (unsigned)((n + per_block - 1) / per_block);
    hipLaunchKernelGGL(k_query_kmers<W>, dim3(grid), dim3(256), 0, ctx->stream, keys, n, ctx->words_out, query_table(ctx), out);
}

}  // namespace

extern "C" {

int dskgpu_query_prepare(dskgpu_ctx* ctx) {
    if (!ctx) return DSKGPU_E_ARG;
    CK(hipSetDevice(ctx->cfg.device));
    query_begin(ctx);
    if (const int rc = ensure_index(ctx)) return rc;
    ctx->mark("query index");
    return query_finish(ctx);
}

int dskgpu_query_kmers(dskgpu_ctx* ctx, const void* d_kmers, uint64_t n, void* d_abundance) {
    if (!ctx) return DSKGPU_E_ARG;
    if (n == 0) return DSKGPU_OK;
    if (!d_kmers || !d_abundance) return fail(ctx, DSKGPU_E_ARG, "dskgpu_query_kmers: null pointer");
    if (n > (0x7FFFFFFFull << 8)) return fail(ctx, DSKGPU_E_ARG, "dskgpu_query_kmers: more values than one launch takes; split the call");
    CK(hipSetDevice(ctx->cfg.device));
    query_begin(ctx);
    if (const int rc = ensure_index(ctx)) return rc;
    ctx->mark("query index");
    const u64* keys = static_cast<const u64*>(d_kmers); u32* out = static_cast<u32*>(d_abundance);
    if (ctx->W == 1) launch_kmers<1>(ctx, keys, n, out); else if (ctx->W == 2) launch_kmers<2>(ctx, keys, n, out); else launch_kmers<4>(ctx, keys, n, out);
    CKL("k_query_kmers");
    ctx->mark("query");
    return query_finish(ctx);
}

int dskgpu_query_reads(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, void* d_abundance) {
    if (!ctx) return DSKGPU_E_ARG;
    if (nbytes == 0) return DSKGPU_OK;
    if (!d_bytes || !d_abundance) return fail(ctx, DSKGPU_E_ARG, "dskgpu_query_reads: null pointer");
    if (nbytes > (0x7FFFFFFFull << 11)) return fail(ctx, DSKGPU_E_ARG, "dskgpu_query_reads: a longer stream than one launch takes; split the call");
    CK(hipSetDevice(ctx->cfg.device));
    query_begin(ctx);
    if (const int rc = ensure_index(ctx)) return rc;
    ctx->mark("query index");
    Query& q = ctx->query;
    const u64 nwords = (nbytes + 31) / 32;
    if (const int rc = query_ensure(ctx, q.packed, (nwords + 1) * 8, "encode buffer")) return rc;
    if (const int rc = query_ensure(ctx, q.inval, (nwords + 1) * 4, "encode buffer")) return rc;
    if (const int rc = encode_into(ctx, static_cast<const uint8_t*>(d_bytes), nbytes, q.packed.as<u64>(), q.inval.as<u32>())) return rc;
    u32* out = static_cast<u32*>(d_abundance);
    if (ctx->W == 1) launch_reads<1>(ctx, nwords, nbytes, out); else if (ctx->W == 2) launch_reads<2>(ctx, nwords, nbytes, out); else launch_reads<4>(ctx, nwords, nbytes, out);
    CKL("k_query_reads");
    ctx->mark("query");
    return query_finish(ctx);
}

}  // extern "C"
