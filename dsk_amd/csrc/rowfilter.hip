// rowfilter.hip -- rows taken out of a result on the device, and the rounds of (a rule -> the filter of the rows it flags) that the graph
// rules run with it: dskgpu_filter_rows (include/dskgpu.h), round_once / rounds_run and their parts (engine.h).  Host side of rowfilter.h;
// owns dskgpu_ctx::filtered.  The filter reads the result (res_w / res_ab / n_rows) and the partition layout (rows_partition_range) and
// leaves both describing the kept rows, in buffers of its own; the lookup index, the compaction and the edges are marked stale and built
// again, in the memory they have, by whoever asks next.  A round of rounds_run reads back ONE record: the four counters of the rule and the
// new partition offsets, the last of which is the kept total.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "engine.h"
#include "rowfilter.h"

// ---- the machinery of a round (engine.h), shared with rules.hip and components.hip
int abandon(dskgpu_ctx* ctx, int rc) {
    (void)hipStreamSynchronize(ctx->stream);
    ctx->marks.clear(); ctx->ev_used = 0;
    return rc;
}

// the record of a round: [REC_COUNTERS counters, zeroed | one new offset per entry of old_off].  old_off = the first row of every partition
// (DSKGPU_F_PARTITION_ORDER only) and, last, n_rows: its new offset is the kept total
int begin_record(dskgpu_ctx* ctx, bool with_offsets, std::vector<u64>& old_off) {
    Filtered& F = ctx->filtered;
    old_off.clear();
    if (with_offsets) {
        if (ctx->rs.part_mode) {
            const u32 P = rows_partitions(ctx);
            for (u32 p = 0; p < P; ++p) { u64 b, e; rows_partition_range(ctx, p, &b, &e); old_off.push_back(b); if (p + 1 == P) old_off.push_back(e); }
            if (P == 0) old_off.push_back(0);
        }
        old_off.push_back(ctx->n_rows);
    }
    if (const int rc = query_ensure(ctx, F.rec, (REC_COUNTERS + old_off.size()) * 8, "tip record")) return rc;
    CK(hipMemsetAsync(F.rec.p, 0, REC_COUNTERS * 8, ctx->stream));
    return DSKGPU_OK;
}

// enqueue: the exclusive scan of the keep flags and, from it, the new offsets into the record.  n_rows > 0; old_off lives until the read-back
int filter_scan(dskgpu_ctx* ctx, const unsigned char* keep, const std::vector<u64>& old_off) {
    Filtered& F = ctx->filtered;
    const u64 n = ctx->n_rows, n_off = old_off.size();
    if (const int rc = query_ensure(ctx, F.scan, n * 8, "keep scan")) return rc;
    if (const int rc = query_ensure(ctx, F.off_in, n_off * 8, "partition offsets")) return rc;
    u64* scan = F.scan.as<u64>();
    auto flags = rocprim::make_transform_iterator(keep, TKeepFlag());
    size_t tmp_bytes = 0;
    CK(rocprim::exclusive_scan(nullptr, tmp_bytes, flags, scan, 0ull, (size_t)n, rocprim::plus<u64>(), ctx->stream));      // LIBRARY SCAN (rocprim): plumbing, one pass over a byte per row
    if (const int rc = query_ensure(ctx, F.tmp, tmp_bytes ? tmp_bytes : 8, "keep scan")) return rc;
    CK(rocprim::exclusive_scan(F.tmp.p, tmp_bytes, flags, scan, 0ull, (size_t)n, rocprim::plus<u64>(), ctx->stream));
    CK(hipMemcpyAsync(F.off_in.p, old_off.data(), n_off * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_filter_offsets, dim3(blocks(n_off, 256)), dim3(256), 0, ctx->stream, F.off_in.as<u64>(), n_off, scan, keep, n, F.rec.as<u64>() + REC_COUNTERS);
    CKL("k_filter_offsets");
    return DSKGPU_OK;
}

namespace {

template <int W>
void launch_compact(dskgpu_ctx* ctx, const unsigned char* keep, u64 n_kept, int dst) {
    Filtered& F = ctx->filtered;
    RowsIn in; RowsOut out;
    for (int x = 0; x < 4; ++x) { in.w[x] = ctx->res_w[x]; out.w[x] = x < W ? F.w[dst][x].as<u64>() : nullptr; }
    hipLaunchKernelGGL(k_rows_compact<W>, dim3(blocks(ctx->n_rows, 256)), dim3(256), 0, ctx->stream, in, ctx->res_ab, keep, F.scan.as<u64>(), ctx->n_rows, n_kept,
                       out, F.ab[dst].as<u32>());
}

}  // namespace

// the kept rows into the set that does not hold the result, then the result is that set.  new_off: the record's offsets on the host.
// Nothing of the context changes before every buffer is there and the kernel is enqueued
int filter_apply(dskgpu_ctx* ctx, const unsigned char* keep, const u64* new_off, u64 n_off) {
    Filtered& F = ctx->filtered;
    const u64 n = ctx->n_rows, n_kept = new_off[n_off - 1];
    const int W = ctx->W, dst = F.cur == 0 ? 1 : 0;
    if (n_kept > n) return fail(ctx, DSKGPU_E_DEVICE, "dskgpu_filter_rows: more rows kept than there are (internal error)");
    for (u64 i = 0; i + 1 < n_off; ++i)
        if (new_off[i] > new_off[i + 1]) return fail(ctx, DSKGPU_E_DEVICE, "dskgpu_filter_rows: the kept partitions do not ascend (internal error)");
    for (int x = 0; x < W; ++x)
        if (const int rc = query_ensure(ctx, F.w[dst][x], (n_kept + 1) * 8, "kept rows")) return rc;
    if (const int rc = query_ensure(ctx, F.ab[dst], (n_kept + 1) * 4, "kept rows")) return rc;
    if (W == 1) launch_compact<1>(ctx, keep, n_kept, dst); else if (W == 2) launch_compact<2>(ctx, keep, n_kept, dst); else launch_compact<4>(ctx, keep, n_kept, dst);
    CKL("k_rows_compact");
    for (int x = 0; x < 4; ++x) ctx->res_w[x] = x < W ? F.w[dst][x].as<u64>() : nullptr;
    ctx->res_ab = F.ab[dst].as<u32>();
    ctx->n_rows = n_kept;
    F.cur = dst;
    if (ctx->rs.part_mode) F.part_off.assign(new_off, new_off + (n_off - 1)); else F.part_off.clear();
    ctx->query.invalidate(); ctx->unitigs.invalidate(); ctx->threading.release(); ctx->variants.release(); ctx->readsum.release(); ctx->colors.release();
    return DSKGPU_OK;
}

int read_record(dskgpu_ctx* ctx, std::vector<u64>& h, u64 n_off) {
    h.assign(REC_COUNTERS + n_off, 0);
    CK(hipMemcpyAsync(h.data(), ctx->filtered.rec.p, h.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return DSKGPU_OK;
}

int flag_rows(dskgpu_ctx* ctx, unsigned char* d_row_flag, bool want_keep) {
    Filtered& F = ctx->filtered;
    const Unitigs& U = ctx->unitigs;
    const u64 n = ctx->n_rows;
    if (!d_row_flag && !want_keep) return DSKGPU_OK;
    if (want_keep) if (const int rc = query_ensure(ctx, F.keep, n, "keep flags")) return rc;
    hipLaunchKernelGGL(k_tip_rows, dim3(blocks(n, 256)), dim3(256), 0, ctx->stream, U.unitig.as<u32>(), F.bits.as<unsigned char>(), n, U.stats.n_unitigs, d_row_flag,
                       want_keep ? F.keep.as<unsigned char>() : (unsigned char*)nullptr);
    CKL("k_tip_rows");
    return DSKGPU_OK;
}

// one round of a rule on the current result, no row changes (dskgpu_graph_tips and its kin, whose arguments the caller has checked): builds
// the edges, enqueues the rule, copies the bits out and reads the counters back.  A result without rows: zero counters, nothing written
int round_once(dskgpu_ctx* ctx, const char* who, const char* stage, RoundEnqueue enqueue, const void* params, void* d_row_flag, void* d_unitig_bits, u64* counters) {
    std::fill(counters, counters + REC_COUNTERS, 0ull);
    if (const int rc = ensure_edges(ctx, who)) return rc;
    if (ctx->n_rows == 0) return query_finish(ctx);
    std::vector<u64> old_off, h;
    if (const int rc = begin_record(ctx, false, old_off)) return abandon(ctx, rc);
    if (const int rc = enqueue(ctx, params, static_cast<unsigned char*>(d_row_flag), false)) return abandon(ctx, rc);
    if (d_unitig_bits) CK(hipMemcpyAsync(d_unitig_bits, ctx->filtered.bits.p, ctx->unitigs.stats.n_unitigs, hipMemcpyDeviceToDevice, ctx->stream));
    ctx->mark(stage);
    if (const int rc = read_record(ctx, h, 0)) return abandon(ctx, rc);
    if (const int rc = query_finish(ctx)) return rc;
    std::copy(h.begin(), h.begin() + REC_COUNTERS, counters);
    return DSKGPU_OK;
}

// rounds of (the rule -> the filter of the rows it flags) until a round flags no row or max_rounds rounds have removed some (dskgpu_clip_tips
// and its kin).  counters: the sums over the rounds that ran, the last one that removed nothing included; *n_rounds: the rounds that removed
// something.  On return, an error or not, the context holds the result of the rounds that were done
int rounds_run(dskgpu_ctx* ctx, const char* who, const char* stage, u64 max_rounds, RoundEnqueue enqueue, const void* params, u64* counters, u64* n_rounds) {
    std::fill(counters, counters + REC_COUNTERS, 0ull);
    *n_rounds = 0;
    std::vector<u64> old_off, h;
    int rc = DSKGPU_OK;
    for (;;) {
        if ((rc = ensure_edges(ctx, who))) break;                            // (of the final rows too: the graph is ready when the call returns)
        if (ctx->n_rows == 0 || *n_rounds == max_rounds) { rc = query_finish(ctx); break; }
        const u64 n = ctx->n_rows;
        if ((rc = begin_record(ctx, true, old_off)) || (rc = enqueue(ctx, params, nullptr, true))) { abandon(ctx, rc); break; }
        ctx->mark(stage);
        const unsigned char* keep = ctx->filtered.keep.as<unsigned char>();
        if ((rc = filter_scan(ctx, keep, old_off)) || (rc = read_record(ctx, h, old_off.size()))) { abandon(ctx, rc); break; }
        if (h[REC_ROWS] == 0) {                                               // (every unitig has a row: no row flagged <=> no unitig flagged)
            for (int i = 0; i < REC_COUNTERS; ++i) counters[i] += h[i];
            rc = query_finish(ctx);
            break;
        }
        if (h[REC_ROWS] + h.back() != n) { rc = abandon(ctx, fail(ctx, DSKGPU_E_DEVICE, std::string(who) + ": the removed rows and the kept rows do not add up (internal error)")); break; }
        if ((rc = filter_apply(ctx, keep, h.data() + REC_COUNTERS, old_off.size()))) { abandon(ctx, rc); break; }
        ctx->mark("filter rows");
        for (int i = 0; i < REC_COUNTERS; ++i) counters[i] += h[i];
        ++*n_rounds;
        if ((rc = query_finish(ctx))) break;
    }
    return rc;
}

extern "C" {

int dskgpu_filter_rows(dskgpu_ctx* ctx, const void* d_keep, uint64_t* n_kept) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!ctx->have_result) return fail(ctx, DSKGPU_E_STATE, "no result to filter: count first");
    if (ctx->n_rows == 0) { if (n_kept) *n_kept = 0; return DSKGPU_OK; }
    if (!d_keep) return fail(ctx, DSKGPU_E_ARG, "dskgpu_filter_rows: null d_keep");
    CK(hipSetDevice(ctx->cfg.device));
    query_begin(ctx);
    const unsigned char* keep = static_cast<const unsigned char*>(d_keep);
    std::vector<u64> old_off, h;
    if (const int rc = begin_record(ctx, true, old_off)) return abandon(ctx, rc);
    if (const int rc = filter_scan(ctx, keep, old_off)) return abandon(ctx, rc);
    if (const int rc = read_record(ctx, h, old_off.size())) return abandon(ctx, rc);
    if (const int rc = filter_apply(ctx, keep, h.data() + REC_COUNTERS, old_off.size())) return abandon(ctx, rc);
    ctx->mark("filter rows");
    if (const int rc = query_finish(ctx)) return rc;
    if (n_kept) *n_kept = ctx->n_rows;
    return DSKGPU_OK;
}

}  // extern "C"
