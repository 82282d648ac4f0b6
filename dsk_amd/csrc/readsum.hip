// readsum.hip -- per-read abundance summaries and read selection: dskgpu_read_summaries / _read_summaries_table / _read_marks /
// dskgpu_select_reads (include/dskgpu.h).  Host side of readsum.h; owns dskgpu_ctx::readsum.  dskgpu_read_summaries reads the lookup index
// (ensure_index builds it) and the result's rows and encodes the stream into scratch of its own, which goes -- with the values, the valid
// bits, the record ends and the block sums -- when the call returns; what is kept is the table.  dskgpu_select_reads reads nothing of the
// context but its stream and its device.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include "engine.h"
#include "readsum.h"

namespace {

struct Scratch {
    DevBuf packed, inval, vals, vbits, bsum, bbase, tmp, ends, list, olen, obase, stat;
    ~Scratch() { for (DevBuf* b : {&packed, &inval, &vals, &vbits, &bsum, &bbase, &tmp, &ends, &list, &olen, &obase, &stat}) b->release(); }
};

int scan64(dskgpu_ctx* ctx, DevBuf& tmp, u64* in, u64* out, u64 n) {
    size_t tmp_bytes = 0;
    CK(rocprim::exclusive_scan(nullptr, tmp_bytes, in, out, 0ull, (size_t)n, rocprim::plus<u64>(), ctx->stream));      // LIBRARY SCAN (rocprim): plumbing, 8 bytes per 4096 positions or per record
    if (const int rc = query_ensure(ctx, tmp, tmp_bytes ? tmp_bytes : 8, "record scan")) return rc;
    CK(rocprim::exclusive_scan(tmp.p, tmp_bytes, in, out, 0ull, (size_t)n, rocprim::plus<u64>(), ctx->stream));
    return DSKGPU_OK;
}

unsigned record_grid(const dskgpu_ctx* ctx, u64 items, u64 per_block) {          // a grid-stride kernel over the records
    return (unsigned)std::max<u64>(1, std::min<u64>((items + per_block - 1) / per_block, (u64)ctx->num_cu * 32));
}

template <bool EMIT>
void launch_records(dskgpu_ctx* ctx, const Scratch& S, const unsigned char* s, u64 nbytes, u64 nblocks, u64 n_nl, u64 n_rec) {
    u64 *bsum = EMIT ? nullptr : S.bsum.as<u64>(), *ends = EMIT ? S.ends.as<u64>() : nullptr;
    const u64* bbase = EMIT ? S.bbase.as<u64>() : nullptr;
    if ((reinterpret_cast<uintptr_t>(s) & 15) == 0)
        hipLaunchKernelGGL((k_rs_records<EMIT, true>), dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, s, nbytes, bsum, bbase, ends, n_nl, n_rec);
    else
        hipLaunchKernelGGL((k_rs_records<EMIT, false>), dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, s, nbytes, bsum, bbase, ends, n_nl, n_rec);
}

// the records of the stream (nbytes > 0): count per block, scan, one read-back of the total and of the last byte, emit -> S.ends, *n_rec
int find_records(dskgpu_ctx* ctx, Scratch& S, const void* d_bytes, u64 nbytes, u64* n_rec_out) {
    const unsigned char* s = static_cast<const unsigned char*>(d_bytes);
    const u64 nblocks = (nbytes + RS_BLOCK - 1) / RS_BLOCK;
    if (const int rc = query_ensure(ctx, S.bsum, (nblocks + 1) * 8, "record block sums")) return rc;
    if (const int rc = query_ensure(ctx, S.bbase, (nblocks + 1) * 8, "record block sums")) return rc;
    CK(hipMemsetAsync(S.bsum.as<u64>() + nblocks, 0, 8, ctx->stream));              // the scan's last input: bbase[nblocks] = the total
    launch_records<false>(ctx, S, s, nbytes, nblocks, 0, 0);
    CKL("k_rs_records");
    if (const int rc = scan64(ctx, S.tmp, S.bsum.as<u64>(), S.bbase.as<u64>(), nblocks + 1)) return rc;
    u64 n_nl = 0;
    unsigned char last = 0;
    CK(hipMemcpyAsync(&n_nl, S.bbase.as<u64>() + nblocks, 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(&last, s + nbytes - 1, 1, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    if (n_nl > nbytes) return fail(ctx, DSKGPU_E_DEVICE, "read records: more line ends than bytes (internal error)");
    const u64 n_rec = n_nl + (last != 0x0A ? 1 : 0);
    if (const int rc = query_ensure(ctx, S.ends, (n_rec + 1) * 8, "record ends")) return rc;
    launch_records<true>(ctx, S, s, nbytes, nblocks, n_nl, n_rec);
    CKL("k_rs_records");
    *n_rec_out = n_rec;
    return DSKGPU_OK;
}

template <int W>
void launch_values(dskgpu_ctx* ctx, const Scratch& S, u64 nwords, u64 nbytes) {
    constexpr int TPW = 32 / QBatch<W>::N;
    const unsigned grid = (unsigned)((nwords * TPW + 255) / 256);
    hipLaunchKernelGGL(k_rs_values<W>, dim3(grid), dim3(256), 0, ctx->stream, S.packed.as<u64>(), S.inval.as<u32>(), nwords, nbytes, (int)ctx->cfg.kmer_size,
                       query_table(ctx), S.vals.as<u32>(), S.vbits.as<u32>());
}

int summarise(dskgpu_ctx* ctx, const void* d_bytes, u64 nbytes, u32 tmin) {
    ReadSummaries& R = ctx->readsum;
    Scratch S;
    const u64 nwords = (nbytes + 31) / 32;
    if (const int rc = query_ensure(ctx, S.packed, (nwords + 1) * 8, "encode buffer")) return rc;
    if (const int rc = query_ensure(ctx, S.inval, (nwords + 1) * 4, "encode buffer")) return rc;
    if (const int rc = query_ensure(ctx, S.vals, nwords * 32 * 4, "read values")) return rc;
    if (const int rc = query_ensure(ctx, S.vbits, (nwords + 1) * 4, "read values")) return rc;
    if (const int rc = query_ensure(ctx, S.stat, RS_ST_COUNT * 8, "read counters")) return rc;
    CK(hipMemsetAsync(S.stat.p, 0, RS_ST_COUNT * 8, ctx->stream));
    if (const int rc = encode_into(ctx, static_cast<const uint8_t*>(d_bytes), nbytes, S.packed.as<u64>(), S.inval.as<u32>())) return rc;
    if (ctx->W == 1) launch_values<1>(ctx, S, nwords, nbytes); else if (ctx->W == 2) launch_values<2>(ctx, S, nwords, nbytes); else launch_values<4>(ctx, S, nwords, nbytes);
    CKL("k_rs_values");
    ctx->mark("read values");

    u64 n_rec = 0;
    if (const int rc = find_records(ctx, S, d_bytes, nbytes, &n_rec)) return rc;
    u64* stat = S.stat.as<u64>();
    u64 h[RS_ST_COUNT] = {0};
    if (n_rec) {
        if (const int rc = query_ensure(ctx, R.table, n_rec * sizeof(RsSummary), "read summaries")) return rc;
        if (const int rc = query_ensure(ctx, S.list, (nbytes / ((u64)RS_WAVE_CAP + 1) + 1) * 8, "long records")) return rc;
        hipLaunchKernelGGL(k_rs_spans, dim3(record_grid(ctx, n_rec, 256)), dim3(256), 0, ctx->stream, (const u64*)S.ends.as<u64>(), n_rec, R.table.as<RsSummary>(), S.list.as<u64>(), stat);
        CKL("k_rs_spans");
        CK(hipMemcpyAsync(h, stat, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));          // one read-back: the long records, a record above the limit
        CK(hipStreamSynchronize(ctx->stream));
        if (h[RS_ST_TOOLONG]) return fail(ctx, DSKGPU_E_ARG, "dskgpu_read_summaries: a record is longer than 2^32 - 1 bytes; a summary holds its length in 32 bits");
        if (h[RS_ST_NLONG] > nbytes / ((u64)RS_WAVE_CAP + 1) + 1) return fail(ctx, DSKGPU_E_DEVICE, "dskgpu_read_summaries: more long records than the stream holds (internal error)");
    }
    ctx->mark("read records");

    if (n_rec) {
        hipLaunchKernelGGL(k_rs_short, dim3(record_grid(ctx, n_rec, 4)), dim3(256), 0, ctx->stream, (const u32*)S.vals.as<u32>(), (const u32*)S.vbits.as<u32>(), n_rec, tmin,
                           R.table.as<RsSummary>(), stat);
        CKL("k_rs_short");
        if (const u64 n_long = h[RS_ST_NLONG]) {
            hipLaunchKernelGGL(k_rs_long, dim3(record_grid(ctx, n_long, 1)), dim3(256), 0, ctx->stream, (const u32*)S.vals.as<u32>(), (const u32*)S.vbits.as<u32>(),
                               (const u64*)S.list.as<u64>(), n_long, tmin, R.table.as<RsSummary>(), stat);
            CKL("k_rs_long");
        }
    }
    ctx->mark("read summaries");
    CK(hipMemcpyAsync(h, stat, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));                                           // the scratch goes when this returns
    R.stats.n_records = n_rec; R.stats.n_empty = h[RS_ST_EMPTY]; R.stats.n_valid = h[RS_ST_VALID]; R.stats.n_solid = h[RS_ST_SOLID]; R.stats.max_len = h[RS_ST_MAXLEN];
    return DSKGPU_OK;
}

int select_records(dskgpu_ctx* ctx, const void* d_bytes, u64 nbytes, const void* d_keep, u64 n_records, void* d_out, u64 capacity, uint64_t* out_bytes, uint64_t* out_records) {
    Scratch S;
    u64 n_rec = 0;
    if (const int rc = find_records(ctx, S, d_bytes, nbytes, &n_rec)) return rc;
    ctx->mark("read records");
    if (n_rec != n_records) return fail(ctx, DSKGPU_E_ARG, "dskgpu_select_reads: n_records is " + std::to_string(n_records) + ", the stream has " + std::to_string(n_rec) + " records");
    const unsigned char* keep = static_cast<const unsigned char*>(d_keep);
    const u64 max_long = nbytes / ((u64)RS_WAVE_CAP + 1) + 1;
    if (const int rc = query_ensure(ctx, S.stat, RS_ST_COUNT * 8, "read counters")) return rc;
    if (const int rc = query_ensure(ctx, S.olen, (n_rec + 1) * 8, "kept lengths")) return rc;
    if (const int rc = query_ensure(ctx, S.obase, (n_rec + 1) * 8, "kept lengths")) return rc;
    if (const int rc = query_ensure(ctx, S.list, max_long * 8, "long records")) return rc;
    CK(hipMemsetAsync(S.stat.p, 0, RS_ST_COUNT * 8, ctx->stream));
    u64* stat = S.stat.as<u64>();
    const u64* ends = S.ends.as<u64>();
    hipLaunchKernelGGL(k_rs_outlen, dim3(record_grid(ctx, n_rec + 1, 256)), dim3(256), 0, ctx->stream, ends, n_rec, keep, S.olen.as<u64>(), S.list.as<u64>(), stat);
    CKL("k_rs_outlen");
    if (const int rc = scan64(ctx, S.tmp, S.olen.as<u64>(), S.obase.as<u64>(), n_rec + 1)) return rc;
    u64 h[RS_ST_COUNT] = {0}, need = 0;
    CK(hipMemcpyAsync(h, stat, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(&need, S.obase.as<u64>() + n_rec, 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    if (need > nbytes + 1 || h[RS_ST_KEPT] > n_rec || h[RS_ST_NLONG] > max_long) return fail(ctx, DSKGPU_E_DEVICE, "dskgpu_select_reads: the kept records do not add up (internal error)");
    if (out_bytes) *out_bytes = need;
    if (out_records) *out_records = h[RS_ST_KEPT];
    if (d_out && capacity < need) return fail(ctx, DSKGPU_E_ARG, "dskgpu_select_reads: the selection takes " + std::to_string(need) + " bytes, capacity is " + std::to_string(capacity));
    if (d_out && need) {
        const unsigned char* s = static_cast<const unsigned char*>(d_bytes);
        unsigned char* out = static_cast<unsigned char*>(d_out);
        hipLaunchKernelGGL(k_rs_copy_short, dim3(record_grid(ctx, n_rec, 4)), dim3(256), 0, ctx->stream, s, ends, n_rec, keep, (const u64*)S.obase.as<u64>(), out);
        CKL("k_rs_copy_short");
        if (const u64 n_long = h[RS_ST_NLONG]) {
            hipLaunchKernelGGL(k_rs_copy_long, dim3(record_grid(ctx, n_long, 1)), dim3(256), 0, ctx->stream, s, ends, (const u64*)S.list.as<u64>(), n_long, (const u64*)S.obase.as<u64>(), out);
            CKL("k_rs_copy_long");
        }
    }
    ctx->mark("read select");
    CK(hipStreamSynchronize(ctx->stream));                                           // the scratch goes when this returns
    return DSKGPU_OK;
}

}  // namespace

extern "C" {

int dskgpu_read_summaries(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, const dskgpu_read_summary_params* params, dskgpu_read_summary_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (nbytes && !d_bytes) return fail(ctx, DSKGPU_E_ARG, "dskgpu_read_summaries: null pointer");
    if (params && (params->flags || params->reserved[0] || params->reserved[1] || params->reserved[2]))
        return fail(ctx, DSKGPU_E_ARG, "dskgpu_read_summaries: flags and reserved words must be 0");
    if (nbytes > (0x7FFFFFFFull << 11)) return fail(ctx, DSKGPU_E_ARG, "dskgpu_read_summaries: a longer stream than one launch takes; split the call");
    if (ctx->cfg.world_size > 1)
        return fail(ctx, DSKGPU_E_STATE, "dskgpu_read_summaries: a rank holds only the k-mers it owns; its rows do not give a read's abundances (world_size > 1)");
    if (!ctx->have_result) return fail(ctx, DSKGPU_E_STATE, "no result to summarise reads against: count first");
    CK(hipSetDevice(ctx->cfg.device));
    ReadSummaries& R = ctx->readsum;
    R.release();
    if (nbytes == 0) { R.valid = true; if (stats) *stats = R.stats; return DSKGPU_OK; }
    query_begin(ctx);
    if (const int rc = ensure_index(ctx)) return abandon(ctx, rc);
    ctx->mark("query index");
    const u32 tmin = params && params->trust_min > 1 ? params->trust_min : 1u;       // (0 and 1: any row)
    int rc = summarise(ctx, d_bytes, nbytes, tmin);
    if (rc == DSKGPU_OK) rc = query_finish(ctx); else rc = abandon(ctx, rc);
    if (rc != DSKGPU_OK) { R.release(); return rc; }
    R.valid = true;
    if (stats) *stats = R.stats;
    return DSKGPU_OK;
}

int dskgpu_read_summaries_table(dskgpu_ctx* ctx, void* d_records) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!d_records) return fail(ctx, DSKGPU_E_ARG, "dskgpu_read_summaries_table: null pointer");
    const ReadSummaries& R = ctx->readsum;
    if (!R.valid) return fail(ctx, DSKGPU_E_STATE, "dskgpu_read_summaries_table: no table is kept: dskgpu_read_summaries first");
    CK(hipSetDevice(ctx->cfg.device));
    if (R.stats.n_records) CK(hipMemcpyAsync(d_records, R.table.p, R.stats.n_records * sizeof(RsSummary), hipMemcpyDeviceToDevice, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return DSKGPU_OK;
}

int dskgpu_read_marks(dskgpu_ctx* ctx, const dskgpu_read_rule* rule, void* d_keep, dskgpu_read_mark_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!d_keep && !stats) return fail(ctx, DSKGPU_E_ARG, "dskgpu_read_marks: neither d_keep nor stats");
    if (rule && ((rule->flags & ~DSKGPU_READS_INVERT) || rule->reserved)) return fail(ctx, DSKGPU_E_ARG, "dskgpu_read_marks: unknown flag bits or a non-zero reserved word");
    const ReadSummaries& R = ctx->readsum;
    if (!R.valid) return fail(ctx, DSKGPU_E_STATE, "dskgpu_read_marks: no table is kept: dskgpu_read_summaries first");
    CK(hipSetDevice(ctx->cfg.device));
    dskgpu_read_mark_stats out{};
    const u64 n_rec = R.stats.n_records;
    out.n_records = n_rec;
    if (n_rec) {
        Scratch S;
        if (const int rc = query_ensure(ctx, S.stat, RS_ST_COUNT * 8, "read counters")) return rc;
        CK(hipMemsetAsync(S.stat.p, 0, RS_ST_COUNT * 8, ctx->stream));
        const RsRule rr = rule ? RsRule{rule->min_valid, rule->median_min, rule->median_max, rule->solid_num, rule->solid_den, rule->flags & DSKGPU_READS_INVERT} : RsRule{0u, 0u, 0u, 0u, 0u, 0u};
        hipLaunchKernelGGL(k_rs_marks, dim3(record_grid(ctx, n_rec, 256)), dim3(256), 0, ctx->stream, (const RsSummary*)R.table.as<RsSummary>(), n_rec, rr, static_cast<unsigned char*>(d_keep), S.stat.as<u64>());
        CKL("k_rs_marks");
        u64 h[RS_ST_COUNT] = {0};
        CK(hipMemcpyAsync(h, S.stat.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        out.n_kept = h[RS_ST_KEPT]; out.kept_bytes = h[RS_ST_KBYTES]; out.kept_valid = h[RS_ST_KVALID];
    }
    if (stats) *stats = out;
    return DSKGPU_OK;
}

int dskgpu_select_reads(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, const void* d_keep, uint64_t n_records, void* d_out, uint64_t capacity,
                        uint64_t* out_bytes, uint64_t* out_records) {
    if (!ctx) return DSKGPU_E_ARG;
    if (nbytes && !d_bytes) return fail(ctx, DSKGPU_E_ARG, "dskgpu_select_reads: null pointer");
    if (n_records && !d_keep) return fail(ctx, DSKGPU_E_ARG, "dskgpu_select_reads: null d_keep");
    if (nbytes > (0x7FFFFFFFull << 11)) return fail(ctx, DSKGPU_E_ARG, "dskgpu_select_reads: a longer stream than one launch takes; split the call");
    if (nbytes == 0) {
        if (n_records) return fail(ctx, DSKGPU_E_ARG, "dskgpu_select_reads: n_records is not 0, the stream has 0 records");
        if (out_bytes) *out_bytes = 0;
        if (out_records) *out_records = 0;
        return DSKGPU_OK;
    }
    CK(hipSetDevice(ctx->cfg.device));
    query_begin(ctx);
    if (const int rc = select_records(ctx, d_bytes, nbytes, d_keep, n_records, d_out, capacity, out_bytes, out_records)) return abandon(ctx, rc);
    ctx->resolve_marks();
    return DSKGPU_OK;
}

}  // extern "C"
