// loadrows.hip -- dskgpu_load_rows (include/dskgpu.h): saved (k-mer, abundance) rows become the context's result, equal k-mers combined.
// Host side of loadrows.h.  A load is a count whose input is rows: check + transpose (k_load_check) -> the row order (order_rows of rowsort.hip,
// global, skipped for ascending input) -> head flags, their scan, the combined abundances (k_load_heads, run_scan, k_load_combine) -> histogram,
// filter and compaction (k_load_finish, run_scan, k_load_compact).  It keeps no state of its own: the rows end in the count path's row buffers
// (out_* / srt_*), its scratch is the row sort's (srt_k, srt_idx, srt_idx2).  Until the input is known to be valid the buffers that may hold the
// previous result are set aside (Stash), so that DSKGPU_E_ARG leaves that result and everything built on it as it was.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "engine.h"
#include "loadrows.h"

namespace {

struct Scratch {
    DevBuf rec;
    ~Scratch() { rec.release(); }
};

// The buffers the row order works in -- and the previous result may lie in -- set aside while a load that may still end in DSKGPU_E_ARG runs in
// new ones; with them what order_rows changes of the previous result's description.  restore(): the previous result is back; drop(): it is
// gone for good (the load goes on in the new buffers).  Left active (an error on the way): there is no result, and both sets are freed.
struct Stash {
    dskgpu_ctx* ctx; bool active = false;
    DevBuf out_w[4], srt_w[4], out_ab, srt_ab, l0buf;
    const u64* res_w[4] = {nullptr, nullptr, nullptr, nullptr}; const u32* res_ab = nullptr;
    bool part_mode = false; u32 n_parts = 0; u64 sort_fallback = 0;
    explicit Stash(dskgpu_ctx* c) : ctx(c) {}
    void swap_bufs() {
        for (int x = 0; x < 4; ++x) { std::swap(out_w[x], ctx->out_w[x]); std::swap(srt_w[x], ctx->srt_w[x]); }
        std::swap(out_ab, ctx->out_ab); std::swap(srt_ab, ctx->srt_ab); std::swap(l0buf, ctx->l0buf);
    }
    void free_mine() { for (int x = 0; x < 4; ++x) { out_w[x].release(); srt_w[x].release(); } out_ab.release(); srt_ab.release(); l0buf.release(); }
    void take() {
        swap_bufs();
        for (int x = 0; x < 4; ++x) res_w[x] = ctx->res_w[x];
        res_ab = ctx->res_ab; part_mode = ctx->rs.part_mode; n_parts = ctx->rs.n_parts; sort_fallback = ctx->stats.sort_fallback;
        active = true;
    }
    void restore() {
        if (!active) return;
        swap_bufs(); free_mine();
        for (int x = 0; x < 4; ++x) ctx->res_w[x] = res_w[x];
        ctx->res_ab = res_ab; ctx->rs.part_mode = part_mode; ctx->rs.n_parts = n_parts; ctx->stats.sort_fallback = sort_fallback;
        active = false;
    }
    void drop() { if (active) free_mine(); active = false; }
    ~Stash() { if (active) { (void)hipStreamSynchronize(ctx->stream); ctx->drop_result(); free_mine(); } }
};

// what is wrong with input row i (host copy of its ow words and its abundance), or null
const char* row_fault(const u64* w, int ow, u32 ab, u32 k) {
    u64 x[4] = {0, 0, 0, 0}, rc[4] = {0, 0, 0, 0};
    for (int j = 0; j < ow; ++j) {
        x[j] = w[j];
        const int bits = 2 * (int)k - 64 * j;
        if (bits < 64 && (bits <= 0 ? x[j] : x[j] >> bits) != 0ull) return "is not below 4^k";
    }
    for (u32 i = 0; i < k; ++i) {
        const u64 b = ((x[(2 * i) >> 6] >> ((2 * i) & 63)) & 3ull) ^ 2ull;
        const u32 t = k - 1 - i;
        rc[(2 * t) >> 6] |= b << ((2 * t) & 63);
    }
    for (int j = 3; j >= 0; --j) if (rc[j] != x[j]) { if (rc[j] < x[j]) return "is not canonical (its reverse complement is smaller)"; break; }
    if (ab == 0) return "has abundance 0";
    return nullptr;
}

int read_row(dskgpu_ctx* ctx, const u64* in, const u32* ab, u64 i, int ow, u64* w, u32* a) {
    CK(hipMemcpyAsync(w, in + i * (u64)ow, (size_t)ow * 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(a, ab + i, 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return DSKGPU_OK;
}

template <int W>
int launch_combine(dskgpu_ctx* ctx, u32 combine, RowsIn rows, const u32* ab, u64 n, const u32* pos, RowsOut dk, u64* acc) {
    const dim3 grid(blocks(n, (u64)LR_BLOCK * LR_RPT));
    if (combine == DSKGPU_LOAD_MAX) hipLaunchKernelGGL((k_load_combine<W, LR_M_MAX>), grid, dim3(LR_BLOCK), 0, ctx->stream, rows, ab, n, pos, dk, acc);
    else if (combine == DSKGPU_LOAD_MIN) hipLaunchKernelGGL((k_load_combine<W, LR_M_MIN>), grid, dim3(LR_BLOCK), 0, ctx->stream, rows, ab, n, pos, dk, acc);
    else hipLaunchKernelGGL((k_load_combine<W, LR_M_SUM>), grid, dim3(LR_BLOCK), 0, ctx->stream, rows, ab, n, pos, dk, acc);
    CKL("k_load_combine");
    return DSKGPU_OK;
}

template <int W>
int load_impl(dskgpu_ctx* ctx, const u64* in, const u32* ab, u64 n, u32 combine, dskgpu_load_stats* st) {
    const int ow = ctx->words_out, k = (int)ctx->cfg.kmer_size;
    const u32 nh = ctx->cfg.histo_max + 1;
    const bool unique = combine == DSKGPU_LOAD_UNIQUE;
    const u64 ncu = (u64)ctx->num_cu;
    Scratch S; Stash old(ctx);
    // the point where a count drops the old result: once nothing can end in DSKGPU_E_ARG any more
    auto commit = [&]() {
        ctx->drop_result(); old.drop();
        const u64 fb = ctx->stats.sort_fallback;
        ctx->stats = dskgpu_stats{}; ctx->stats.sort_fallback = fb;
        ctx->banks.forget_hist2d();
        ctx->hist.assign(nh, 0);
    };
    // the stage times of the call before are the previous result's too: they are set aside with it and come back on DSKGPU_E_ARG
    std::vector<const char*> old_names; std::vector<float> old_ms;
    old_names.swap(ctx->st_names); old_ms.swap(ctx->st_ms);
    ctx->marks.clear(); ctx->ev_used = 0;
    auto refuse = [&](const std::string& msg) {
        old.restore();
        ctx->st_names.swap(old_names); ctx->st_ms.swap(old_ms); ctx->marks.clear(); ctx->ev_used = 0;
        return fail(ctx, DSKGPU_E_ARG, msg);
    };
    // (the row order indexes four-word rows with 32 bits up to here; one- and two-word rows have their slab path)
    if (W == 4 && n >= 0xFFFF0000ull) return refuse("dskgpu_load_rows: " + std::to_string(n) + " rows: for k > 64 a load takes fewer than 2^32 - 65536");
    ctx->mark("start");
    CK(ctx->scalars.ensure(SC_COUNT * 4));
    CK(ctx->ghist.ensure(((size_t)nh + 2) * 8));      // (+ 2: k_sort_back's words)
    u32* sc = ctx->scalars.as<u32>();
    if (n == 0) {
        commit();
        for (int x = 0; x < 4; ++x) ctx->res_w[x] = x < W ? ctx->out_w[x].as<u64>() : nullptr;
        ctx->res_ab = ctx->out_ab.as<u32>();
        ctx->rs.part_mode = false; ctx->n_rows = 0; ctx->stats.sort_fallback = 0;
        st->sorted_input = 1;
        ctx->stats.n_partitions = rows_partitions(ctx);
        ctx->have_result = true;
        ctx->marks.clear(); ctx->ev_used = 0;      // (nothing ran: no stage)
        return DSKGPU_OK;
    }
    if (ctx->have_result) old.take();
    // ---- check + transpose
    CK(S.rec.ensure(LR_COUNT * 8));
    u64* rec = S.rec.as<u64>();
    u64 h_rec[LR_COUNT];
    for (int i = 0; i < LR_COUNT; ++i) h_rec[i] = (i == LR_BAD || i == LR_REPEAT) ? ~0ull : 0ull;
    CK(hipMemcpyAsync(rec, h_rec, sizeof(h_rec), hipMemcpyHostToDevice, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));          // (h_rec is read back into below)
    RowsOut in_rows{};
    for (int x = 0; x < W; ++x) { CK(ctx->out_w[x].ensure(n * 8)); in_rows.w[x] = ctx->out_w[x].as<u64>(); }
    CK(ctx->out_ab.ensure(n * 4));
    hipLaunchKernelGGL(k_load_check<W>, dim3((unsigned)std::min<u64>(blocks(n, LR_BLOCK), ncu * 16)), dim3(LR_BLOCK), 0, ctx->stream, in, ab, n, ow, k, in_rows,
                       ctx->out_ab.as<u32>(), rec);
    CKL("k_load_check");
    ctx->mark("load check");
    CK(hipMemcpyAsync(h_rec, rec, sizeof(h_rec), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    if (h_rec[LR_BAD] != ~0ull) {
        const u64 i = h_rec[LR_BAD];
        u64 w[4] = {0, 0, 0, 0}; u32 a = 0;
        if (const int rc = read_row(ctx, in, ab, i, ow, w, &a)) return rc;
        const char* what = row_fault(w, ow, a, (u32)k);
        return refuse("dskgpu_load_rows: row " + std::to_string(i) + " " + (what ? what : "is not a valid row"));
    }
    const bool sorted = h_rec[LR_DESC] == 0;
    if (!unique) commit();
    // ---- order
    for (int x = 0; x < 4; ++x) ctx->res_w[x] = x < W ? ctx->out_w[x].as<u64>() : nullptr;
    ctx->res_ab = ctx->out_ab.as<u32>();
    ctx->rs.part_mode = false;
    ctx->stats.sort_fallback = 0;
    if (!sorted) { if (const int rc = order_rows(ctx, n, 1, true)) return rc; }
    ctx->mark("load order");      // (behind the listed sub-buckets' rounds and the fallback; ascending input: an empty stage)
    RowsIn rows{};
    for (int x = 0; x < W; ++x) rows.w[x] = ctx->res_w[x];
    const u32* rows_ab = ctx->res_ab;
    // ---- the distinct values
    u64 nd = n;
    u32* pos = nullptr;
    if (!sorted) {
        CK(ctx->srt_idx.ensure((n + 1) * 4));
        pos = ctx->srt_idx.as<u32>();
        hipLaunchKernelGGL(k_load_heads<W>, dim3(blocks(n, LR_BLOCK)), dim3(LR_BLOCK), 0, ctx->stream, rows, n, pos);
        hipLaunchKernelGGL(k_load_set, dim3(1), dim3(64), 0, ctx->stream, sc + SC_RSLEN, (u32)n);
        CKL("k_load_heads");
        if (const int rc = run_scan(ctx, pos, sc + SC_RSLEN, n)) return rc;
        u32 h_nd = 0;
        CK(hipMemcpyAsync(&h_nd, pos + n, 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        nd = h_nd;
    }
    if (unique && nd != n) {      // the lowest input index whose value stands at a lower index too
        CK(ctx->srt_idx2.ensure(n * 4));
        u32* first = ctx->srt_idx2.as<u32>();
        CK(hipMemsetAsync(first, 0xFF, n * 4, ctx->stream));
        hipLaunchKernelGGL(k_load_first<W>, dim3(blocks(n, LR_BLOCK)), dim3(LR_BLOCK), 0, ctx->stream, in, n, ow, rows, first);
        hipLaunchKernelGGL(k_load_repeat<W>, dim3(blocks(n, LR_BLOCK)), dim3(LR_BLOCK), 0, ctx->stream, in, n, ow, rows, (const u32*)first, rec);
        CKL("k_load_repeat");
        u64 i = 0;
        CK(hipMemcpyAsync(&i, rec + LR_REPEAT, 8, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        if (i >= n) return fail(ctx, DSKGPU_E_DEVICE, "dskgpu_load_rows: the ordered rows hold a repeat that the input does not");
        u64 w[4] = {0, 0, 0, 0}; u32 a = 0;
        if (const int rc = read_row(ctx, in, ab, i, ow, w, &a)) return rc;
        char hex[80]; std::string val = "0x";
        for (int j = ow - 1; j >= 0; --j) { snprintf(hex, sizeof hex, "%016llx", (unsigned long long)w[j]); val += hex; }
        return refuse("dskgpu_load_rows: row " + std::to_string(i) + " repeats the value " + val + " of a row before it (DSKGPU_LOAD_UNIQUE)");
    }
    if (unique) commit();
    // ---- combine: the keys and 64-bit abundances of the distinct values, into the row set the ordered rows are not in
    const bool merged = nd != n;
    const bool rows_in_out = rows.w[0] == ctx->out_w[0].as<u64>();
    RowsIn dk = rows; const u64* acc = nullptr; const u32* d_ab = rows_ab;
    if (merged) {
        DevBuf* dw = rows_in_out ? ctx->srt_w : ctx->out_w;
        RowsOut dko{};
        for (int x = 0; x < W; ++x) { CK(dw[x].ensure(nd * 8)); dko.w[x] = dw[x].as<u64>(); dk.w[x] = dko.w[x]; }
        CK(ctx->srt_k.ensure(nd * 8));
        CK(hipMemsetAsync(ctx->srt_k.p, combine == DSKGPU_LOAD_MIN ? 0xFF : 0, nd * 8, ctx->stream));
        if (const int rc = launch_combine<W>(ctx, combine, rows, rows_ab, n, pos, dko, ctx->srt_k.as<u64>())) return rc;
        acc = ctx->srt_k.as<u64>(); d_ab = nullptr;
    }
    // ---- histogram, filter, compaction into the other row set
    const bool fin_in_srt = dk.w[0] == ctx->out_w[0].as<u64>();
    DevBuf* fw = fin_in_srt ? ctx->srt_w : ctx->out_w; DevBuf& fab = fin_in_srt ? ctx->srt_ab : ctx->out_ab;
    RowsOut fin{};
    for (int x = 0; x < W; ++x) { CK(fw[x].ensure(nd * 8)); fin.w[x] = fw[x].as<u64>(); }
    CK(fab.ensure(nd * 4));
    CK(ctx->srt_idx2.ensure((nd + 1) * 4));
    u32* keep = ctx->srt_idx2.as<u32>();
    u64* gh = ctx->ghist.as<u64>();
    CK(hipMemsetAsync(gh, 0, (size_t)nh * 8, ctx->stream));
    const u32 nl = std::min<u32>(nh, LR_HIST_LDS);
    const dim3 gfin((unsigned)std::min<u64>(blocks(nd, LR_BLOCK), ncu * 8));
    const u32 amin = ctx->cfg.abundance_min, amax = ctx->cfg.abundance_max;
    if (merged) hipLaunchKernelGGL(k_load_finish<true>, gfin, dim3(LR_BLOCK), ((size_t)nl + 3) * 4, ctx->stream, acc, d_ab, nd, amin, amax, ctx->cfg.histo_max, nl, gh, keep, rec);
    else hipLaunchKernelGGL(k_load_finish<false>, gfin, dim3(LR_BLOCK), ((size_t)nl + 3) * 4, ctx->stream, acc, d_ab, nd, amin, amax, ctx->cfg.histo_max, nl, gh, keep, rec);
    hipLaunchKernelGGL(k_load_set, dim3(1), dim3(64), 0, ctx->stream, sc + SC_RSLEN, (u32)nd);
    CKL("k_load_finish");
    if (const int rc = run_scan(ctx, keep, sc + SC_RSLEN, nd)) return rc;
    if (merged) hipLaunchKernelGGL((k_load_compact<W, true>), dim3(blocks(nd, LR_BLOCK)), dim3(LR_BLOCK), 0, ctx->stream, dk, acc, d_ab, nd, (const u32*)keep, fin, fab.as<u32>());
    else hipLaunchKernelGGL((k_load_compact<W, false>), dim3(blocks(nd, LR_BLOCK)), dim3(LR_BLOCK), 0, ctx->stream, dk, acc, d_ab, nd, (const u32*)keep, fin, fab.as<u32>());
    CKL("k_load_compact");
    ctx->mark("load combine");
    u32 h_kept = 0;
    CK(hipMemcpyAsync(ctx->hist.data(), gh, (size_t)nh * 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(h_rec, rec, sizeof(h_rec), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(&h_kept, keep + nd, 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    ctx->resolve_marks();
    // ---- the record of the load stands where the count's would
    for (int x = 0; x < 4; ++x) ctx->res_w[x] = x < W ? fin.w[x] : nullptr;
    ctx->res_ab = fab.as<u32>();
    ctx->rs.part_mode = false;
    ctx->n_rows = h_kept;
    ctx->stats.n_kmers = h_rec[LR_KMERS]; ctx->stats.n_distinct = nd; ctx->stats.n_solid = h_kept;
    ctx->stats.n_partitions = rows_partitions(ctx);
    ctx->have_result = true;
    st->n_distinct = nd; st->n_rows = h_kept; st->n_below = h_rec[LR_BELOW]; st->n_above = h_rec[LR_ABOVE]; st->n_kmers = h_rec[LR_KMERS];
    st->n_saturated = h_rec[LR_SAT]; st->sorted_input = sorted ? 1 : 0;
    return DSKGPU_OK;
}

}  // namespace

extern "C" int dskgpu_load_rows(dskgpu_ctx* ctx, const void* d_kmers, const void* d_abundance, uint64_t n, uint32_t combine, dskgpu_load_stats* stats) {
    if (!ctx) return DSKGPU_E_ARG;
    if (combine > DSKGPU_LOAD_UNIQUE) return fail(ctx, DSKGPU_E_ARG, "dskgpu_load_rows: combine must be DSKGPU_LOAD_SUM, _MAX, _MIN or _UNIQUE");
    if (n && (!d_kmers || !d_abundance)) return fail(ctx, DSKGPU_E_ARG, "dskgpu_load_rows: null pointer");
    if (n && ((reinterpret_cast<uintptr_t>(d_kmers) & 7) || (reinterpret_cast<uintptr_t>(d_abundance) & 3)))
        return fail(ctx, DSKGPU_E_ARG, "dskgpu_load_rows: d_kmers must be 8-byte aligned and d_abundance 4-byte aligned");
    if (n > 0xFFFFFFFEull) return fail(ctx, DSKGPU_E_ARG, "dskgpu_load_rows: " + std::to_string(n) + " rows: a load takes at most 2^32 - 2 (the limit of the lookup index)");
    if (ctx->cfg.world_size != 1) return fail(ctx, DSKGPU_E_STATE, "dskgpu_load_rows: a rank of a group owns a slice of the k-mer space, and a load knows nothing of it (world_size must be 1)");
    CK(hipSetDevice(ctx->cfg.device));
    dskgpu_load_stats st{};
    st.n_in = n;
    const u64* in = static_cast<const u64*>(d_kmers); const u32* ab = static_cast<const u32*>(d_abundance);
    const int rc = ctx->W == 1 ? load_impl<1>(ctx, in, ab, n, combine, &st) : ctx->W == 2 ? load_impl<2>(ctx, in, ab, n, combine, &st) : load_impl<4>(ctx, in, ab, n, combine, &st);
    if (rc == DSKGPU_OK && stats) *stats = st;
    return rc;
}
