// banks.hip -- the per-bank count (solidity kinds other than sum, 2-D histogram) and the bank ends it works from (dskgpu_ctx::banks,
// engine.h: Banks; kernels: banks.h).  Of the count path it needs one thing, count_reads (dskgpu.hip); the union is ordered by rowsort.hip.
// Multi-bank count: every bank is counted on its own (all distinct k-mers kept), the per-bank rows are
// united and sorted by k-mer, and k_merge_banks applies the solidity kind / builds the histograms.  In steps, so that the
// in-process group (group.hip) can put its own count -- scatter, exchange, mg_count -- between them:
//   banks_begin   the per-bank counts keep every k-mer (abundance window 1 .. max, rows unsorted); the union is empty
//   banks_select  the context's read stream = bank b of the stream it was given (or all of it again: b = ~0u)
//   banks_add     the rows of the count just finished join the union as bank b
//   banks_finish  configuration and read stream restored; union sorted by k-mer, merged -> the result of the context
#include "engine.h"
#include "banks.h"
#include <rocprim/device/device_radix_sort.hpp>

namespace {
// -> ends: the bank ends of the current reads, with the implied last bank: reads behind the last declared end, or no end declared at all
void bank_ends_of(const dskgpu_ctx* ctx, std::vector<u64>& ends) {
    ends = ctx->banks.ends;
    if (ends.empty() || ends.back() < ctx->n_bytes) ends.push_back(ctx->n_bytes);
}
int banks_begin(dskgpu_ctx* ctx) {
    BankJob& j = ctx->banks.job;
    bank_ends_of(ctx, j.ends);
    if (j.ends.size() > 32) return fail(ctx, DSKGPU_E_ARG, "at most 32 banks are supported by the solidity kinds");
    if (ctx->enc_keep) return fail(ctx, DSKGPU_E_STATE, "per-bank counts (-solidity-kind, -histo2D) need the reads themselves: not after dskgpu_encode_reads");
    j.cfg = ctx->cfg; j.base = ctx->d_reads; j.total = ctx->n_bytes;
    j.nu = 0; j.tot_kmers = 0; j.passes = 1; j.retries = 0; j.active = true;
    ctx->cfg.abundance_min = 1; ctx->cfg.abundance_max = 0xFFFFFFFFu; ctx->cfg.flags |= DSKGPU_F_NO_SORT;
    return DSKGPU_OK;
}
void banks_select(dskgpu_ctx* ctx, u32 b) {
    BankJob& j = ctx->banks.job;
    if (!j.active) return;
    if (b >= j.ends.size()) { ctx->d_reads = j.base; ctx->n_bytes = j.total; }
    else { const u64 beg = b ? j.ends[b - 1] : 0; ctx->d_reads = j.base + beg; ctx->n_bytes = j.ends[b] - beg; }
    ctx->enc_fresh = false; ctx->sender.prepared = false;
}
void banks_abort(dskgpu_ctx* ctx) {      // (an error inside a per-bank count: the context gets its configuration and its read stream back)
    BankJob& j = ctx->banks.job;
    if (!j.active) return;
    ctx->cfg = j.cfg; ctx->d_reads = j.base; ctx->n_bytes = j.total; j.active = false;
}
template <int W>
int banks_add(dskgpu_ctx* ctx, u32 b) {
    Banks& B = ctx->banks; BankJob& j = B.job;
    const u64 n = ctx->n_rows, nu = j.nu;
    j.tot_kmers += ctx->stats.n_kmers; j.passes = std::max<u32>(j.passes, (u32)ctx->stats.n_passes); j.retries += ctx->stats.n_retries;
    bool nomem = B.u_val.ensure_keep((nu + n + 1) * 8, nu * 8, ctx->stream) != 0;
    for (int x = 0; x < W; ++x) nomem = nomem || B.u_w[x].ensure_keep((nu + n + 1) * 8, nu * 8, ctx->stream) != 0;
    if (nomem) return fail(ctx, DSKGPU_E_NOMEM, "bank rows");
    if (n) {
        for (int x = 0; x < W; ++x)
            CK(hipMemcpyAsync(B.u_w[x].as<u64>() + nu, ctx->res_w[x], n * 8, hipMemcpyDeviceToDevice, ctx->stream));
        hipLaunchKernelGGL(k_pack_bank, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, B.u_val.as<u64>() + nu, ctx->res_ab, n, b);
        CK(hipStreamSynchronize(ctx->stream));
    }
    j.nu += n;
    return DSKGPU_OK;
}
template <int W>
int banks_finish(dskgpu_ctx* ctx) {
    Banks& B = ctx->banks; BankJob& j = B.job;
    const u32 nbanks = (u32)j.ends.size();
    const u64 nu = j.nu, total = j.total, tot_kmers = j.tot_kmers; const u32 passes = j.passes, retries = j.retries;
    banks_abort(ctx);                          // configuration and read stream back
    ctx->drop_result();
    int rc = DSKGPU_OK;
    if (nu >= 0xFFFF0000ull) return fail(ctx, DSKGPU_E_ARG, "too many distinct k-mers over the banks for the merge");
    // ---- sort the union by k-mer
    CK(B.s_w[0].ensure((nu + 1) * 8)); CK(ctx->s_val.ensure((nu + 1) * 8));
    const unsigned gb = (unsigned)std::max<u64>(1, (nu + 255) / 256);
    if (nu) {
        size_t tmp = 0;
        if (W == 1) {
            const unsigned end_bit = std::min(64u, 2u * ctx->cfg.kmer_size);
            // LIBRARY SORT (rocprim), labelled: bank merges (-solidity-kind other than sum / -histo2D) order (value, bank) pairs once per job -- not on the sum path
            CK(rocprim::radix_sort_pairs(nullptr, tmp, B.u_w[0].as<u64>(), B.s_w[0].as<u64>(), B.u_val.as<u64>(), ctx->s_val.as<u64>(), (size_t)nu, 0u, end_bit, ctx->stream));
            CK(ctx->srt_tmp.ensure(tmp));
            CK(rocprim::radix_sort_pairs(ctx->srt_tmp.p, tmp, B.u_w[0].as<u64>(), B.s_w[0].as<u64>(), B.u_val.as<u64>(), ctx->s_val.as<u64>(), (size_t)nu, 0u, end_bit, ctx->stream));
        } else {
            const u64* rows[4] = {nullptr, nullptr, nullptr, nullptr};
            for (int x = 0; x < W; ++x) rows[x] = B.u_w[x].as<u64>();
            if ((rc = sort_index_multiword(ctx, rows, nu, W))) return rc;
            const u32* idx = ctx->srt_idx.as<u32>();
            for (int x = 0; x < W; ++x) {
                CK(B.s_w[x].ensure((nu + 1) * 8));
                hipLaunchKernelGGL(k_gather<u64>, dim3(gb), dim3(256), 0, ctx->stream, B.s_w[x].as<u64>(), B.u_w[x].as<u64>(), idx, nu);
            }
            CK(ctx->s_val.ensure((nu + 1) * 8));
            hipLaunchKernelGGL(k_gather<u64>, dim3(gb), dim3(256), 0, ctx->stream, ctx->s_val.as<u64>(), B.u_val.as<u64>(), idx, nu);
        }
        CKL("bank sort");
    }
    // ---- merge: solidity + histograms
    const size_t nh = (size_t)ctx->cfg.histo_max + 1;
    CK(B.m_flag.ensure((nu + 2) * 4)); CK(B.m_pos.ensure((nu + 2) * 4)); CK(B.m_sum.ensure((nu + 2) * 4));
    CK(B.gh2d.ensure(nh * 11 * 8));
    CK(hipMemsetAsync(ctx->ghist.p, 0, nh * 8, ctx->stream));
    CK(hipMemsetAsync(B.gh2d.p, 0, nh * 11 * 8, ctx->stream));
    CK(hipMemsetAsync(ctx->gstats.p, 0, 32, ctx->stream));
    MergeParams mp{nbanks, ctx->cfg.solidity_kind, ctx->cfg.solidity_custom, ctx->cfg.abundance_min, ctx->cfg.abundance_max, ctx->cfg.histo_max,
                   (ctx->cfg.flags & DSKGPU_F_HISTO2D) ? 1u : 0u};
    u64 n_solid = 0;
    if (nu) {
        RowsIn ri{}; RowsOut ro{};
        for (int x = 0; x < W; ++x) ri.w[x] = B.s_w[x].as<u64>();
        hipLaunchKernelGGL(k_merge_banks<W>, dim3(gb), dim3(256), 0, ctx->stream, ri,
                           ctx->s_val.as<u64>(), nu, mp, B.m_flag.as<u32>(), B.m_sum.as<u32>(), ctx->ghist.as<u64>(), B.gh2d.as<u64>(), ctx->gstats.as<u64>());
        hipLaunchKernelGGL(k_copy_u32, dim3(gb), dim3(256), 0, ctx->stream, B.m_pos.as<u32>(), B.m_flag.as<u32>(), nu);
        CKL("k_merge_banks");
        ctx->h_sc[SC_F] = (u32)nu;
        CK(hipMemcpyAsync(ctx->scalars.as<u32>() + SC_F, &ctx->h_sc[SC_F], 4, hipMemcpyHostToDevice, ctx->stream));
        if ((rc = run_scan(ctx, B.m_pos.as<u32>(), ctx->scalars.as<u32>() + SC_F, nu))) return rc;
        CK(hipMemcpyAsync(&ctx->h_back[1], B.m_pos.as<u32>() + nu, 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        n_solid = ctx->h_back[1];
        CK(ctx->out_ab.ensure((n_solid + 1) * 4));
        for (int x = 0; x < W; ++x) { CK(ctx->out_w[x].ensure((n_solid + 1) * 8)); ro.w[x] = ctx->out_w[x].as<u64>(); }
        hipLaunchKernelGGL(k_pick_rows<W>, dim3(gb), dim3(256), 0, ctx->stream, ri,
                           B.m_sum.as<u32>(), B.m_flag.as<u32>(), B.m_pos.as<u32>(), nu, ro, ctx->out_ab.as<u32>());
        CKL("k_pick_rows");
    }
    ctx->hist.assign(nh, 0); B.hist2d.assign(nh * 11, 0);
    CK(hipMemcpyAsync(ctx->hist.data(), ctx->ghist.p, nh * 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(B.hist2d.data(), B.gh2d.p, nh * 11 * 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(&ctx->h_stats[0], ctx->gstats.p, 32, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    for (int x = 0; x < 4; ++x) ctx->res_w[x] = x < W ? ctx->out_w[x].as<u64>() : nullptr;
    ctx->res_ab = ctx->out_ab.as<u32>();
    ctx->n_rows = n_solid;
    ctx->stats.n_bytes = total; ctx->stats.n_kmers = tot_kmers; ctx->stats.n_distinct = ctx->h_stats[0]; ctx->stats.n_solid = n_solid;
    ctx->stats.n_passes = passes; ctx->stats.n_retries = retries;
    ctx->stats.n_partitions = ctx->cfg.nb_partitions ? ctx->cfg.nb_partitions : 4u;
    ctx->have_result = true;
    return DSKGPU_OK;
}
int banks_add(dskgpu_ctx* ctx, u32 b) { return ctx->W == 1 ? banks_add<1>(ctx, b) : ctx->W == 2 ? banks_add<2>(ctx, b) : banks_add<4>(ctx, b); }
int banks_finish(dskgpu_ctx* ctx) { return ctx->W == 1 ? banks_finish<1>(ctx) : ctx->W == 2 ? banks_finish<2>(ctx) : banks_finish<4>(ctx); }
}  // namespace

bool per_bank_job(const dskgpu_ctx* ctx) {
    const std::vector<u64>& ends = ctx->banks.ends;
    return (ends.size() > 1 || (!ends.empty() && ends.back() < ctx->n_bytes)) && (ctx->cfg.solidity_kind != DSKGPU_SOLIDITY_SUM || (ctx->cfg.flags & DSKGPU_F_HISTO2D));
}
int run_banks(dskgpu_ctx* ctx) {
    int rc = banks_begin(ctx);
    if (rc) return rc;
    const u32 B = (u32)ctx->banks.job.ends.size();
    for (u32 b = 0; b < B; ++b) {
        banks_select(ctx, b);
        if ((rc = count_reads(ctx)) || (rc = banks_add(ctx, b))) { banks_abort(ctx); return rc; }
    }
    return banks_finish(ctx);
}

// ---- the same steps for group.hip (one library, not part of the C-ABI)
HIDDEN bool dskgpu_i_per_bank(dskgpu_ctx* ctx) { return per_bank_job(ctx); }
HIDDEN uint32_t dskgpu_i_banks(dskgpu_ctx* ctx) { std::vector<u64> ends; bank_ends_of(ctx, ends); return (u32)ends.size(); }
HIDDEN int dskgpu_i_banks_begin(dskgpu_ctx* ctx) { return banks_begin(ctx); }
HIDDEN void dskgpu_i_banks_select(dskgpu_ctx* ctx, uint32_t b) { banks_select(ctx, b); }
HIDDEN void dskgpu_i_banks_abort(dskgpu_ctx* ctx) { banks_abort(ctx); }
HIDDEN int dskgpu_i_banks_add(dskgpu_ctx* ctx, uint32_t b) { return banks_add(ctx, b); }
HIDDEN int dskgpu_i_banks_finish(dskgpu_ctx* ctx) { return banks_finish(ctx); }

extern "C" {
int dskgpu_next_bank(dskgpu_ctx* ctx) {
    if (!ctx) return DSKGPU_E_ARG;
    if (ctx->reads.raw_pending) { CK(hipSetDevice(ctx->cfg.device)); RAW_SYNC(ctx); }
    // (every call ends a bank, an empty one too: a rank of a group that was handed nothing of a small bank must count as many banks as
    //  the others -- until r06 a bank that added no bytes was not recorded: the ranks of `dsk -nb-gpus 4 -solidity-kind min` then ran
    //  different numbers of per-bank steps and waited for each other for ever; on one GPU an empty input file was not a bank at all)
    ctx->banks.ends.push_back(ctx->reads.len);
    return DSKGPU_OK;
}

int dskgpu_set_banks(dskgpu_ctx* ctx, const uint64_t* end_offsets, uint32_t n_banks) {
    if (!ctx || (!end_offsets && n_banks)) return DSKGPU_E_ARG;
    std::vector<u64>& ends = ctx->banks.ends;
    ends.assign(end_offsets, end_offsets + n_banks);
    for (size_t i = 1; i < ends.size(); ++i)
        if (ends[i] < ends[i - 1]) { ends.clear(); return fail(ctx, DSKGPU_E_ARG, "bank end offsets must be non-decreasing"); }
    return DSKGPU_OK;
}

int dskgpu_histogram2d(const dskgpu_ctx* ctx, uint64_t* out, uint32_t nrows) {
    if (!ctx || !out) return DSKGPU_E_ARG;
    if (!ctx->have_result || ctx->banks.hist2d.empty()) return DSKGPU_E_STATE;
    if (nrows != ctx->cfg.histo_max + 1) return DSKGPU_E_ARG;
    std::memcpy(out, ctx->banks.hist2d.data(), ctx->banks.hist2d.size() * 8);
    return DSKGPU_OK;
}
}  // extern "C"
