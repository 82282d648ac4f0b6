// rowsort.hip -- the row order of a count: the solid rows ascending by k-mer value, globally or inside the output partitions of
// DSKGPU_F_PARTITION_ORDER (the reference's Partition<Count> rows, utils/dsk2ascii.cpp:61,77).  One entry point, order_rows, picks
// the path -- hand-written MSD sorts of one-, two- and four-word rows (rowsort.h, rowsort2.h), group by group above RS_MAX_ROWS,
// slab by slab from 2^32 rows, the one-pass partition sort (partsort.h) -- and finishes it: the flag read-back that rides with
// the histogram, another round for listed sub-buckets, the partition -> global retry, the labelled library fallbacks.
#include <cstdio>
#include <vector>

#include "engine.h"
#include "partsort.h"
#include "planning_rowsort.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace {

// the row sort's device scalars (matrix length, two work counters [, the ties flag]) set from KERNEL ARGUMENTS: the sorts are called many
// times back to back from host loops, and an asynchronous copy from one host-side array would only be correct as long as the runtime
// stages pageable copies synchronously
// (z0, z1: two more words to clear -- the sort's "not finished in place" flag and the count of listed sub-buckets -- or null)
__global__ void k_set_rs_scalars(u32* __restrict__ sc4, u32 len, u32 nwords, u32* __restrict__ z0 = nullptr, u32* __restrict__ z1 = nullptr) {
    if (threadIdx.x == 0) sc4[0] = len;
    else if (threadIdx.x < nwords) sc4[threadIdx.x] = 0u;
    if (threadIdx.x == 32 && z0) *z0 = 0u;
    if (threadIdx.x == 33 && z1) *z1 = 0u;
}
// the row sort's two words for the host (its "could not finish in place" flag, the number of listed sub-buckets), put behind the abundance
// histogram so that the end of a step is ONE copy
__global__ void k_sort_back(const u32* __restrict__ sc, const u32* __restrict__ ovs, u64* __restrict__ out) {
    if (threadIdx.x == 0) { out[0] = sc[SC_SORTFLAG]; out[1] = ovs ? ovs[0] : 0u; }
}
#ifndef SORT_TOP_BITS
#define SORT_TOP_BITS 32u      // 4 radix passes; 40 bits (5 passes) cost 0.3 ms more on 43 M rows, the in-place run fix-up absorbs the extra ties
#endif

// a pinned host buffer of at least `need` elements (allocated with `alloc` >= need of them)
template <class T>
int grow_pinned(dskgpu_ctx* ctx, T*& p, size_t& cap, size_t need, size_t alloc) {
    if (cap >= need) return DSKGPU_OK;
    if (p) CK(hipHostFree(p));
    p = nullptr; cap = 0;
    CK(hipHostMalloc(reinterpret_cast<void**>(&p), alloc * sizeof(T), hipHostMallocDefault));
    cap = alloc;
    return DSKGPU_OK;
}

}  // namespace

// most rows the MSD sort takes in one piece (DSKGPU_RS_MAX_ROWS lowers it: tests)
u64 rs_max_rows(const dskgpu_ctx* ctx) { return ctx->tune.rs_max_rows ? std::min<u64>(ctx->tune.rs_max_rows, RS_MAX_ROWS) : RS_MAX_ROWS; }

// Index permutation that sorts n rows of W words (struct-of-arrays in `rows`) ascending: W stable 64-bit
// radix passes, least significant word first.  Result in ctx->srt_idx.
int sort_index_multiword(dskgpu_ctx* ctx, const u64* const* rows, u64 n, int W) {
    CK(ctx->srt_k.ensure(n * 8));
    CK(ctx->srt_idx.ensure(n * 4));
    CK(ctx->srt_idx2.ensure(n * 4));
    DevBuf& keys_sorted = ctx->s_val;           // scratch for the sorted keys of a pass (not needed afterwards)
    CK(keys_sorted.ensure(n * 8));
    const unsigned gb = (unsigned)((n + 255) / 256);
    const unsigned top_bits = std::min(64u, std::max(1u, 2u * ctx->cfg.kmer_size - 64u * (unsigned)(W - 1)));
    u32* idx = ctx->srt_idx.as<u32>(); u32* idx2 = ctx->srt_idx2.as<u32>();
    hipLaunchKernelGGL(k_iota, dim3(gb), dim3(256), 0, ctx->stream, idx, n);
    size_t tmp = 0, tmp2 = 0;
    // LIBRARY SORT (rocprim), labelled FALLBACK: index permutation of multi-word rows in full-width order (W stable passes), behind a raised flag only
    CK(rocprim::radix_sort_pairs(nullptr, tmp, ctx->srt_k.as<u64>(), keys_sorted.as<u64>(), idx, idx2, (size_t)n, 0u, 64u, ctx->stream));
    CK(rocprim::radix_sort_pairs(nullptr, tmp2, ctx->srt_k.as<u64>(), keys_sorted.as<u64>(), idx, idx2, (size_t)n, 0u, top_bits, ctx->stream));
    CK(ctx->srt_tmp.ensure(std::max(tmp, tmp2)));
    for (int x = 0; x < W; ++x) {
        const u64* src = rows[x];
        const unsigned bits = x == W - 1 ? top_bits : 64u;
        if (x == 0) {
            CK(rocprim::radix_sort_pairs(ctx->srt_tmp.p, tmp, src, keys_sorted.as<u64>(), idx, idx2, (size_t)n, 0u, bits, ctx->stream));
        } else {
            hipLaunchKernelGGL(k_gather<u64>, dim3(gb), dim3(256), 0, ctx->stream, ctx->srt_k.as<u64>(), src, idx, n);
            size_t t = x == W - 1 ? tmp2 : tmp;
            CK(rocprim::radix_sort_pairs(ctx->srt_tmp.p, t, ctx->srt_k.as<u64>(), keys_sorted.as<u64>(), idx, idx2, (size_t)n, 0u, bits, ctx->stream));
        }
        std::swap(idx, idx2);
    }
    if (idx != ctx->srt_idx.as<u32>()) std::swap(ctx->srt_idx, ctx->srt_idx2);
    CKL("sort_index_multiword");
    return DSKGPU_OK;
}

namespace {

// full-width order of multi-word rows: W stable radix passes over an index permutation, then gathers
int sort_rows_full_multiword(dskgpu_ctx* ctx, u64 n) {
    const int W = ctx->W;
    const u64* rows[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int x = 0; x < W; ++x) rows[x] = ctx->out_w[x].as<u64>();
    int rc = sort_index_multiword(ctx, rows, n, W);
    if (rc) return rc;
    const unsigned gb = (unsigned)((n + 255) / 256);
    const u32* idx = ctx->srt_idx.as<u32>();
    CK(ctx->srt_ab.ensure(n * 4));
    for (int x = 0; x < W; ++x) {
        CK(ctx->srt_w[x].ensure(n * 8));
        hipLaunchKernelGGL(k_gather<u64>, dim3(gb), dim3(256), 0, ctx->stream, ctx->srt_w[x].as<u64>(), ctx->out_w[x].as<u64>(), idx, n);
        ctx->res_w[x] = ctx->srt_w[x].as<u64>();
    }
    hipLaunchKernelGGL(k_gather<u32>, dim3(gb), dim3(256), 0, ctx->stream, ctx->srt_ab.as<u32>(), ctx->out_ab.as<u32>(), idx, n);
    CKL("sort_rows");
    ctx->res_ab = ctx->srt_ab.as<u32>();
    return DSKGPU_OK;
}

// (step_a_chunks, step_a_chunks_sparse: planning_rowsort.h)

// the fewest top bits of the first digit (bA bits; bucket b = [start[b], start[b + 1])) whose groups of buckets hold <= rs_max rows
// each; -1 when one bucket alone holds more
template <class T>
int group_bits(const std::vector<T>& start, int bA, u64 rs_max) {
    for (int bits = 0; bits <= bA; ++bits) {
        const u32 per = (1u << bA) >> bits;
        bool ok = true;
        for (u32 g0 = 0; g0 < (1u << bA) && ok; g0 += per) ok = (u64)start[g0 + per] - start[g0] <= rs_max;
        if (ok) return bits;
    }
    return -1;
}

// What the first round of a row sort leaves for order_rows to finish
struct Round {
    int back = 0;             // what k_sort_back reads back with the histogram: 1 = the flag + the listed count, 2 = the flag only; 0 = the sort
                              // copied them to rs.flag / rs.listed itself (valid after order_rows' synchronisation)
    bool partial = false;     // ordered by the hand-written kernels: listed sub-buckets and the full-width fallback may still apply
    u64* k = nullptr; u32* v = nullptr;      // one-word rows: where the result lies (sort_oversize)
    Rows2 scratch{};          // two-word rows ordered in the scratch copy: copied back to out_* before the fallback
};

// ---- hand-written MSD radix sort (rowsort.h) of n (64-bit key, 32-bit value) pairs on the `total` low bits of the key, in place
// (tk / tv: scratch of the same size).  One-word rows: (k-mer value, abundance); multi-word rows: (top 63 bits of the value,
// row index).  Whatever the kernels do not order themselves raises SC_SORTFLAG (zeroed here): the caller falls back to a
// full-width library sort (k / v and tk / tv each hold a complete permutation of the pairs either way).
int msd_sort_pairs(dskgpu_ctx* ctx, u64* k, u32* v, u64* tk, u32* tv, u64 n, int total, bool reset_flags = true, u32 base = 0, const SparseRows* spr = nullptr) {
    // second digit: 8 bits up to 96 M rows, 9 up to 192 M, 10 beyond (sub-buckets stay near 200 rows: one wave each in step C)
    int wantB = n <= (96ull << 20) ? 8 : n <= (192ull << 20) ? 9 : 10;
    if (ctx->tune.rs_bbits >= 8 && ctx->tune.rs_bbits <= 10) wantB = (int)ctx->tune.rs_bbits;      // tests
    const int bA = std::min(RS_ABITS, total), r1 = total - bA, bB = std::min(wantB, r1), r2 = r1 - bB, bC = std::min(8, r2), r3 = r2 - bC;
    const u32 BB = 1u << wantB;
    RsSpec sp{r1, r2, r3, (1u << bA) - 1u, (1u << bB) - 1u, (1u << bC) - 1u};
    const u64 ncu = (u64)ctx->num_cu;
    u64 chunk, nch = step_a_chunks(n, ncu, RS_TILE, &chunk);
    RsSparse sps{}; u64 nch_sp = 0;
    if (spr) { u32 qpc; nch = step_a_chunks_sparse(spr->F, spr->n_sparse, spr->n_tail, ncu, &qpc, &nch_sp, &chunk); sps = spr->as<RsSparse>(qpc); }
    const u64 M = (u64)RS_ABINS * nch;
    if (M >= 0xFFFFFFF0ull) return fail(ctx, DSKGPU_E_ARG, "row sort: chunk matrix too large");
    const u64 nsubw = (u64)RS_ABINS * (BB + 1);                           // sub-bucket starts; behind them the list of large sub-buckets
    CK(ctx->srt_tmp.ensure((M + 2 + 2 * nsubw + 16) * 4));
    u32* matrix = static_cast<u32*>(ctx->srt_tmp.p);
    u32* sub = matrix + M + 2;
    u32* biglist = sub + nsubw;
    u32* sc = ctx->scalars.as<u32>();
    CK(ctx->rs.ovs.ensure((1 + 3 * RS_OVS_CAP) * 4));
    hipLaunchKernelGGL(k_set_rs_scalars, dim3(1), dim3(64), 0, ctx->stream, sc + SC_RSLEN, (u32)M, reset_flags ? 4u : 3u,      // (length, two work counters [, ties seen])
                       reset_flags ? sc + SC_SORTFLAG : (u32*)nullptr, reset_flags ? ctx->rs.ovs.as<u32>() : (u32*)nullptr);
    const size_t ldsA = RsLds<RS_ABINS, RS_TILE>::bytes;
    const size_t ldsB = BB == 256 ? RsLds<256, RS_BTILE>::bytes : BB == 512 ? RsLds<512, RS_BTILE>::bytes : RsLds<1024, RS_BTILE>::bytes;
    { const int e = allow_big_lds(ctx, reinterpret_cast<const void*>(&k_rs_scatter<false>)); if (e) return e; }
    if (spr) {
        const size_t ldsS = ldsA + ((size_t)RS_SP_MAXQ + 1) * 4;
        { const int e = allow_big_lds(ctx, reinterpret_cast<const void*>(&k_rs_scatter_sp)); if (e) return e; }
        hipLaunchKernelGGL(k_rs_hist_sp, dim3((unsigned)nch_sp), dim3(RS_NT), 0, ctx->stream, sps, (u32)nch, matrix, sp);
        if (spr->n_tail) hipLaunchKernelGGL(k_rs_hist, dim3(1), dim3(RS_NT), 0, ctx->stream, spr->tail_w.w[0], (u64)spr->n_tail, (u32)chunk, (u32)nch, matrix, sp, (u32)nch_sp);
        CKL("k_rs_hist_sp");
        { const int e = run_scan(ctx, matrix, sc + SC_RSLEN, M); if (e) return e; }
        hipLaunchKernelGGL(k_rs_scatter_sp, dim3((unsigned)nch_sp), dim3(RS_NT), ldsS, ctx->stream, sps, (u32)nch, (const u32*)matrix, tk, tv, sp);
        if (spr->n_tail) hipLaunchKernelGGL(k_rs_scatter<false>, dim3(1), dim3(RS_NT), ldsA, ctx->stream, spr->tail_w.w[0], spr->tail_ab, (u64)spr->n_tail, (u32)chunk, (u32)nch, (const u32*)matrix, tk, tv, sp, (const u64*)nullptr, (u32)nch_sp);
        CKL("k_rs_scatter_sp");
    } else {
        hipLaunchKernelGGL(k_rs_hist, dim3((unsigned)nch), dim3(RS_NT), 0, ctx->stream, k, n, (u32)chunk, (u32)nch, matrix, sp, 0u);
        CKL("k_rs_hist");
        { const int e = run_scan(ctx, matrix, sc + SC_RSLEN, M); if (e) return e; }
        hipLaunchKernelGGL(k_rs_scatter<false>, dim3((unsigned)nch), dim3(RS_NT), ldsA, ctx->stream, k, v, n, (u32)chunk, (u32)nch, matrix, tk, tv, sp, (const u64*)nullptr, 0u);
        CKL("k_rs_scatter");
    }
    // a bucket above 64 x the mean (+ 256 K rows) is not a k-mer spectrum any more (canonical k-mers: at most ~2 x; a low-complexity stretch of
    // 200 kb puts 180 K rows under AAAAA: that is still one block's 0.2 ms -- the limit was 16 x + 64 K until seeds 208 / 292 / 319 of
    // tools/stress_random.py took the 12 ms library fallback for it): one block would
    // walk it alone, so it goes to the full-width fallback instead
    u32 heavy = (u32)std::min<u64>(0xFFFFFFFFull, n / RS_ABINS * 64 + 262144);
    if (ctx->tune.rs_heavy) heavy = ctx->tune.rs_heavy;
    const unsigned gridB = (unsigned)std::min<u64>(ncu * (160 * 1024 / (ldsB + 1024)), RS_ABINS);
    auto split = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(gridB), dim3(RS_BNT), ldsB, ctx->stream, tk, tv, (u32)nch, matrix, k, v, sub, sp, sc + SC_RSWORK2, heavy, sc + SC_SORTFLAG);
    };
    if (BB == 1024 && ldsB > 64 * 1024) { const int e = allow_big_lds(ctx, reinterpret_cast<const void*>(&k_rs_split<1024>)); if (e) return e; }
    if (BB == 256) split(k_rs_split<256>); else if (BB == 512) split(k_rs_split<512>); else split(k_rs_split<1024>);
    CKL("k_rs_split");
    const u32 nsub = RS_ABINS * BB;
    hipLaunchKernelGGL(k_rs_cells, dim3(nsub / (RS_CNT / 64)), dim3(RS_CNT), 0, ctx->stream, k, v, sub, nsub, BB, sp, biglist, sc + SC_RSWORK, sc + SC_SORTFLAG, sc + SC_RSTIES);
    CKL("k_rs_cells");
    const u32 block_rows = ctx->tune.rs_block_rows ? std::min<u32>(ctx->tune.rs_block_rows, RS_BLOCK_ROWS) : RS_BLOCK_ROWS;
    hipLaunchKernelGGL(k_rs_big, dim3((unsigned)std::min<u64>(ncu, 256)), dim3(RS_NT), 0, ctx->stream, k, v, sub, sp, biglist, sc + SC_RSWORK, sc + SC_SORTFLAG, block_rows, sc + SC_RSTIES, base, ctx->rs.ovs.as<u32>());
    CKL("k_rs_big");
    return DSKGPU_OK;
}

// ---- the same sort for two-word rows (rowsort2.h): the rows themselves -- (hi, lo, abundance) in three arrays -- ordered in place on
// the `total` low bits of hi:lo (t: scratch of the same size).  What it lists (sub-buckets above RS_BLOCK_ROWS rows) is left in
// ctx->rs.ovs for the caller's next round; a heavy first-digit bucket or a full list raises SC_SORTFLAG.  k holds a complete
// permutation of the rows either way.
// spr: step A reads the rows in the count kernel's regions (+ a dense tail: the rows of the k-mers counted apart), as in msd_sort_pairs
int msd_sort_rows2(dskgpu_ctx* ctx, Rows2 k, Rows2 t, u64 n, int total, bool reset_flags, u32 base, const SparseRows* spr = nullptr) {
    int wantB = n <= (96ull << 20) ? 8 : n <= (192ull << 20) ? 9 : 10;
    if (ctx->tune.rs_bbits >= 8 && ctx->tune.rs_bbits <= 10) wantB = (int)ctx->tune.rs_bbits;      // tests
    const int bA = std::min(RS2_ABITS, total), r1 = total - bA, bB = std::min(wantB, r1), r2 = r1 - bB, bC = std::min(8, r2), r3 = r2 - bC;
    const u32 BB = 1u << wantB;
    RsSpec sp{r1, r2, r3, (1u << bA) - 1u, (1u << bB) - 1u, (1u << bC) - 1u};
    const u64 ncu = (u64)ctx->num_cu;
    u64 chunk, nch = step_a_chunks(n, ncu, RS2_TILE, &chunk);
    Rs2Sparse sps{}; u64 nch_sp = 0;
    if (spr) { u32 qpc; nch = step_a_chunks_sparse(spr->F, spr->n_sparse, spr->n_tail, ncu, &qpc, &nch_sp, &chunk); sps = spr->as<Rs2Sparse>(qpc); }
    const u64 M = (u64)RS2_ABINS * nch;
    const u64 nsubw = (u64)RS2_ABINS * (BB + 1);
    CK(ctx->srt_tmp.ensure((M + 2 + 2 * nsubw + 16) * 4));
    u32* matrix = static_cast<u32*>(ctx->srt_tmp.p);
    u32* sub = matrix + M + 2;
    u32* biglist = sub + nsubw;
    u32* sc = ctx->scalars.as<u32>();
    CK(ctx->rs.ovs.ensure((1 + 3 * RS_OVS_CAP) * 4));
    hipLaunchKernelGGL(k_set_rs_scalars, dim3(1), dim3(64), 0, ctx->stream, sc + SC_RSLEN, (u32)M, reset_flags ? 4u : 3u,
                       reset_flags ? sc + SC_SORTFLAG : (u32*)nullptr, reset_flags ? ctx->rs.ovs.as<u32>() : (u32*)nullptr);
    const size_t ldsA = Rs2Lds<RS2_ABINS, RS2_TILE>::bytes;
    const size_t ldsB = BB == 256 ? Rs2Lds<256, RS2_BTILE>::bytes : BB == 512 ? Rs2Lds<512, RS2_BTILE>::bytes : Rs2Lds<1024, RS2_BTILE>::bytes;
    const size_t ldsBig = (size_t)RS_BLOCK_ROWS * 20 + 2 * RS_CELLS * 4;
    { const int e = allow_big_lds(ctx, reinterpret_cast<const void*>(&k2_scatter<false>)); if (e) return e; }
    { const int e = allow_big_lds(ctx, reinterpret_cast<const void*>(&k2_big), (int)ldsBig); if (e) return e; }
    const Rows2C kc{k.hi, k.lo, k.ab}, tc{t.hi, t.lo, t.ab};
    if (spr) {
        const size_t ldsS = ldsA + ((size_t)RS_SP_MAXQ + 1) * 4;
        { const int e = allow_big_lds(ctx, reinterpret_cast<const void*>(&k2_scatter_sp)); if (e) return e; }
        hipLaunchKernelGGL(k2_hist_sp, dim3((unsigned)nch_sp), dim3(RS_NT), 0, ctx->stream, sps, (u32)nch, matrix, sp);
        if (spr->n_tail) hipLaunchKernelGGL(k2_hist, dim3(1), dim3(RS_NT), 0, ctx->stream, spr->tail2(), (u64)spr->n_tail, (u32)chunk, (u32)nch, matrix, sp, (u32)nch_sp);
        CKL("k2_hist_sp");
        { const int e = run_scan(ctx, matrix, sc + SC_RSLEN, M); if (e) return e; }
        hipLaunchKernelGGL(k2_scatter_sp, dim3((unsigned)nch_sp), dim3(RS_NT), ldsS, ctx->stream, sps, (u32)nch, (const u32*)matrix, t, sp);
        if (spr->n_tail) hipLaunchKernelGGL(k2_scatter<false>, dim3(1), dim3(RS_NT), ldsA, ctx->stream, spr->tail2(), (u64)spr->n_tail, (u32)chunk, (u32)nch, matrix, t, sp, (const u64*)nullptr, (u32)nch_sp);
        CKL("k2_scatter_sp");
    } else {
        hipLaunchKernelGGL(k2_hist, dim3((unsigned)nch), dim3(RS_NT), 0, ctx->stream, kc, n, (u32)chunk, (u32)nch, matrix, sp, 0u);
        CKL("k2_hist");
        { const int e = run_scan(ctx, matrix, sc + SC_RSLEN, M); if (e) return e; }
        hipLaunchKernelGGL(k2_scatter<false>, dim3((unsigned)nch), dim3(RS_NT), ldsA, ctx->stream, kc, n, (u32)chunk, (u32)nch, matrix, t, sp, (const u64*)nullptr, 0u);
        CKL("k2_scatter");
    }
    u32 heavy = (u32)std::min<u64>(0xFFFFFFFFull, n / RS2_ABINS * 64 + 262144);
    if (ctx->tune.rs_heavy) heavy = ctx->tune.rs_heavy;
    const unsigned gridB = (unsigned)std::min<u64>(ncu * (160 * 1024 / (ldsB + 1024)), RS2_ABINS);
    auto split = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(gridB), dim3(RS_BNT), ldsB, ctx->stream, tc, (u32)nch, matrix, k, sub, sp, sc + SC_RSWORK2, heavy, sc + SC_SORTFLAG);
    };
    if (BB == 256) split(k2_split<256>); else if (BB == 512) split(k2_split<512>); else split(k2_split<1024>);
    CKL("k2_split");
    const u32 nsub = RS2_ABINS * BB;
    hipLaunchKernelGGL(k2_cells, dim3(nsub / (RS_CNT / 64)), dim3(RS_CNT), 0, ctx->stream, k, sub, nsub, BB, sp, biglist, sc + SC_RSWORK);
    CKL("k2_cells");
    const u32 block_rows = ctx->tune.rs_block_rows ? std::min<u32>(ctx->tune.rs_block_rows, RS_BLOCK_ROWS) : RS_BLOCK_ROWS;
    hipLaunchKernelGGL(k2_big, dim3((unsigned)std::min<u64>(ncu, 256)), dim3(RS_NT), ldsBig, ctx->stream, k, sub, sp, biglist, sc + SC_RSWORK, sc + SC_SORTFLAG, block_rows, base, ctx->rs.ovs.as<u32>());
    CKL("k2_big");
    return DSKGPU_OK;
}

// the sub-buckets a two-word sort listed (ctx->rs.ovs; offsets are absolute rows of R, the array that holds the result; S = scratch of
// the same shape): every listed range goes round again on the bits it has not used, until nothing is listed any more
int rows2_rounds(dskgpu_ctx* ctx, Rows2 R, Rows2 S) {
    u32* sc = ctx->scalars.as<u32>();
    std::vector<u32> list;
    for (int round = 0; ; ++round) {
        u32 cnt = 0;
        CK(hipMemcpyAsync(&ctx->rs.flag, sc + SC_SORTFLAG, 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipMemcpyAsync(&cnt, ctx->rs.ovs.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        if (ctx->rs.flag || cnt == 0) break;
        if (cnt > RS2_OVS_CAP || round >= 8) { ctx->rs.flag = 1; CK(hipMemsetAsync(sc + SC_SORTFLAG, 0xFF, 4, ctx->stream)); break; }
        list.resize(3 * (size_t)cnt);
        CK(hipMemcpyAsync(list.data(), ctx->rs.ovs.as<u32>() + 1, list.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        CK(hipMemsetAsync(ctx->rs.ovs.p, 0, 4, ctx->stream));
        if (ctx->tune.verbose) fprintf(stderr, "[dskgpu] two-word row sort, round %d: %u sub-bucket(s) above %u rows go round again (first: %u rows, %u bits left)\n", round + 1, cnt, (u32)RS_BLOCK_ROWS, list[1], list[2]);
        for (u32 r = 0; r < cnt; ++r) {
            const u64 off = list[3 * r]; const u32 len = list[3 * r + 1], bits = list[3 * r + 2];
            const Rows2 k2{R.hi + off, R.lo + off, R.ab + off}, t2{S.hi + off, S.lo + off, S.ab + off};
            const int e = msd_sort_rows2(ctx, k2, t2, len, (int)bits, false, (u32)off);
            if (e) return e;
        }
    }
    return DSKGPU_OK;
}

// two-word rows, <= RS_MAX_ROWS: out_* ordered in place; the sub-buckets the sort lists go round again on their remaining bits,
// range by range (a handful on real reads; each round consumes 26-28 bits: at most ceil(128 / 18) rounds).  Leaves the flag
// read-back to order_rows like the other sorts (the full-width fallback reads out_*).  spr: the rows are still sparse (step A reads them there)
int sort_rows2_msd(dskgpu_ctx* ctx, u64 n, Round* r, const SparseRows* spr = nullptr) {
    for (int x = 0; x < 2; ++x) CK(ctx->srt_w[x].ensure(n * 8));
    CK(ctx->srt_ab.ensure(n * 4));
    const Rows2 K{ctx->out_w[1].as<u64>(), ctx->out_w[0].as<u64>(), ctx->out_ab.as<u32>()};
    const Rows2 T{ctx->srt_w[1].as<u64>(), ctx->srt_w[0].as<u64>(), ctx->srt_ab.as<u32>()};
    { const int e = msd_sort_rows2(ctx, K, T, n, 2 * (int)ctx->cfg.kmer_size, true, 0u, spr); if (e) return e; }
    { const int e = rows2_rounds(ctx, K, T); if (e) return e; }
    r->back = 2; r->partial = true;
    return DSKGPU_OK;
}

// two-word row sets above RS_MAX_ROWS (all of configs[3]'s volume on one GPU: 7 * 10^8 rows): sort_rows_big's scheme with the
// rowsort2.h kernels -- step A once over all rows (out_* -> scratch), then the groups of 10-bit buckets that share their top `sb` bits
// are ordered one by one (in the scratch copy, out_* their scratch), then the listed sub-buckets' rounds.  Result: ctx->res_* = the
// scratch copy; on a raised flag order_rows copies it back to out_* for the full-width fallback (r->scratch).
int sort_rows2_big(dskgpu_ctx* ctx, u64 n, Round* r) {
    const Rows2 K{ctx->out_w[1].as<u64>(), ctx->out_w[0].as<u64>(), ctx->out_ab.as<u32>()};
    const size_t n_al = (size_t)((n + 31) & ~(u64)31), need = n_al * 20 + 256;
    Rows2 T;
    if (ctx->l0buf.cap >= need) { T.hi = ctx->l0buf.as<u64>(); T.lo = T.hi + n_al; T.ab = reinterpret_cast<u32*>(T.lo + n_al); }
    else {
        size_t free_b = 0, total_b = 0;
        CK(hipMemGetInfo(&free_b, &total_b));
        if (ctx->srt_w[0].cap + ctx->srt_w[1].cap + ctx->srt_ab.cap + free_b < need + ((size_t)2 << 30)) { ctx->l0buf.release(); ctx->bufA.release(); ctx->bufB.release(); }
        for (int x = 0; x < 2; ++x) CK(ctx->srt_w[x].ensure(n * 8));
        CK(ctx->srt_ab.ensure(n * 4));
        T = Rows2{ctx->srt_w[1].as<u64>(), ctx->srt_w[0].as<u64>(), ctx->srt_ab.as<u32>()};
    }
    const int total = 2 * (int)ctx->cfg.kmer_size;
    const int bA = std::min(RS2_ABITS, total);
    RsSpec sp{total - bA, 0, 0, (1u << bA) - 1u, 0u, 0u};
    const u64 ncu = (u64)ctx->num_cu;
    u64 chunk; const u64 nch = step_a_chunks(n, ncu, 0, &chunk);
    const u64 M = (u64)RS2_ABINS * nch;
    if (M >= 0xFFFFFFF0ull) return fail(ctx, DSKGPU_E_ARG, "row sort: too many rows");
    CK(ctx->mat2.ensure((M + 2) * 4));
    u32* matrix = ctx->mat2.as<u32>();
    u32* sc = ctx->scalars.as<u32>();
    CK(ctx->rs.ovs.ensure((1 + 3 * RS_OVS_CAP) * 4));
    hipLaunchKernelGGL(k_set_rs_scalars, dim3(1), dim3(64), 0, ctx->stream, sc + SC_RSLEN, (u32)M, 4u, sc + SC_SORTFLAG, ctx->rs.ovs.as<u32>());
    ctx->rs.listed = 0;
    { const int e = allow_big_lds(ctx, reinterpret_cast<const void*>(&k2_scatter<false>)); if (e) return e; }
    const Rows2C kc{K.hi, K.lo, K.ab};
    hipLaunchKernelGGL(k2_hist, dim3((unsigned)nch), dim3(RS_NT), 0, ctx->stream, kc, n, (u32)chunk, (u32)nch, matrix, sp);
    CKL("k2_hist");
    { const int e = run_scan(ctx, matrix, sc + SC_RSLEN, M); if (e) return e; }
    const size_t ldsA = Rs2Lds<RS2_ABINS, RS2_TILE>::bytes;
    hipLaunchKernelGGL(k2_scatter<false>, dim3((unsigned)nch), dim3(RS_NT), ldsA, ctx->stream, kc, n, (u32)chunk, (u32)nch, matrix, T, sp, (const u64*)nullptr);
    CKL("k2_scatter");
    std::vector<u32> start(RS2_ABINS + 1);
    CK(hipMemcpy2DAsync(start.data(), 4, matrix, nch * 4, 4, RS2_ABINS + 1, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    start[RS2_ABINS] = (u32)n;
    const u64 rs_max = rs_max_rows(ctx);
    const int sb = group_bits(start, bA, rs_max);
    ctx->res_w[1] = T.hi; ctx->res_w[0] = T.lo; ctx->res_ab = T.ab;
    r->partial = true; r->scratch = T;
    if (sb < 0) { ctx->rs.flag = 1; return DSKGPU_OK; }
    const u32 per = (1u << bA) >> sb;
    for (u32 g0 = 0; g0 < (1u << bA); g0 += per) {
        const u64 b = start[g0], e = start[g0 + per];
        if (e - b < 2 || total - sb < 1) continue;
        const Rows2 r2{T.hi + b, T.lo + b, T.ab + b}, s2{K.hi + b, K.lo + b, K.ab + b};
        const int rc = msd_sort_rows2(ctx, r2, s2, e - b, total - sb, false, (u32)b);
        if (rc) return rc;
    }
    { const int e = rows2_rounds(ctx, T, K); if (e) return e; }
    CK(hipMemcpyAsync(&ctx->rs.flag, sc + SC_SORTFLAG, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (ctx->tune.verbose) fprintf(stderr, "[dskgpu] two-word row sort: %llu rows in %u groups on their top %d bits, MSD sort per group\n", (unsigned long long)n, 1u << sb, sb);
    return DSKGPU_OK;
}

// one-word rows: out_* ordered in place (srt_* = scratch and, for the fallback, a complete permutation of the rows).  spr: as above
int sort_rows_msd(dskgpu_ctx* ctx, u64 n, Round* r, const SparseRows* spr = nullptr) {
    CK(ctx->srt_w[0].ensure(n * 8)); CK(ctx->srt_ab.ensure(n * 4));
    const int e = msd_sort_pairs(ctx, ctx->out_w[0].as<u64>(), ctx->out_ab.as<u32>(), ctx->srt_w[0].as<u64>(), ctx->srt_ab.as<u32>(), n,
                                 (int)std::min(64u, 2u * ctx->cfg.kmer_size), true, 0u, spr);
    if (e) return e;
    r->back = 1; r->partial = true;      // (flag and sub-bucket count travel with the histogram)
    r->k = ctx->out_w[0].as<u64>(); r->v = ctx->out_ab.as<u32>();
    ctx->res_w[0] = r->k; ctx->res_ab = r->v;
    return DSKGPU_OK;
}

// The sub-buckets a row sort listed instead of ordering them (k_rs_big: more than RS_BLOCK_ROWS rows share two digits -- the error
// variants of a k-mer with 10^8 occurrences share 13 and more leading bases): the rows of all listed ranges are gathered under
// the composite key (range number, value bits the range has not used yet), ordered by ONE more MSD sort and put back
// (k_ovs_gather / k_ovs_scatter) -- which may list ranges of the gathered array again: a few rounds at most, the rows of a range
// share ever longer prefixes.  Called after the host has seen a non-zero count (ctx->rs.listed); synchronous.  Leaves
// ctx->rs.flag != 0 when rounds or list run out: the caller's full-width fallback.
int sort_oversize(dskgpu_ctx* ctx, u64* res_k, u32* res_v, int depth = 0) {
    u32* sc = ctx->scalars.as<u32>();
    const u32 cnt = ctx->rs.listed;
    if (cnt == 0) return DSKGPU_OK;
    if (cnt > RS_OVS_CAP || depth >= 4) { ctx->rs.flag = 1; return DSKGPU_OK; }
    std::vector<u32> list(3 * (size_t)cnt), starts(cnt + 1, 0);
    CK(hipMemcpyAsync(list.data(), ctx->rs.ovs.as<u32>() + 1, list.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    u64 tot = 0; u32 maxbits = 1;
    for (u32 i = 0; i < cnt; ++i) { starts[i] = (u32)tot; tot += list[3 * i + 1]; maxbits = std::max(maxbits, list[3 * i + 2]); }
    if (tot >= 0xFFFF0000ull || maxbits > RS_OVS_SHIFT) { ctx->rs.flag = 1; return DSKGPU_OK; }
    if (ctx->tune.verbose) fprintf(stderr, "[dskgpu] row sort: %u sub-bucket(s) above %u rows (%llu rows in all, up to %u bits left) go round again\n", cnt, (u32)RS_BLOCK_ROWS, (unsigned long long)tot, maxbits);
    DevBuf& g = ctx->rs.g[depth];
    const size_t n_al = (size_t)((tot + 31) & ~(u64)31);
    const size_t meta = ((size_t)cnt * 4 * 4 + (size_t)cnt * 8 + 255) & ~size_t(255);      // list (3 words) + starts, then the prefixes
    CK(g.ensure(2 * n_al * 12 + meta + 256));
    u64* gk = g.as<u64>(); u64* tk = gk + n_al; u32* gv = reinterpret_cast<u32*>(tk + n_al); u32* tv = gv + n_al;
    u32* d_list = tv + n_al; u32* d_starts = d_list + 3 * (size_t)cnt;
    u64* d_prefix = reinterpret_cast<u64*>(reinterpret_cast<char*>(d_list) + (((size_t)cnt * 16 + 7) & ~size_t(7)));
    CK(hipMemcpyAsync(d_list, list.data(), list.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    CK(hipMemcpyAsync(d_starts, starts.data(), (size_t)cnt * 4, hipMemcpyHostToDevice, ctx->stream));
    const unsigned gridr = (unsigned)std::min<u64>(cnt, (u64)ctx->num_cu * 8);
    hipLaunchKernelGGL(k_ovs_gather, dim3(gridr), dim3(256), 0, ctx->stream, (const u64*)res_k, (const u32*)res_v, (const u32*)d_list, (const u32*)d_starts, cnt, gk, gv, d_prefix, maxbits);
    CKL("k_ovs_gather");
    CK(hipStreamSynchronize(ctx->stream));          // (list / starts were read from host vectors)
    CK(hipMemsetAsync(ctx->rs.ovs.p, 0, 4, ctx->stream));
    int idbits = 1; while ((1u << idbits) < cnt) ++idbits;
    { const int rc = msd_sort_pairs(ctx, gk, gv, tk, tv, tot, (int)maxbits + idbits, false, 0u); if (rc) return rc; }
    ctx->rs.listed = 0;
    CK(hipMemcpyAsync(&ctx->rs.listed, ctx->rs.ovs.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(&ctx->rs.flag, sc + SC_SORTFLAG, 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    if (!ctx->rs.flag && ctx->rs.listed) { const int rc = sort_oversize(ctx, gk, gv, depth + 1); if (rc) return rc; }
    if (ctx->rs.flag) return DSKGPU_OK;
    hipLaunchKernelGGL(k_ovs_scatter, dim3(gridr), dim3(256), 0, ctx->stream, res_k, res_v, (const u32*)d_list, (const u32*)d_starts, cnt, (const u64*)gk, (const u32*)gv, (const u64*)d_prefix, maxbits);
    CKL("k_ovs_scatter");
    return DSKGPU_OK;
}

// Row sets above RS_MAX_ROWS (one-word rows; the 3 * 10^9 solid k-mers of a 30x human run, the 6 * 10^8 of 200 M reads): step A of
// the MSD sort ONCE over all rows -- 1024 buckets on the top 10 value bits, exact offsets (rows < 2^32) -- then the rows that
// share their top `sb` bits (sb = the fewest bits for which every such group holds <= RS_MAX_ROWS rows: 3-5 for those inputs)
// are ordered group by group with the MSD sort on the remaining bits.  No library kernel; what the MSD kernels do not order
// themselves raises the same flag as for small row sets (full-width fallback in run_pipeline).  Scratch for the second copy of
// the rows: the level-0 buffer of a multi-pass count when it is large enough (its key arrays are dead by now), else srt_* --
// after giving back the partition buffers when HBM is short (the next count allocates them again).
// In: rows in out_w[0] / out_ab.  Out: ctx->res_* = r->k / r->v (the scratch copy, a permutation of the rows for the fallback).
int sort_rows_big(dskgpu_ctx* ctx, u64 n, Round* r) {
    u64* k = ctx->out_w[0].as<u64>(); u32* v = ctx->out_ab.as<u32>();
    const size_t n_al = (size_t)((n + 31) & ~(u64)31), need = n_al * 12 + 256;
    u64* tk; u32* tv;
    if (ctx->l0buf.cap >= need) { tk = ctx->l0buf.as<u64>(); tv = reinterpret_cast<u32*>(tk + n_al); }
    else {
        size_t free_b = 0, total_b = 0;
        CK(hipMemGetInfo(&free_b, &total_b));
        if (ctx->srt_w[0].cap + ctx->srt_ab.cap + free_b < need + ((size_t)2 << 30)) { ctx->l0buf.release(); ctx->bufA.release(); ctx->bufB.release(); }
        CK(ctx->srt_w[0].ensure(n * 8)); CK(ctx->srt_ab.ensure(n * 4));
        tk = ctx->srt_w[0].as<u64>(); tv = ctx->srt_ab.as<u32>();
    }
    const int total = (int)std::min(64u, 2u * ctx->cfg.kmer_size);
    const int bA = std::min(RS_ABITS, total);
    RsSpec sp{total - bA, 0, 0, (1u << bA) - 1u, 0u, 0u};
    const u64 ncu = (u64)ctx->num_cu;
    u64 chunk; const u64 nch = step_a_chunks(n, ncu, 0, &chunk);
    const u64 M = (u64)RS_ABINS * nch;
    if (M >= 0xFFFFFFF0ull) return fail(ctx, DSKGPU_E_ARG, "row sort: too many rows");
    CK(ctx->mat2.ensure((M + 2) * 4));
    u32* matrix = ctx->mat2.as<u32>();
    u32* sc = ctx->scalars.as<u32>();
    CK(ctx->rs.ovs.ensure((1 + 3 * RS_OVS_CAP) * 4));
    hipLaunchKernelGGL(k_set_rs_scalars, dim3(1), dim3(64), 0, ctx->stream, sc + SC_RSLEN, (u32)M, 4u, sc + SC_SORTFLAG, ctx->rs.ovs.as<u32>());
    ctx->rs.listed = 0;
    { const int e = allow_big_lds(ctx, reinterpret_cast<const void*>(&k_rs_scatter<false>)); if (e) return e; }
    hipLaunchKernelGGL(k_rs_hist, dim3((unsigned)nch), dim3(RS_NT), 0, ctx->stream, k, n, (u32)chunk, (u32)nch, matrix, sp, 0u);
    CKL("k_rs_hist");
    { const int e = run_scan(ctx, matrix, sc + SC_RSLEN, M); if (e) return e; }
    const size_t ldsA = RsLds<RS_ABINS, RS_TILE>::bytes;
    hipLaunchKernelGGL(k_rs_scatter<false>, dim3((unsigned)nch), dim3(RS_NT), ldsA, ctx->stream, k, v, n, (u32)chunk, (u32)nch, matrix, tk, tv, sp, (const u64*)nullptr, 0u);
    CKL("k_rs_scatter");
    // bucket starts -> host (entry b * nch of the scanned matrix; the scan leaves the total behind the last entry)
    std::vector<u32> start(RS_ABINS + 1);
    CK(hipMemcpy2DAsync(start.data(), 4, matrix, nch * 4, 4, RS_ABINS + 1, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    start[RS_ABINS] = (u32)n;
    const u64 rs_max = rs_max_rows(ctx);
    const int sb = group_bits(start, bA, rs_max);
    ctx->res_w[0] = tk; ctx->res_ab = tv;
    r->partial = true; r->k = tk; r->v = tv;
    if (sb < 0) {                                          // one 10-bit bucket alone exceeds the MSD sort: not a k-mer spectrum -> full-width fallback
        ctx->rs.flag = 1;
        return DSKGPU_OK;
    }
    const u32 per = (1u << bA) >> sb;
    bool first = true;
    for (u32 g0 = 0; g0 < (1u << bA); g0 += per) {
        const u64 b = start[g0], e = start[g0 + per];
        if (e - b < 2 || total - sb < 1) continue;
        const int rc = msd_sort_pairs(ctx, tk + b, tv + b, k + b, v + b, e - b, total - sb, false, (u32)b);      // (in place in tk / tv; k / v = its scratch)
        if (rc) return rc;
        first = false;
    }
    (void)first;
    CK(hipMemcpyAsync(&ctx->rs.flag, sc + SC_SORTFLAG, 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(&ctx->rs.listed, ctx->rs.ovs.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (ctx->tune.verbose) fprintf(stderr, "[dskgpu] row sort: %llu rows in %u groups on their top %d bits, MSD sort per group\n", (unsigned long long)n, 1u << sb, sb);
    return DSKGPU_OK;
}


// ---- row sets of 2^32 rows and more (one- and two-word rows): `-abundance-min 1` on a 200 M-read input, the solid k-mers of a deeper
// human run.  The reference streams rows to Partition<Count> without any such bound (utils/dsk2ascii.cpp:61,77).  The MSD kernels
// index rows with 32 bits, so step A runs SLAB by slab (2^31 rows each): per slab the first-digit histogram and its (32-bit, slab-
// local) scan, then the host lays the 1024 buckets out over ALL rows in 64 bits -- bucket b = [B[b], B[b + 1]), inside it the slabs'
// shares in slab order -- and hands every slab's scatter a 64-bit offset per bin (k_rs_scatter<true>: output index = slab-local
// index + gdel[bin]).  After that every bucket is far below 2^32 rows and the groups of buckets that share their top bits (<= RS_MAX_ROWS
// rows each) are ordered one by one with the ordinary MSD sort, each group with its own flag / list round trip: what a group's sort
// does not order itself goes through the library radix sort FOR THAT GROUP (one-word rows; a group is < 2^32 rows) -- exact for any
// value distribution.  Scratch = a second copy of the rows (the level-0 buffer of the multi-pass count when it is large enough).
template <int W>
int sort_rows_huge(dskgpu_ctx* ctx, u64 n) {
    static_assert(W == 1 || W == 2, "one- and two-word rows");
    constexpr int ABITS = W == 1 ? RS_ABITS : RS2_ABITS;       // first digit of the one- / two-word kernels
    constexpr u32 ABINS = 1u << ABITS;
    const size_t n_al = (size_t)((n + 31) & ~(u64)31), row_bytes = W == 1 ? 12 : 20, need = n_al * row_bytes + 256;
    u64* k = ctx->out_w[0].as<u64>(); u32* v = ctx->out_ab.as<u32>();
    u64* tk = nullptr; u32* tv = nullptr;              // one-word rows: the scratch copy (becomes the result)
    Rows2 K{nullptr, nullptr, nullptr}, T{nullptr, nullptr, nullptr};
    if (W == 2) K = Rows2{ctx->out_w[1].as<u64>(), ctx->out_w[0].as<u64>(), ctx->out_ab.as<u32>()};
    if (ctx->l0buf.cap >= need) {
        u64* base = ctx->l0buf.as<u64>();
        if (W == 1) { tk = base; tv = reinterpret_cast<u32*>(tk + n_al); }
        else { T.hi = base; T.lo = T.hi + n_al; T.ab = reinterpret_cast<u32*>(T.lo + n_al); }
    } else {
        ctx->l0buf.release(); ctx->bufA.release(); ctx->bufB.release();       // (the next count allocates them again)
        for (int x = 0; x < W; ++x) CK(ctx->srt_w[x].ensure(n * 8));
        CK(ctx->srt_ab.ensure(n * 4));
        if (W == 1) { tk = ctx->srt_w[0].as<u64>(); tv = ctx->srt_ab.as<u32>(); }
        else T = Rows2{ctx->srt_w[1].as<u64>(), ctx->srt_w[0].as<u64>(), ctx->srt_ab.as<u32>()};
    }
    const int total = W == 1 ? (int)std::min(64u, 2u * ctx->cfg.kmer_size) : 2 * (int)ctx->cfg.kmer_size;
    const int bA = std::min(ABITS, total);
    const u32 NB = 1u << bA;
    RsSpec sp{total - bA, 0, 0, NB - 1u, 0u, 0u};
    const u64 ncu = (u64)ctx->num_cu;
    const u64 slab = ctx->tune.rs_slab_rows ? std::max<u64>(ctx->tune.rs_slab_rows, 1024) : (1ull << 31);
    const u32 S = (u32)((n + slab - 1) / slab);
    // per slab: chunks of ~64 K rows (a multiple of the CU count of them), matrix of ABINS x nch counters
    std::vector<u64> s_n(S), s_nch(S), s_chunk(S), s_moff(S + 1, 0);
    for (u32 sl = 0; sl < S; ++sl) {
        const u64 ns = std::min<u64>(slab, n - (u64)sl * slab);
        u64 chunk; const u64 nch = step_a_chunks(ns, ncu, W == 1 ? RS_TILE : RS2_TILE, &chunk);
        s_n[sl] = ns; s_nch[sl] = nch; s_chunk[sl] = chunk;
        s_moff[sl + 1] = s_moff[sl] + (u64)ABINS * nch + 2;
    }
    CK(ctx->mat2.ensure(s_moff[S] * 4));
    CK(ctx->rs.lens.ensure((size_t)S * 4));
    ctx->rs.h_lens.resize(S);
    for (u32 sl = 0; sl < S; ++sl) ctx->rs.h_lens[sl] = (u32)((u64)ABINS * s_nch[sl]);
    CK(hipMemcpyAsync(ctx->rs.lens.p, ctx->rs.h_lens.data(), (size_t)S * 4, hipMemcpyHostToDevice, ctx->stream));
    u32* sc = ctx->scalars.as<u32>();
    CK(ctx->rs.ovs.ensure((1 + 3 * RS_OVS_CAP) * 4));
    ctx->rs.h_lin.assign((size_t)S * (ABINS + 1), 0);
    for (u32 sl = 0; sl < S; ++sl) {
        const u64 r0 = (u64)sl * slab;
        u32* matrix = ctx->mat2.as<u32>() + s_moff[sl];
        if (W == 1) hipLaunchKernelGGL(k_rs_hist, dim3((unsigned)s_nch[sl]), dim3(RS_NT), 0, ctx->stream, (const u64*)(k + r0), s_n[sl], (u32)s_chunk[sl], (u32)s_nch[sl], matrix, sp, 0u);
        else { const Rows2C kc{K.hi + r0, K.lo + r0, K.ab + r0}; hipLaunchKernelGGL(k2_hist, dim3((unsigned)s_nch[sl]), dim3(RS_NT), 0, ctx->stream, kc, s_n[sl], (u32)s_chunk[sl], (u32)s_nch[sl], matrix, sp); }
        CKL("k_rs_hist(slab)");
        { const int e = run_scan(ctx, matrix, ctx->rs.lens.as<u32>() + sl, (u64)ABINS * s_nch[sl]); if (e) return e; }
        // bucket starts inside the slab (entry b * nch of the scanned matrix; the scan leaves the slab's total behind the last entry)
        CK(hipMemcpy2DAsync(ctx->rs.h_lin.data() + (size_t)sl * (ABINS + 1), 4, matrix, s_nch[sl] * 4, 4, ABINS + 1, hipMemcpyDeviceToHost, ctx->stream));
    }
    CK(hipStreamSynchronize(ctx->stream));
    // the buckets over all rows, and every (slab, bin) pair's place inside its bucket
    std::vector<u64> B(ABINS + 1, 0);
    for (u32 b = 0; b < ABINS; ++b) {
        u64 t = 0;
        for (u32 sl = 0; sl < S; ++sl) { const u32* lin = ctx->rs.h_lin.data() + (size_t)sl * (ABINS + 1); t += (u64)(lin[b + 1] - lin[b]); }
        B[b + 1] = B[b] + t;
    }
    if (B[ABINS] != n) return fail(ctx, DSKGPU_E_DEVICE, "row sort: the slabs' histograms do not add up to the rows");
    ctx->rs.h_del.assign((size_t)S * ABINS, 0);
    {
        std::vector<u64> at(B.begin(), B.end() - 1);              // next free row of every bucket
        for (u32 sl = 0; sl < S; ++sl) {
            const u32* lin = ctx->rs.h_lin.data() + (size_t)sl * (ABINS + 1);
            for (u32 b = 0; b < ABINS; ++b) { ctx->rs.h_del[(size_t)sl * ABINS + b] = at[b] - (u64)lin[b]; at[b] += (u64)(lin[b + 1] - lin[b]); }      // (wraps in 64 bits: added back by the kernel)
        }
    }
    CK(ctx->rs.del.ensure(ctx->rs.h_del.size() * 8));
    CK(hipMemcpyAsync(ctx->rs.del.p, ctx->rs.h_del.data(), ctx->rs.h_del.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    if (W == 1) { const int e = allow_big_lds(ctx, reinterpret_cast<const void*>(&k_rs_scatter<true>)); if (e) return e; }
    else { const int e = allow_big_lds(ctx, reinterpret_cast<const void*>(&k2_scatter<true>)); if (e) return e; }
    const size_t ldsA1 = RsLds<RS_ABINS, RS_TILE>::bytes, ldsA2 = Rs2Lds<RS2_ABINS, RS2_TILE>::bytes;
    for (u32 sl = 0; sl < S; ++sl) {
        const u64 r0 = (u64)sl * slab;
        const u32* matrix = ctx->mat2.as<u32>() + s_moff[sl];
        const u64* gdel = ctx->rs.del.as<u64>() + (size_t)sl * ABINS;
        if (W == 1) hipLaunchKernelGGL(k_rs_scatter<true>, dim3((unsigned)s_nch[sl]), dim3(RS_NT), ldsA1, ctx->stream, (const u64*)(k + r0), (const u32*)(v + r0), s_n[sl],
                                       (u32)s_chunk[sl], (u32)s_nch[sl], matrix, tk, tv, sp, gdel, 0u);
        else { const Rows2C kc{K.hi + r0, K.lo + r0, K.ab + r0};
               hipLaunchKernelGGL(k2_scatter<true>, dim3((unsigned)s_nch[sl]), dim3(RS_NT), ldsA2, ctx->stream, kc, s_n[sl], (u32)s_chunk[sl], (u32)s_nch[sl], matrix, T, sp, gdel); }
        CKL("k_rs_scatter(slab)");
    }
    CK(hipStreamSynchronize(ctx->stream));                    // (h_rs_del / h_rs_lens were read from host vectors)
    // groups of buckets that share their top sb bits, each <= RS_MAX_ROWS rows; a single bucket above that stands alone (library sort)
    const u64 rs_max = rs_max_rows(ctx);
    const int g = group_bits(B, bA, rs_max), sb = g < 0 ? bA : g;
    const u32 per = NB >> sb;
    ctx->rs.listed = 0;
    u32 ngroups = 0, nlib = 0;
    for (u32 g0 = 0; g0 < NB; g0 += per) {
        const u64 b = B[g0], e = B[g0 + per], m = e - b;
        if (m < 2 || total - sb < 1) continue;
        ++ngroups;
        bool lib = m > rs_max;
        if (!lib) {
            CK(hipMemsetAsync(sc + SC_SORTFLAG, 0, 4, ctx->stream)); CK(hipMemsetAsync(ctx->rs.ovs.p, 0, 4, ctx->stream));
            if (W == 1) {
                const int rc = msd_sort_pairs(ctx, tk + b, tv + b, k + b, v + b, m, total - sb, false, 0u);
                if (rc) return rc;
                ctx->rs.listed = 0;
                CK(hipMemcpyAsync(&ctx->rs.flag, sc + SC_SORTFLAG, 4, hipMemcpyDeviceToHost, ctx->stream));
                CK(hipMemcpyAsync(&ctx->rs.listed, ctx->rs.ovs.p, 4, hipMemcpyDeviceToHost, ctx->stream));
                CK(hipStreamSynchronize(ctx->stream));
                if (!ctx->rs.flag && ctx->rs.listed) { const int e2 = sort_oversize(ctx, tk + b, tv + b); if (e2) return e2; CK(hipStreamSynchronize(ctx->stream)); }
            } else {
                const Rows2 r2{T.hi + b, T.lo + b, T.ab + b}, s2{K.hi + b, K.lo + b, K.ab + b};
                const int rc = msd_sort_rows2(ctx, r2, s2, m, total - sb, false, 0u);
                if (rc) return rc;
                { const int e2 = rows2_rounds(ctx, r2, s2); if (e2) return e2; }      // (synchronises; leaves the flag in ctx->rs.flag)
            }
            lib = ctx->rs.flag != 0;
        }
        if (lib && m >= 0xFFFF0000ull) return fail(ctx, DSKGPU_E_OVERFLOW, "row sort: one value range of the >= 2^32 rows holds 2^32 rows itself (not a k-mer spectrum)");
        if (lib && W == 2) {
            // two-word rows of this group in full-width order: W stable radix passes over an index permutation, gathered into the
            // other copy and copied back (the group's rows in T are a complete permutation whatever the MSD kernels did to them)
            const u64* src[2] = {T.lo + b, T.hi + b};
            { const int rc = sort_index_multiword(ctx, src, m, 2); if (rc) return rc; }
            const unsigned gb = (unsigned)((m + 255) / 256);
            const u32* idx = ctx->srt_idx.as<u32>();
            hipLaunchKernelGGL(k_gather<u64>, dim3(gb), dim3(256), 0, ctx->stream, K.lo + b, (const u64*)(T.lo + b), idx, m);
            hipLaunchKernelGGL(k_gather<u64>, dim3(gb), dim3(256), 0, ctx->stream, K.hi + b, (const u64*)(T.hi + b), idx, m);
            hipLaunchKernelGGL(k_gather<u32>, dim3(gb), dim3(256), 0, ctx->stream, K.ab + b, (const u32*)(T.ab + b), idx, m);
            CKL("row sort: group gather");
            CK(hipMemcpyAsync(T.lo + b, K.lo + b, m * 8, hipMemcpyDeviceToDevice, ctx->stream));
            CK(hipMemcpyAsync(T.hi + b, K.hi + b, m * 8, hipMemcpyDeviceToDevice, ctx->stream));
            CK(hipMemcpyAsync(T.ab + b, K.ab + b, m * 4, hipMemcpyDeviceToDevice, ctx->stream));
            CK(hipStreamSynchronize(ctx->stream));
            ctx->stats.sort_fallback = 1; ++nlib;
        } else if (lib) {
            size_t tmp = 0;
            const unsigned end_bit = (unsigned)(total - sb);
            // LIBRARY SORT (rocprim), labelled FALLBACK: one group of a >= 2^32-row set that the MSD kernels gave up on (or that exceeds them alone)
            CK(rocprim::radix_sort_pairs(nullptr, tmp, tk + b, k + b, tv + b, v + b, (size_t)m, 0u, end_bit, ctx->stream));
            CK(ctx->srt_tmp.ensure(tmp));
            CK(rocprim::radix_sort_pairs(ctx->srt_tmp.p, tmp, tk + b, k + b, tv + b, v + b, (size_t)m, 0u, end_bit, ctx->stream));
            CK(hipMemcpyAsync(tk + b, k + b, m * 8, hipMemcpyDeviceToDevice, ctx->stream));
            CK(hipMemcpyAsync(tv + b, v + b, m * 4, hipMemcpyDeviceToDevice, ctx->stream));
            CK(hipStreamSynchronize(ctx->stream));
            ctx->stats.sort_fallback = 1; ++nlib;
        }
    }
    if (ctx->tune.verbose) fprintf(stderr, "[dskgpu] row sort: %llu rows (>= 2^32 path) in %u slab(s), %u group(s) on their top %d bits, %u through the library sort\n", (unsigned long long)n, S, ngroups, sb, nlib);
    ctx->rs.flag = 0; ctx->rs.listed = 0;
    if (W == 1) { ctx->res_w[0] = tk; ctx->res_ab = tv; }
    else { ctx->res_w[1] = T.hi; ctx->res_w[0] = T.lo; ctx->res_ab = T.ab; }
    return DSKGPU_OK;
}

}  // namespace

// ---- DSKGPU_F_PARTITION_ORDER: the rows of a single pass, ordered inside output partitions of <= PS_CAP / PS2_CAP / PS4_CAP rows (one- / two- /
// four-word rows) by one LDS pass (partsort.h).  In: the sparse rows of the pass (SparseRows).  Out: dense, partition after
// partition -- srt_w[] / srt_ab, four-word rows in out_w[] / out_ab (where sort_rows4 expects its input, should a block give up);
// part_off on the device and (after the caller's synchronisation) in h_part_off; SC_SORTFLAG raised when a block could not order its partition.
// rows a block orders, and the sub-partitions per output partition / the partitions for F sub-partitions holding n_sparse rows (+ a tail)
static u64 part_sort_cap(int W) { return W == 1 ? PS_CAP : W == 2 ? PS2_CAP : PS4_CAP; }
static u32 part_sort_qpp(int W, u64 F, u64 n_sparse) {
    const u64 mean = std::max<u64>(1, (n_sparse + F - 1) / std::max<u64>(F, 1));
    return (u32)std::min<u64>(std::max<u64>(1, (part_sort_cap(W) * 3 / 4) / mean), PS_MAXQ);
}
// partitions a launch will make of `rows`
u32 part_sort_nparts(const SparseRows& rows) {
    const u32 qpp = part_sort_qpp(rows.W, rows.F, rows.n_sparse);
    return (u32)((rows.F + qpp - 1) / qpp) + (rows.n_tail ? 1u : 0u);
}
// one launch: the sparse rows -> dense rows at out / out_ab, partition offsets (relative to the first row) at d_part_off[0 .. *nparts],
// *d_flag raised when a block could not order its partition (the rows are complete either way)
int launch_part_sort(dskgpu_ctx* ctx, const SparseRows& rows, RowsOut out, u32* out_ab, u32* d_part_off, u32* d_flag, u32* nparts_out) {
    const int W = rows.W;
    const u32 qpp = part_sort_qpp(W, rows.F, rows.n_sparse), nparts = part_sort_nparts(rows), nps = nparts - (rows.n_tail ? 1u : 0u);
    const int sh = std::max(0, 2 * (int)ctx->cfg.kmer_size - 12);
    const PsParams pp{qpp, nps, W == 1 ? std::min(sh, 52) : sh, rows.n_tail, ctx->tune.ps_maxc ? std::min<u32>(ctx->tune.ps_maxc, PS_MAXC) : PS_MAXC};
    if (W == 1) hipLaunchKernelGGL(k_part_sort, dim3(nparts), dim3(PS_NT), 0, ctx->stream, rows.as<RsSparse>(), rows.tail_w.w[0], rows.tail_ab, pp, out.w[0], out_ab, d_part_off, d_flag);
    else if (W == 2) hipLaunchKernelGGL(k_part_sort2, dim3(nparts), dim3(PS_NT), 0, ctx->stream, rows.as<Rs2Sparse>(), rows.tail2(), pp, Rows2{out.w[1], out.w[0], out_ab}, d_part_off, d_flag);
    else hipLaunchKernelGGL(k_part_sort4, dim3(nparts), dim3(PS_NT), 0, ctx->stream, rows.as<Rs4Sparse>(), pp, out, out_ab, d_part_off, d_flag);
    CKL("k_part_sort");
    *nparts_out = nparts;
    return DSKGPU_OK;
}

namespace {

int sort_rows_partition_order(dskgpu_ctx* ctx, const SparseRows& rows, u64 n, Round* r) {
    const int W = rows.W;
    const u32 nparts = part_sort_nparts(rows);
    // four-word rows go to out_* (pass_rows sized them for the pass's rows; nothing else is in them while the rows are sparse): the
    // retry in global order, sort_rows4, finds a complete dense copy of the rows where it reads its input
    DevBuf* dst_w = W == 4 ? ctx->out_w : ctx->srt_w;
    DevBuf& dst_ab = W == 4 ? ctx->out_ab : ctx->srt_ab;
    for (int x = 0; x < W; ++x) CK(dst_w[x].ensure(n * 8));
    CK(dst_ab.ensure(n * 4));
    CK(ctx->rs.part_off.ensure(((size_t)nparts + 2) * 4));
    { const int rc = grow_pinned(ctx, ctx->rs.h_part_off, ctx->rs.h_part_cap, (size_t)nparts + 2, ((size_t)nparts + 2) * 2); if (rc) return rc; }
    u32* sc = ctx->scalars.as<u32>();
    hipLaunchKernelGGL(k_set_rs_scalars, dim3(1), dim3(64), 0, ctx->stream, sc + SC_RSLEN, 0u, 1u, sc + SC_SORTFLAG, (u32*)nullptr);
    u32 np = 0;
    RowsOut out{};
    for (int x = 0; x < W; ++x) out.w[x] = dst_w[x].as<u64>();
    { const int rc = launch_part_sort(ctx, rows, out, dst_ab.as<u32>(), ctx->rs.part_off.as<u32>(), sc + SC_SORTFLAG, &np); if (rc) return rc; }
    CK(hipMemcpyAsync(ctx->rs.h_part_off, ctx->rs.part_off.p, ((size_t)nparts + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
    ctx->rs.part_mode = true; ctx->rs.n_parts = nparts; ctx->rs.h_part_off64.clear();
    r->back = 2;            // (the flag travels with the histogram)
    for (int x = 0; x < W; ++x) ctx->res_w[x] = dst_w[x].as<u64>();
    ctx->res_ab = dst_ab.as<u32>();
    return DSKGPU_OK;
}

// four-word rows (k > 64): (top 63 bits of the value, row index) pairs through the MSD sort, gather, then the runs of equal prefix are
// ordered in place by full comparison (exact fallback: sort_rows_full_multiword).  Row sets above RS_MAX_ROWS: the pairs through the
// LIBRARY radix sort on their top 32 bits instead (rocprim: the one library sort on a non-fallback path; 384 M four-word rows are 14 GB)
int sort_rows4(dskgpu_ctx* ctx, u64 n, Round* r) {
    constexpr int W = 4;
    CK(ctx->srt_k.ensure(n * 8)); CK(ctx->s_val.ensure(n * 8));
    CK(ctx->srt_idx.ensure(n * 4)); CK(ctx->srt_idx2.ensure(n * 4));
    const unsigned gb = (unsigned)((n + 255) / 256);
    RowsIn ri{}; RowsOut ro{};
    for (int x = 0; x < W; ++x) { CK(ctx->srt_w[x].ensure(n * 8)); ri.w[x] = ctx->out_w[x].as<u64>(); ro.w[x] = ctx->srt_w[x].as<u64>(); }
    const int bits = 2 * (int)ctx->cfg.kmer_size;
    const bool msd = n <= RS_MAX_ROWS;
    u64* aos = nullptr;
    if (msd) {      // + one record per row for the gather (the full-width fallback buffers are free until then)
        CK(ctx->srt_k2.ensure(n * 8 * (size_t)AosRow<W>::WORDS));
        aos = ctx->srt_k2.as<u64>();
        hipLaunchKernelGGL(k_top_key_aos<W>, dim3(gb), dim3(256), 0, ctx->stream, ri, ctx->out_ab.as<u32>(), n, bits, ctx->srt_k.as<u64>(), ctx->srt_idx.as<u32>(), aos);
    } else hipLaunchKernelGGL(k_top_key<W>, dim3(gb), dim3(256), 0, ctx->stream, ri, n, bits, ctx->srt_k.as<u64>(), ctx->srt_idx.as<u32>());
    u32* flag = ctx->scalars.as<u32>() + SC_SORTFLAG;
    const u32* ties = nullptr;                     // MSD path: the tie pass returns at once unless the sort met equal keys
    const u32* idx; const u64* skey; int run_shift;
    if (msd) {
        // the hand-written MSD sort on (top 63 bits, row index): fully ordered by those 63 bits, what is left to k_fix_runs_multi
        // are the rows that share all of them
        const int e = msd_sort_pairs(ctx, ctx->srt_k.as<u64>(), ctx->srt_idx.as<u32>(), ctx->s_val.as<u64>(), ctx->srt_idx2.as<u32>(), n, 63);
        if (e) return e;
        // sub-buckets the sort listed for another round (thousands of rows sharing 26 and more leading bits): ordered before the rows are
        // gathered by index (one host round trip; a 63-bit prefix leaves ties to k_fix_runs_multi either way)
        CK(hipMemcpyAsync(&ctx->rs.flag, flag, 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipMemcpyAsync(&ctx->rs.listed, ctx->rs.ovs.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        if (!ctx->rs.flag && ctx->rs.listed) {
            const int e2 = sort_oversize(ctx, ctx->srt_k.as<u64>(), ctx->srt_idx.as<u32>());
            if (e2) return e2;
            ctx->rs.listed = 0;
        }
        idx = ctx->srt_idx.as<u32>(); skey = ctx->srt_k.as<u64>(); run_shift = 0; ties = ctx->scalars.as<u32>() + SC_RSTIES;
    } else {
        const unsigned begin_bit = 63u - SORT_TOP_BITS;
        size_t tmp = 0;
        // LIBRARY SORT (rocprim), labelled: four-word rows (k > 64) above RS_MAX_ROWS = 384 M rows -- the (63-bit key, index) pairs on their top 32 bits
        CK(rocprim::radix_sort_pairs(nullptr, tmp, ctx->srt_k.as<u64>(), ctx->s_val.as<u64>(), ctx->srt_idx.as<u32>(), ctx->srt_idx2.as<u32>(),
                                     (size_t)n, begin_bit, 63u, ctx->stream));
        CK(ctx->srt_tmp.ensure(tmp));
        CK(rocprim::radix_sort_pairs(ctx->srt_tmp.p, tmp, ctx->srt_k.as<u64>(), ctx->s_val.as<u64>(), ctx->srt_idx.as<u32>(), ctx->srt_idx2.as<u32>(),
                                     (size_t)n, begin_bit, 63u, ctx->stream));
        CK(hipMemsetAsync(flag, 0, 4, ctx->stream));
        idx = ctx->srt_idx2.as<u32>(); skey = ctx->s_val.as<u64>(); run_shift = (int)begin_bit;
    }
    if (aos) hipLaunchKernelGGL(k_gather_aos<W>, dim3(gb), dim3(256), 0, ctx->stream, ro, ctx->srt_ab.as<u32>(), aos, idx, n);
    else hipLaunchKernelGGL(k_gather_rows<W>, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, ctx->stream, ro, ctx->srt_ab.as<u32>(), ri, ctx->out_ab.as<u32>(), idx, n);
    const unsigned gfix = (unsigned)std::min<u64>(gb, (u64)ctx->num_cu * 32);      // grid-stride kernel: when there are no ties its blocks leave at once
    CK(ctx->rs.fix_list.ensure((1 + 2 * (size_t)FIX_LIST_CAP) * 4));
    CK(hipMemsetAsync(ctx->rs.fix_list.p, 0, 4, ctx->stream));
    u32* fl = ctx->rs.fix_list.as<u32>();
    hipLaunchKernelGGL(k_fix_runs_multi<W>, dim3(gfix), dim3(256), 0, ctx->stream, ro, ctx->srt_ab.as<u32>(), skey, n, run_shift, flag, ties, fl);
    hipLaunchKernelGGL(k_fix_long_runs<W>, dim3((unsigned)ctx->num_cu), dim3(1024), 0, ctx->stream, ro, ctx->srt_ab.as<u32>(), (const u32*)fl, ties);
    CKL("sort_rows");
    CK(hipMemcpyAsync(&ctx->rs.flag, flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    r->partial = true;
    for (int x = 0; x < W; ++x) ctx->res_w[x] = ctx->srt_w[x].as<u64>();
    ctx->res_ab = ctx->srt_ab.as<u32>();
    return DSKGPU_OK;
}

// ---- the first round of a row sort: the path for (W, n, flags, switches), which order_rows finishes.  rows: where the rows lie while they are
// still sparse (W = 0: dense in out_*)
// loaded: the rows of dskgpu_load_rows, which knows neither flag: always ordered, always globally
int sort_rows(dskgpu_ctx* ctx, u64 n, const SparseRows& rows, bool global, Round* r, bool loaded) {
    const int W = ctx->W;
    for (int x = 0; x < 4; ++x) ctx->res_w[x] = x < W ? ctx->out_w[x].as<u64>() : nullptr;
    ctx->res_ab = ctx->out_ab.as<u32>();
    ctx->rs.part_mode = false;
    ctx->rs.listed = 0;
    // (four-word rows have one sparse reader, the partition-order pass: sparse rows that it will not take are an error, not a quiet detour)
    const bool part = (ctx->cfg.flags & DSKGPU_F_PARTITION_ORDER) && !global && n < 0xFFFF0000ull;
    const bool no_sort = (ctx->cfg.flags & DSKGPU_F_NO_SORT) && !loaded;
    if (rows.W && (n == 0 || no_sort || rows.W != W || (W == 4 && !part)))
        return fail(ctx, DSKGPU_E_STATE, "row sort: sparse rows on a path that cannot read them");
    if (n == 0 || no_sort) return DSKGPU_OK;
    if (rows.W && part) return sort_rows_partition_order(ctx, rows, n, r);
    if (rows.W == 1) return sort_rows_msd(ctx, n, r, &rows);      // the rows of a single one-word pass, still in the count kernel's regions (pass_rows made sure this sort takes them)
    if (rows.W == 2) return sort_rows2_msd(ctx, n, r, &rows);     // (the two-word twin)
    const u64 rs_max = rs_max_rows(ctx);
    // 2^32 rows and more (or DSKGPU_RS_SLAB_ROWS: tests): step A slab by slab with 64-bit bucket offsets
    if ((n >= 0xFFFF0000ull || ctx->tune.rs_slab_rows) && W <= 2 && (W == 1 || 2u * ctx->cfg.kmer_size > 64u)) return W == 1 ? sort_rows_huge<1>(ctx, n) : sort_rows_huge<2>(ctx, n);
    if (n >= 0xFFFF0000ull) return fail(ctx, DSKGPU_E_ARG, "row sort: 2^32 rows and more are supported for k <= 64");
    // one-word rows: the hand-written MSD sort (rowsort.h) -- in one piece or group by group (slab by slab above)
    if (W == 1) return n > rs_max ? sort_rows_big(ctx, n, r) : sort_rows_msd(ctx, n, r);
    CK(ctx->srt_w[0].ensure(n * 8)); CK(ctx->srt_ab.ensure(n * 4));
    // two-word rows: the rows themselves through the MSD sort (rowsort2.h)
    if (W == 2) return n <= rs_max ? sort_rows2_msd(ctx, n, r) : sort_rows2_big(ctx, n, r);
    return sort_rows4(ctx, n, r);
}

}  // namespace

// ---- the row order of a count: the n solid rows in out_* (npass > 1: the job's rows, each pass's partitions already ordered when
// ctx->rs.mp.ok held) -> ctx->res_* ascending, globally or inside the partitions of ctx->rs (DSKGPU_F_PARTITION_ORDER).  Finishes
// what the first round left (k_sort_back's read-back, the listed sub-buckets, the full-width library fallback: stats.sort_fallback)
// and, for a single pass (hist_back), copies the abundance histogram to ctx->hist with the same read-back.  Synchronous.
// loaded: the caller is dskgpu_load_rows (loadrows.hip), not a count -- dense rows that may hold EQUAL values, the global order whatever
// the context's flags say, and no histogram to read back (the load bins its own once the equal rows are combined).
int order_rows(dskgpu_ctx* ctx, u64 n, u32 npass, bool loaded) {
    const int W = ctx->W;
    RowSort& rs = ctx->rs;
    PartPasses& mp = rs.mp;
    // the rows of a single pass where the count kernel left them (W = 0: dense in out_*).  The partition order's retry in global order reads the
    // same sparse rows, except four-word ones: sort_rows4 reads the dense rows the partition pass left in out_*
    const SparseRows sparse = ctx->take_sparse_rows();
    // partition order over all passes: every pass ordered its partitions on the way in -- nothing left to sort unless a block gave up
    if (npass > 1 && mp.ok && !mp.passes.empty() && !loaded) {
        u32 h_flag = 1;
        mp.h_off.resize(mp.off_used);
        CK(hipMemcpyAsync(&h_flag, mp.flag.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipMemcpyAsync(mp.h_off.data(), mp.part_off.p, (size_t)mp.off_used * 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        if (!h_flag) {
            rs.h_part_off64.clear();
            for (const auto& pass : mp.passes)
                for (u32 i = 0; i < pass.nparts; ++i) rs.h_part_off64.push_back(pass.row_base + mp.h_off[pass.off_index + i]);
            rs.h_part_off64.push_back(n);
            rs.part_mode = true; rs.n_parts = (u32)(rs.h_part_off64.size() - 1);
            for (int x = 0; x < 4; ++x) ctx->res_w[x] = x < W ? ctx->out_w[x].as<u64>() : nullptr;
            ctx->res_ab = ctx->out_ab.as<u32>();
            rs.flag = 0; rs.listed = 0;
            return DSKGPU_OK;
        }
        if (ctx->tune.verbose) fprintf(stderr, "[dskgpu] row order: a partition of one pass exceeds what one block orders -- global order over all passes instead\n");
    }
    bool global = loaded;
    const bool hist_back = npass == 1 && !loaded;
    for (;;) {
        Round r;
        int rc = sort_rows(ctx, n, global && sparse.W == 4 ? SparseRows{} : sparse, global, &r, loaded);
        if (rc) return rc;
        if (!loaded) ctx->mark("sort");      // (a load marks "load order" itself, behind the fix-up rounds and the fallback that runs of equal rows can take)
        const size_t nh = ctx->hist.size();
        if (r.back) {      // histogram + the sort's two words: one copy into pinned memory (three pageable ones were ~25 us of idle GPU each)
            if ((rc = grow_pinned(ctx, rs.hist_pin, rs.hist_pin_n, nh + 2, nh + 2))) return rc;
            u64* gh = ctx->ghist.as<u64>();
            hipLaunchKernelGGL(k_sort_back, dim3(1), dim3(64), 0, ctx->stream, (const u32*)ctx->scalars.as<u32>(),
                               r.back == 1 ? (const u32*)rs.ovs.as<u32>() : (const u32*)nullptr, gh + nh);
            CKL("k_sort_back");
            const size_t from = hist_back ? 0 : nh;
            CK(hipMemcpyAsync(rs.hist_pin + from, gh + from, (nh + 2 - from) * 8, hipMemcpyDeviceToHost, ctx->stream));
            CK(hipStreamSynchronize(ctx->stream));
            rs.flag = (u32)rs.hist_pin[nh]; rs.listed = (u32)rs.hist_pin[nh + 1];
            if (hist_back) memcpy(ctx->hist.data(), rs.hist_pin, nh * 8);
        } else {
            if (hist_back) CK(hipMemcpyAsync(ctx->hist.data(), ctx->ghist.p, nh * 8, hipMemcpyDeviceToHost, ctx->stream));
            CK(hipStreamSynchronize(ctx->stream));
        }
        if (rs.part_mode && rs.flag) {      // a partition (or a value bin of one) above what a block orders in LDS: the global sort, on the same sparse rows
            if (ctx->tune.verbose) fprintf(stderr, "[dskgpu] row sort: a partition exceeds what one block orders -- global order instead of partition order\n");
            rs.part_mode = false; rs.flag = 0;
            global = true;
            continue;
        }
        if (!r.partial) return DSKGPU_OK;
        // (multi-word rows read their listed sub-buckets back inside the sort: a count left here came with a raised flag)
        if (W == 1 && !rs.flag && rs.listed && (rc = sort_oversize(ctx, r.k, r.v))) return rc;      // sub-buckets listed for another round on their remaining bits
        if (!rs.flag) return DSKGPU_OK;
        if (W == 1) {
            // a run of equal 32-bit prefixes was too long for the in-place fix-up: sort full width into out_* from the copy that holds a
            // permutation of the rows beside it (the result's scratch twin srt_*, or the result itself when that is the scratch copy)
            const bool in_out = r.k == ctx->out_w[0].as<u64>();
            u64* src_k = in_out ? ctx->srt_w[0].as<u64>() : r.k; u32* src_v = in_out ? ctx->srt_ab.as<u32>() : r.v;
            u64* dst_k = ctx->out_w[0].as<u64>(); u32* dst_v = ctx->out_ab.as<u32>();
            size_t tmp = 0;
            const unsigned end_bit = std::min(64u, 2u * ctx->cfg.kmer_size);
            // LIBRARY SORT (rocprim), labelled FALLBACK: the one-word row sort raised its flag (a value distribution no k-mer spectrum has): full-width order of all rows
            CK(rocprim::radix_sort_pairs(nullptr, tmp, src_k, dst_k, src_v, dst_v, (size_t)n, 0u, end_bit, ctx->stream));
            CK(ctx->srt_tmp.ensure(tmp));
            CK(rocprim::radix_sort_pairs(ctx->srt_tmp.p, tmp, src_k, dst_k, src_v, dst_v, (size_t)n, 0u, end_bit, ctx->stream));
            ctx->res_w[0] = dst_k; ctx->res_ab = dst_v;
        } else {
            if (r.scratch.hi) {      // (two-word rows above RS_MAX_ROWS: the complete permutation is the scratch copy)
                CK(hipMemcpyAsync(ctx->out_w[1].p, r.scratch.hi, n * 8, hipMemcpyDeviceToDevice, ctx->stream));
                CK(hipMemcpyAsync(ctx->out_w[0].p, r.scratch.lo, n * 8, hipMemcpyDeviceToDevice, ctx->stream));
                CK(hipMemcpyAsync(ctx->out_ab.p, r.scratch.ab, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
            }
            if ((rc = sort_rows_full_multiword(ctx, n))) return rc;      // out_w holds the unsorted rows
        }
        CK(hipStreamSynchronize(ctx->stream));
        ctx->stats.sort_fallback = 1;
        return DSKGPU_OK;
    }
}

// partitions of the last result and the rows of partition p
u32 rows_partitions(const dskgpu_ctx* ctx) {
    if (ctx->rs.part_mode) return ctx->rs.n_parts;      // (partition order: the partitions are what the blocks of k_part_sort ordered)
    return ctx->cfg.nb_partitions ? ctx->cfg.nb_partitions : 4u;
}


void rows_partition_range(const dskgpu_ctx* ctx, u32 p, u64* b, u64* e) {
    const RowSort& rs = ctx->rs;
    if (rs.part_mode) {
        if (ctx->filtered.cur >= 0) { *b = ctx->filtered.part_off[p]; *e = ctx->filtered.part_off[p + 1]; return; }      // (dskgpu_filter_rows: the kept rows of every partition)
        if (!rs.h_part_off64.empty()) { *b = rs.h_part_off64[p]; *e = rs.h_part_off64[p + 1]; }      // (several passes: 64-bit row numbers)
        else { *b = rs.h_part_off[p]; *e = rs.h_part_off[p + 1]; }
        return;
    }
    const u64 P = ctx->stats.n_partitions, n = ctx->n_rows;
    *b = n * p / P; *e = n * (p + 1) / P;
}
