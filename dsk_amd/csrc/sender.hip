// sender.hip -- the super-k-mer SENDER: everything that turns the 2-bit read stream (ctx->packed / inval) into records (superkmer.h).
// Two users, one Sender state each (engine.h):
//   the multi-GPU exchange (ctx->sender): dskgpu_mg_sample / _make_table / _set_table balance the owners, sk_prepare sizes the send
//     layout, sk_scatter or the slice calls write the records grouped by owner into the caller's buffer;
//   the record-based level 0 of a multi-pass count (ctx->l0_sender; rec_l0_prepare / rec_l0_sweep, called by run_pipeline): the
//     passes are "virtual owners" and a sweep writes the records of as many of them as HBM holds into ctx->l0buf.
// Of the rest of the context it uses the encoded reads, mat1, the scalars and h_ovf1 as scratch -- nothing of the receiver (dskgpu.hip).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "engine.h"
#include "superkmer.h"

namespace {

// the sender kernels with k and m at compile time for the BASELINE configs (superkmer.h: sk_tile_fx), at run time otherwise
#define SK_DISPATCH(ctx_, SP_, CALL) do { \
        if (!(ctx_)->tune.sk_generic && (SP_).k == 31 && (SP_).m == 10) { CALL(31, 10); } \
        else if (!(ctx_)->tune.sk_generic && (SP_).k == 63 && (SP_).m == 10) { CALL(63, 10); } \
        else { CALL(0, 0); } } while (0)

// (asynchronous on the context's stream; the caller checks the launch with CKL under the name its logs know)
void launch_sk_sample(dskgpu_ctx* ctx, const SkParams& sp, unsigned grid, unsigned long long* load) {
#define CALL(K_, M_) hipLaunchKernelGGL((k_sk_sample<K_, M_>), dim3(grid), dim3(SK_NT), 0, ctx->stream, ctx->packed.as<u64>(), ctx->inval.as<u32>(), sp, load)
    SK_DISPATCH(ctx, sp, CALL);
#undef CALL
}
void launch_sk_hist(dskgpu_ctx* ctx, const SkParams& sp, unsigned grid, u32* mat, unsigned long long* kmers) {
#define CALL(K_, M_) hipLaunchKernelGGL((k_sk_hist<K_, M_>), dim3(grid), dim3(SK_NT), 0, ctx->stream, ctx->packed.as<u64>(), ctx->inval.as<u32>(), sp, mat, kmers)
    SK_DISPATCH(ctx, sp, CALL);
#undef CALL
}
// cb64 == nullptr: the slice layout (k_sk_scatter<true>); else the exact one, cb64 = the record index of every (owner, chunk) pair
void launch_sk_scatter(dskgpu_ctx* ctx, const SkParams& sp, unsigned grid, const unsigned long long* cb64, u64* send, u32* ovf, unsigned long long* kmers) {
#define CALL(K_, M_) do { \
        if (cb64) hipLaunchKernelGGL((k_sk_scatter<false, K_, M_>), dim3(grid), dim3(SK_NT), 0, ctx->stream, ctx->packed.as<u64>(), ctx->inval.as<u32>(), sp, cb64, send, ovf, kmers); \
        else hipLaunchKernelGGL((k_sk_scatter<true, K_, M_>), dim3(grid), dim3(SK_NT), 0, ctx->stream, ctx->packed.as<u64>(), ctx->inval.as<u32>(), sp, cb64, send, ovf, kmers); } while (0)
    SK_DISPATCH(ctx, sp, CALL);
#undef CALL
}

// ---- repartition table of the super-k-mer owner map (superkmer.h)
void default_table(uint32_t world, uint8_t* table) { for (u32 b = 0; b < SK_BUCKETS; ++b) table[b] = (uint8_t)((b * world) / SK_BUCKETS); }
int upload_table(dskgpu_ctx* ctx, Sender& s) {
    if (s.h_table.size() != SK_BUCKETS) { s.h_table.resize(SK_BUCKETS); default_table(s.sp.G, s.h_table.data()); s.table_dirty = true; }
    if (s.table_dirty) {
        CK(s.table.ensure(SK_BUCKETS));
        CK(hipMemcpyAsync(s.table.p, s.h_table.data(), SK_BUCKETS, hipMemcpyHostToDevice, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        s.table_dirty = false;
    }
    s.sp.table = s.table.as<unsigned char>();
    s.sp.has_split = std::find(s.h_table.begin(), s.h_table.end(), (uint8_t)SK_SPLIT) != s.h_table.end() ? 1u : 0u;
    return DSKGPU_OK;
}
// tiles / chunks of the sender kernels over the encoded stream
void sk_geometry(const dskgpu_ctx* ctx, Sender& s, u64 nwords) {
    SkParams& sp = s.sp;
    sp.ngroups = nwords * 2;
    sp.ntiles = std::max<u64>(1, (sp.ngroups + SK_GROUPS - 1) / SK_GROUPS);
    // whole rounds of blocks: the k = 31 kernels (68 VGPRs, 50 KB of LDS) run three 512-thread blocks per CU, the others two
    const u64 per_cu = (!ctx->tune.sk_generic && sp.k == 31 && sp.m == 10) ? 9 : 8;
    u64 nch = std::min<u64>(std::max<u64>(1, sp.ntiles / 8), (u64)ctx->num_cu * per_cu);     // >= 8 tiles per chunk when there are that many
    const u64 tpc = (sp.ntiles + nch - 1) / nch;
    nch = (sp.ntiles + tpc - 1) / tpc;
    sp.tiles_per_chunk = (u32)tpc; sp.nchunks = (u32)nch;
    sp.c0 = 0; sp.c0g = 0; sp.clen = (u32)nch; sp.rbase = 0;      // one layout group: the whole step
}

// The k-mer load of every minimizer bucket of the encoded reads, sampled: every 16th tile of a large input, all tiles of a small one
// (-> *step; the loads are those of the sampled tiles, not scaled).  s.sp holds the geometry (sk_geometry).
int sample_loads(dskgpu_ctx* ctx, Sender& s, uint64_t* loads, u32* step) {
    SkParams ss = s.sp;
    ss.sample_step = *step = ss.tiles_per_chunk >= 16 ? 16u : 1u;
    ss.table = nullptr;
    CK(s.load.ensure((size_t)SK_BUCKETS * 8));
    CK(hipMemsetAsync(s.load.p, 0, (size_t)SK_BUCKETS * 8, ctx->stream));
    launch_sk_sample(ctx, ss, ss.nchunks, s.load.as<unsigned long long>());
    CKL("k_sk_sample");
    CK(hipMemcpyAsync(loads, s.load.p, (size_t)SK_BUCKETS * 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return DSKGPU_OK;
}

// records of a slice sized from a sampled mean: + 8 % + 128
inline u64 padded_slice(u64 sl) { return sl + sl * 2 / 25 + 128; }

}  // namespace

// ---- level 0 of a multi-pass count as super-k-mer RECORDS: the passes are "virtual owners"
// What the multi-GPU step does between GPUs, one GPU does between its passes: the pass of a k-mer is the OWNER that the minimizer
// repartition gives its window (owner = table[bucket of the minimizer], G owners = G passes; heavy buckets are split by k-mer),
// a sweep over the 2-bit reads writes the records of as many owners as HBM holds (k_sk_scatter with an owner window, every owner
// with its own slice length and region), and every pass then runs its level 1 straight from its records (k_scatter<W, 2, 1>),
// sized from a sample of them.  Records are 2.3-2.5 bytes per k-mer where a key array takes 8 (16 for two-word keys): a 90 Gbp
// input goes through in 2-3 sweeps instead of 7, 30 Gbp in one -- and the sender never forms a k-mer, which makes a sweep cheaper
// than the key-array one as well.  DSK writes super-k-mers to its partition files for the same reason (CHANGELOG.md:13;
// doc/paper.tex:65-67 for the passes).  Needs 20 <= k <= 64 (records) and <= SK_MAX_OWNERS passes; anything else, or a slice
// of the sampled layout that overflows, takes the key-array level 0 / the pass filter instead (ctx->rec_l0_off).
// `s` is the level 0's own Sender (ctx->l0_sender): the exchange's owners and table are not touched.
int rec_l0_prepare(dskgpu_ctx* ctx, Sender& s, u64 nwords, u32 G, RecL0* rl) {
    SkParams& sp = s.sp;
    sk_geometry(ctx, s, nwords);
    sp.G = G; sp.olo = 0; sp.ohi = G; sp.oslice = nullptr; sp.obase = nullptr;
    const u64 nch = sp.nchunks, tpc = sp.tiles_per_chunk;
    // 1. the repartition table for G owners, from the sampled k-mer load of every minimizer bucket
    u32 step = 1;
    std::vector<uint64_t> loads(SK_BUCKETS);
    if (const int rc = sample_loads(ctx, s, loads.data(), &step)) return rc;
    s.h_table.resize(SK_BUCKETS);
    dskgpu_mg_make_table(loads.data(), G, s.h_table.data());
    s.table_dirty = true;
    if (const int rc = upload_table(ctx, s)) return rc;
    // 2. records per (owner, chunk), counted on every 16th tile (all tiles of a small input): the slice of an (owner, chunk) pair
    const u64 M = (u64)G * nch;
    CK(ctx->mat1.ensure((M + 1) * 4));
    CK(s.sent.ensure(3 * SK_MAX_OWNERS * 8));
    CK(hipMemsetAsync(s.sent.as<u64>() + SK_MAX_OWNERS, 0, SK_MAX_OWNERS * 8, ctx->stream));
    sp.sample_step = step;
    launch_sk_hist(ctx, sp, (unsigned)nch, ctx->mat1.as<u32>(), s.sent.as<unsigned long long>() + SK_MAX_OWNERS);
    CKL("k_sk_hist");
    std::vector<u32> cells(M);
    CK(hipMemcpyAsync(cells.data(), ctx->mat1.p, M * 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    const u64 sampled_tiles = (tpc + step - 1) / step;
    rl->G = G; rl->nch = nch;
    for (u32 o = 0; o < G; ++o) {
        u64 tot = 0, mx = 0;
        for (u64 c = 0; c < nch; ++c) { const u64 v = cells[(size_t)o * nch + c]; tot += v; mx = std::max(mx, v); }
        u64 sl;
        if (step == 1) sl = mx + 8;                                                        // every tile counted: the busiest chunk's figure is exact
        else sl = padded_slice(tot * tpc / (sampled_tiles * nch) + 1);                     // the mean per chunk, scaled (as the multi-GPU sender)
        if (ctx->tune.sk_slice) sl = ctx->tune.sk_slice;                                   // tests
        if (sl * nch >= 0xFFFF0000ull) return REC_L0_NO;                                   // (record positions inside an owner's region stay 32-bit on the reading side)
        rl->slice[o] = (u32)sl; rl->region[o] = sl * nch;
    }
    ctx->mark("level0_size");
    return DSKGPU_OK;
}

// one sweep: the records of owners [olo, ohi) into ctx->l0buf; base[o] = first 8-byte word of owner o's region; s.h_sent[o] = the k-mers
// inside them.  -> REC_L0_NO when a slice overflowed (the sampled layout did not hold: the caller starts over on the key-array path)
int rec_l0_sweep(dskgpu_ctx* ctx, Sender& s, const RecL0& rl, u32 olo, u32 ohi, u64 (&base_words)[SK_MAX_OWNERS]) {
    SkParams sp = s.sp;
    u64 obase[SK_MAX_OWNERS] = {0}; u32 osl[SK_MAX_OWNERS] = {0};
    u64 tot = 0;
    for (u32 o = 0; o < rl.G; ++o) { osl[o] = rl.slice[o]; obase[o] = tot; if (o >= olo && o < ohi) tot += rl.region[o]; base_words[o] = obase[o] * sp.R; }
    CK(ctx->l0buf.ensure(tot * sp.R * 8 + 64));
    CK(s.lay.ensure(SK_MAX_OWNERS * 12));
    CK(hipMemcpyAsync(s.lay.p, obase, sizeof obase, hipMemcpyHostToDevice, ctx->stream));
    CK(hipMemcpyAsync(s.lay.as<u64>() + SK_MAX_OWNERS, osl, sizeof osl, hipMemcpyHostToDevice, ctx->stream));
    sp.olo = olo; sp.ohi = ohi; sp.obase = s.lay.as<unsigned long long>(); sp.oslice = reinterpret_cast<const u32*>(s.lay.as<u64>() + SK_MAX_OWNERS);
    sp.c0 = 0; sp.c0g = 0; sp.clen = (u32)rl.nch; sp.rbase = 0; sp.slice = 0;
    u32* sc = ctx->scalars.as<u32>();
    CK(hipMemsetAsync(s.sent.p, 0, SK_MAX_OWNERS * 8, ctx->stream));
    CK(hipMemsetAsync(sc + SC_OVF1, 0, 4, ctx->stream));
    launch_sk_scatter(ctx, sp, sp.nchunks, nullptr, ctx->l0buf.as<u64>(), sc + SC_OVF1, s.sent.as<unsigned long long>());
    CKL("k_sk_scatter(passes)");
    ctx->mark("level0");
    CK(hipMemcpyAsync(&ctx->h_ovf1, sc + SC_OVF1, 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(s.h_sent, s.sent.p, SK_MAX_OWNERS * 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));        // (obase / osl are locals)
    if (ctx->tune.verbose) fprintf(stderr, "[dskgpu] level 0 (records): passes %u..%u of %u materialised, %.2f GB%s\n", olo, ohi - 1, rl.G, (double)tot * sp.R * 8e-9,
                                   ctx->h_ovf1 ? " -- a slice overflowed: starting over on the key-array path" : "");
    return ctx->h_ovf1 ? REC_L0_NO : DSKGPU_OK;
}

// ---- multi-GPU exchange as super-k-mer records (superkmer.h)
// Sender, step 1: encode + count the records per (owner, chunk) + scan.  Leaves the record range of every
// owner in h_rstart; the exact send size is known before the caller allocates the send buffer.
static int sk_prepare(dskgpu_ctx* ctx) {
    Sender& s = ctx->sender;
    ctx->st_names.clear(); ctx->st_ms.clear(); ctx->marks.clear(); ctx->ev_used = 0;
    s.prepared = false;
    ctx->mark("start");
    u64 nwords = 0;
    int rc = DSKGPU_OK;
    if (ctx->enc_fresh) { nwords = (ctx->n_bytes + 31) / 32; ctx->enc_fresh = false; }      // (the repartition sample of this step just encoded these reads)
    else if ((rc = encode_current(ctx, &nwords))) return rc;
    ctx->mark("encode");
    SkParams& sp = s.sp;
    sk_geometry(ctx, s, nwords);
    if ((rc = upload_table(ctx, s))) return rc;
    const u64 nch = sp.nchunks, tpc = sp.tiles_per_chunk;
    const u64 M = (u64)sp.G * nch;
    CK(ctx->scalars.ensure(SC_COUNT * 4));
    u32* h_sc = ctx->h_sc;
    std::memset(h_sc, 0, sizeof(ctx->h_sc));
    u32* sc = ctx->scalars.as<u32>();
    CK(hipMemcpyAsync(sc, h_sc, sizeof(ctx->h_sc), hipMemcpyHostToDevice, ctx->stream));
    CK(ctx->mat1.ensure((M + 1) * 4));
    // Exact layout: count every record, one scan places them.  Slice layout (default): count the records of every
    // 16th tile only, give every (owner, chunk) pair one slice of the estimated mean + 8 % + 128 records; the scatter
    // pads the slices with zero-length records.  Saves the full counting pass (1.95 of 5 ms); ~8 % more words to send.
    // Either way every record position is 64-bit from here on (the count matrix -- <= 64 owners x 2048 chunks of u32 -- comes to
    // the host, where it is summed / scanned in 64 bits): a rank's shard may be of any size.  The reference's own human run is
    // ONE execute() over 160 GB of reads (doc/human_log:3-4,20-24; README.md:126-130); on 8 GPUs that is 11.3 GB per rank.
    const bool slices = !s.exact && !ctx->tune.sk_exact && tpc >= 8;
    sp.sample_step = slices ? 16u : 1u;
    CK(s.sent.ensure(3 * SK_MAX_OWNERS * 8));
    CK(hipMemsetAsync(s.sent.as<u64>() + SK_MAX_OWNERS, 0, SK_MAX_OWNERS * 8, ctx->stream));
    launch_sk_hist(ctx, sp, (unsigned)nch, ctx->mat1.as<u32>(), s.sent.as<unsigned long long>() + SK_MAX_OWNERS);
    CKL("k_sk_hist");
    CK(hipMemcpyAsync(s.h_est, s.sent.as<u64>() + SK_MAX_OWNERS, SK_MAX_OWNERS * 8, hipMemcpyDeviceToHost, ctx->stream));
    ctx->mark("mg_hist");
    s.h_cells.resize(M);
    CK(hipMemcpyAsync(s.h_cells.data(), ctx->mat1.p, M * 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    s.h_rstart.assign(sp.G + 1, 0);
    s.slices = false;
    if (slices) {
        u64 worst = 0;                                       // sampled records of the busiest owner
        for (u32 o = 0; o < sp.G; ++o) { u64 t = 0; for (u64 c = 0; c < nch; ++c) t += s.h_cells[(size_t)o * nch + c]; worst = std::max(worst, t); }
        const u64 sampled_tiles = (tpc + sp.sample_step - 1) / sp.sample_step;            // per chunk
        u64 slice = worst * tpc / (sampled_tiles * nch) + 1;                              // records per (owner, chunk), estimated
        const u64 min_slice = ctx->tune.sk_minslice;                                      // (tests lower it)
        const bool small = slice < min_slice || worst < 20000;    // fixed slack too visible in the send volume, or too few sampled records to trust the estimate
        slice = padded_slice(slice);
        if (ctx->tune.sk_slice) slice = ctx->tune.sk_slice;                               // tests
        if (!small && slice < 0xFFFF0000ull) {                                            // (a block's cursor inside ONE slice is 32-bit)
            sp.slice = (u32)slice;
            for (u32 o = 0; o < sp.G; ++o) s.h_est[o] = s.h_est[o] * tpc / sampled_tiles;      // sampled tiles -> all tiles
            for (u32 o = 0; o <= sp.G; ++o) s.h_rstart[o] = (u64)o * nch * slice;
            s.slices = true;
        } else {                                             // small input: count exactly after all
            s.exact = true;
            return sk_prepare(ctx);
        }
    } else {
        // exact layout: the 64-bit exclusive scan of the owner-major count matrix
        s.h_cb64.resize(M + 1);
        u64 run = 0;
        for (u64 i = 0; i < M; ++i) { s.h_cb64[i] = run; run += s.h_cells[i]; }
        s.h_cb64[M] = run;
        for (u32 o = 0; o <= sp.G; ++o) s.h_rstart[o] = s.h_cb64[(u64)o * nch];
        CK(s.cb64.ensure((M + 1) * 8));
        CK(hipMemcpyAsync(s.cb64.p, s.h_cb64.data(), (M + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
    }
    ctx->resolve_marks();
    s.prepared = true;
    return DSKGPU_OK;
}

// words the send buffer of dskgpu_mg_scatter must hold (0: sk_prepare failed -- the error text stays in the context, the scatter reports it)
uint64_t sk_send_capacity_words(dskgpu_ctx* ctx) {
    const Sender& s = ctx->sender;
    if (!s.prepared && sk_prepare(ctx) != DSKGPU_OK) return 0;
    return s.h_rstart[s.sp.G] * s.sp.R + 1;
}

// Sender, step 2: write the records, grouped by owner, into the caller's buffer.
int sk_scatter(dskgpu_ctx* ctx, void* d_send, uint64_t capacity_words, uint64_t* send_words) {
    Sender& s = ctx->sender;
    int rc;
    if (!s.prepared && (rc = sk_prepare(ctx))) return rc;
    const SkParams& sp = s.sp;
    if (capacity_words < s.h_rstart[sp.G] * sp.R) return fail(ctx, DSKGPU_E_ARG, "send buffer too small");
    ctx->marks.clear(); ctx->ev_used = 0;
    ctx->mark("start");
    u32* sc = ctx->scalars.as<u32>();
    CK(hipMemsetAsync(s.sent.p, 0, SK_MAX_OWNERS * 8, ctx->stream));
    if (s.slices) CK(hipMemsetAsync(sc + SC_OVF1, 0, 4, ctx->stream));
    launch_sk_scatter(ctx, sp, sp.nchunks, s.slices ? nullptr : s.cb64.as<unsigned long long>(), static_cast<u64*>(d_send), sc + SC_OVF1, s.sent.as<unsigned long long>());
    CKL("k_sk_scatter");
    ctx->mark("mg_scatter");
    if (s.slices) CK(hipMemcpyAsync(&ctx->h_ovf1, sc + SC_OVF1, 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(s.h_sent, s.sent.p, SK_MAX_OWNERS * 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    ctx->resolve_marks();
    if (s.slices && ctx->h_ovf1) {      // a slice overflowed: exact counts for these reads from now on (and right away)
        s.exact = true; s.prepared = false;
        if ((rc = sk_prepare(ctx))) return rc;
        return sk_scatter(ctx, d_send, capacity_words, send_words);      // may report "send buffer too small": ask for the capacity again
    }
    for (u32 o = 0; o < sp.G; ++o) send_words[o] = (s.h_rstart[o + 1] - s.h_rstart[o]) * sp.R;
    s.prepared = false;      // packed/mat1 are scratch of the next call
    return DSKGPU_OK;
}

extern "C" {

int dskgpu_mg_sample(dskgpu_ctx* ctx, uint64_t* loads) {
    if (!ctx || !loads) return DSKGPU_E_ARG;
    std::memset(loads, 0, (size_t)SK_BUCKETS * 8);
    if (!ctx->sk_mode) return DSKGPU_OK;            // explicit keys: the owner is a bit field of the k-mer hash, balanced by construction
    CK(hipSetDevice(ctx->cfg.device));
    RAW_SYNC(ctx);
    u64 nwords = 0;
    int rc = encode_current(ctx, &nwords);
    if (rc) return rc;
    sk_geometry(ctx, ctx->sender, nwords);
    u32 step = 1;
    if ((rc = sample_loads(ctx, ctx->sender, loads, &step))) return rc;
    for (u32 b = 0; b < SK_BUCKETS; ++b) loads[b] *= step;      // an estimate of the whole shard's load
    ctx->sender.prepared = false;                   // packed / inval were rewritten
    ctx->enc_fresh = true;                          // ... with the encoding of the current reads: the sender's sizing pass reuses it
    return DSKGPU_OK;
}

void dskgpu_mg_make_table(const uint64_t* loads, uint32_t world, uint8_t* table) {
    if (!table) return;
    if (world == 0) world = 1;
    default_table(world, table);
    if (!loads || world == 1) return;
    u64 total = 0;
    for (u32 b = 0; b < SK_BUCKETS; ++b) total += loads[b];
    if (total == 0) return;
    // a bucket that alone holds more than a quarter of an owner's fair share is split over all owners by k-mer
    const u64 heavy = std::max<u64>(1, total / world / 4);
    std::vector<u64> owner_load(world, 0);
    std::vector<u32> order;
    u64 split_load = 0;
    for (u32 b = 0; b < SK_BUCKETS; ++b) {
        if (loads[b] > heavy) { table[b] = (uint8_t)SK_SPLIT; split_load += loads[b]; }
        else if (loads[b]) order.push_back(b);        // (buckets the sample did not see keep their default owner)
    }
    for (u32 o = 0; o < world; ++o) owner_load[o] = split_load / world;
    std::stable_sort(order.begin(), order.end(), [&](u32 a, u32 b) { return loads[a] > loads[b]; });    // largest first, ties by index
    for (u32 b : order) {
        u32 best = 0;
        for (u32 o = 1; o < world; ++o) if (owner_load[o] < owner_load[best]) best = o;
        table[b] = (uint8_t)best;
        owner_load[best] += loads[b];
    }
}

int dskgpu_mg_set_table(dskgpu_ctx* ctx, const uint8_t* table) {
    if (!ctx) return DSKGPU_E_ARG;
    if (table)          // validate before the table in use is touched: a rejected table leaves the context as it was
        for (u32 b = 0; b < SK_BUCKETS; ++b)
            if (table[b] != SK_SPLIT && table[b] >= ctx->cfg.world_size) return fail(ctx, DSKGPU_E_ARG, "repartition table names an owner outside the world");
    Sender& s = ctx->sender;
    s.h_table.resize(SK_BUCKETS);
    if (table) std::memcpy(s.h_table.data(), table, SK_BUCKETS);
    else default_table(ctx->cfg.world_size, s.h_table.data());
    s.table_dirty = true;
    s.prepared = false;
    return DSKGPU_OK;
}

int dskgpu_mg_sent_kmers(dskgpu_ctx* ctx, uint64_t* kmers) {
    if (!ctx || !kmers) return DSKGPU_E_ARG;
    for (u32 o = 0; o < ctx->cfg.world_size; ++o) kmers[o] = ctx->sender.h_sent[o];
    return DSKGPU_OK;
}

// ---- a step in slices (the exchange of slice i overlaps the sender's slice i + 1 and the receiver's level 1 of slice i - 1).
// Only with the sampled send layout (its sizes are known before a record exists): slice s = the chunks [s * nch / S, (s + 1) * nch / S),
// a layout group of its own in the send buffer (SkParams::c0g, clen, rbase), owner-major inside.
static void sk_slice_range(const SkParams& sp, u32 S, u32 s, u32* cb, u32* ce) { *cb = (u32)((u64)s * sp.nchunks / S); *ce = (u32)((u64)(s + 1) * sp.nchunks / S); }

int dskgpu_mg_slices_prepare(dskgpu_ctx* ctx, uint32_t want, uint32_t* nslices, uint64_t* send_words, uint64_t* kmers_est) {
    if (!ctx || !nslices || !send_words || !kmers_est) return DSKGPU_E_ARG;
    *nslices = 0;
    if (!ctx->sk_mode) return DSKGPU_OK;                 // explicit keys: one piece
    CK(hipSetDevice(ctx->cfg.device));
    RAW_SYNC(ctx);
    Sender& s = ctx->sender;
    s.nslices = 0;
    if (!s.prepared) { const int rc = sk_prepare(ctx); if (rc) return rc; }
    const SkParams& sp = s.sp;
    if (!s.slices || want < 2) return DSKGPU_OK;          // exact layout (small input, or a slice overflowed before): one piece
    const u32 S = std::min<u32>(want, sp.nchunks);
    if (S < 2) return DSKGPU_OK;
    for (u32 sl = 0; sl < S; ++sl) {
        u32 cb, ce; sk_slice_range(sp, S, sl, &cb, &ce);
        for (u32 o = 0; o < sp.G; ++o) send_words[(size_t)sl * sp.G + o] = (u64)(ce - cb) * sp.slice * sp.R;
    }
    for (u32 o = 0; o < sp.G; ++o) kmers_est[o] = s.h_est[o];
    *nslices = S; s.nslices = S;
    return DSKGPU_OK;
}

// launch the scatter of slice sl (asynchronous on the context's stream: the caller records an event behind it and starts the exchange)
int dskgpu_mg_scatter_slice(dskgpu_ctx* ctx, void* d_send, uint64_t capacity_words, uint32_t sl) {
    if (!ctx || !d_send) return DSKGPU_E_ARG;
    CK(hipSetDevice(ctx->cfg.device));
    Sender& s = ctx->sender;
    if (!s.prepared || !s.slices || sl >= s.nslices) return fail(ctx, DSKGPU_E_STATE, "dskgpu_mg_scatter_slice without dskgpu_mg_slices_prepare");
    SkParams sp = s.sp;
    if (capacity_words < s.h_rstart[sp.G] * sp.R) return fail(ctx, DSKGPU_E_ARG, "send buffer too small");
    if (sl == 0) {
        ctx->marks.clear(); ctx->ev_used = 0;
        ctx->mark("start");
        CK(hipMemsetAsync(s.sent.p, 0, SK_MAX_OWNERS * 8, ctx->stream));
        CK(hipMemsetAsync(s.sent.as<u64>() + 2 * SK_MAX_OWNERS, 0, 8, ctx->stream));
    }
    u32 cb, ce; sk_slice_range(sp, s.nslices, sl, &cb, &ce);
    sp.c0 = cb; sp.c0g = cb; sp.clen = ce - cb; sp.rbase = (u64)cb * sp.G * sp.slice;
    // (the overflow flag of a sliced step lives apart from the scalars: the receiver's pipeline, which runs before the flag is
    //  read, resets those)
    if (ce > cb) launch_sk_scatter(ctx, sp, ce - cb, nullptr, static_cast<u64*>(d_send), reinterpret_cast<u32*>(s.sent.as<u64>() + 2 * SK_MAX_OWNERS), s.sent.as<unsigned long long>());
    CKL("k_sk_scatter");
    if (sl + 1 == s.nslices) ctx->mark("mg_scatter");
    return DSKGPU_OK;
}

// end of the sender's part: did a slice of the send layout overflow (then the records of this step are incomplete -- every rank
// repeats the step in one piece; this context will use exact counts), and the k-mers that were packed
int dskgpu_mg_slices_finish(dskgpu_ctx* ctx, int* overflowed) {
    if (!ctx || !overflowed) return DSKGPU_E_ARG;
    CK(hipSetDevice(ctx->cfg.device));
    Sender& s = ctx->sender;
    if (!s.nslices) return fail(ctx, DSKGPU_E_STATE, "dskgpu_mg_slices_finish without dskgpu_mg_slices_prepare");
    CK(hipMemcpyAsync(&ctx->h_ovf1, s.sent.as<u64>() + 2 * SK_MAX_OWNERS, 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(s.h_sent, s.sent.p, SK_MAX_OWNERS * 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    *overflowed = ctx->h_ovf1 ? 1 : 0;
    if (ctx->h_ovf1) s.exact = true;
    s.prepared = false; s.nslices = 0;
    return DSKGPU_OK;
}

}  // extern "C"
