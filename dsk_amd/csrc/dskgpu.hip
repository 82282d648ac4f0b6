// dskgpu.hip -- the count path over the HIP kernels in kernels.h, and its part of the C-ABI (include/dskgpu.h): create / destroy, count,
// the receive side of the multi-GPU exchange, the result.  The other units and what they own: engine.h.  Host-side orchestration that
// stands where SortingCountAlgorithm<span>::execute() is called (src/DSK.cpp:60).
// gfx950 only; there is no CPU fallback: every entry point needs a HIP device.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <cmath>
#include <string>
#include <vector>

#include "engine.h"
#include "kernels.h"
#include "planning.h"
#include "superkmer_recv.h"

#define DSKGPU_VERSION "dskgpu 0.1 (gfx950)"

namespace {

thread_local std::string g_create_err;

// Where a big buffer lies in HBM decides how fast scattered stores into it go: of several 9.6 GB allocations of one process some take
// the store pattern of the level-1 scatter (256 blocks x 512 streams x 256-byte runs) in 3.14 ms and others in 3.41 (a streaming
// fill: 1.70 / 1.79), the same virtual address changes class after a free + malloc, and the kernels' "two speeds" (level 1: 3.8 /
// 4.5 ms) follow (tools/micro/write_place.hip).  With DSKGPU_PLACE = K > 1 every allocation of >= 256 MB is the best of up to K
// candidates, each timed with that store pattern (one-off: ~0.1 s per candidate of 10 GB); the others are freed.
__global__ __launch_bounds__(1024) void k_place_probe(unsigned long long* __restrict__ out, unsigned long long n) {
    const unsigned long long per_block = n / gridDim.x, per_stream = per_block / 512;
    unsigned long long* base = out + (unsigned long long)blockIdx.x * per_block;
    const int r = threadIdx.x >> 5, l = threadIdx.x & 31;
    for (unsigned long long off = 0; off + 32 <= per_stream; off += 32)
        for (int p = r; p < 512; p += 32) base[(unsigned long long)p * per_stream + off + l] = off;
}
int g_place_k = -1;          // DSKGPU_PLACE (read once)
float place_probe_ms(void* p, size_t bytes) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return 0.f;
    float best = 1e30f;
    for (int i = 0; i < 3; ++i) {
        (void)hipEventRecord(a, 0);
        hipLaunchKernelGGL(k_place_probe, dim3(256), dim3(1024), 0, 0, static_cast<unsigned long long*>(p), (unsigned long long)(bytes / 8));
        (void)hipEventRecord(b, 0);
        (void)hipEventSynchronize(b);
        float ms = 0.f; (void)hipEventElapsedTime(&ms, a, b);
        if (i && ms < best) best = ms;
    }
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    return best;
}
}  // namespace

hipError_t placed_malloc(void** out, size_t bytes) {
    if (g_place_k < 0) { const char* e = getenv("DSKGPU_PLACE"); g_place_k = e ? atoi(e) : 0; }      // (dskgpu_create with DSKGPU_F_PLACE sets 8)
    size_t free_b = 0, total_b = 0;
    if (g_place_k < 2 || bytes < (size_t(1) << 28) || hipMemGetInfo(&free_b, &total_b) != hipSuccess) return hipMalloc(out, bytes);
    const int K = (int)std::min<size_t>((size_t)g_place_k, free_b / 2 / bytes);      // candidates held at once: at most half of what is free
    if (K < 2) return hipMalloc(out, bytes);
    std::vector<void*> cand; std::vector<float> ms;
    for (int i = 0; i < K; ++i) {
        void* q = nullptr;
        if (hipMalloc(&q, bytes) != hipSuccess) { (void)hipGetLastError(); break; }
        static const size_t probe_max = getenv("DSKGPU_PLACE_GB") ? (size_t)(atof(getenv("DSKGPU_PLACE_GB")) * (1ull << 30)) : ~size_t(0);
        cand.push_back(q); ms.push_back(place_probe_ms(q, std::min(bytes, probe_max)));
    }
    if (cand.empty()) return hipErrorOutOfMemory;
    size_t best = 0;
    for (size_t i = 1; i < cand.size(); ++i) if (ms[i] < ms[best]) best = i;
    for (size_t i = 0; i < cand.size(); ++i) if (i != best) (void)hipFree(cand[i]);
    if (getenv("DSKGPU_VERBOSE")) {
        fprintf(stderr, "[dskgpu] placement of %.2f GB: probe ms", bytes * 1e-9);
        for (size_t i = 0; i < cand.size(); ++i) fprintf(stderr, " %.3f%s", ms[i], i == best ? "*" : "");
        fprintf(stderr, "\n");
    }
    *out = cand[best];
    return hipSuccess;
}

namespace {

// everything the host wants to know after the count stage of a pass, gathered into ONE 80-byte record: seven 4- and 32-byte copies from
// four buffers into pageable host memory cost ~20 us of idle GPU each (the runtime stages every one of them), 0.12 ms of a 14 ms step
__global__ void k_gather_back(const u32* __restrict__ sc, const u32* __restrict__ nsolid_total, const u32* __restrict__ nk, const u64* __restrict__ gstats,
                              u64* __restrict__ out) {
    if (threadIdx.x == 0) {
        out[0] = sc[SC_OVERFLOW]; out[1] = *nsolid_total; out[2] = nk ? *nk : 0u; out[3] = sc[SC_OVF2]; out[4] = sc[SC_OVF1]; out[5] = sc[SC_EXT];
        out[6] = gstats[0]; out[7] = gstats[1]; out[8] = gstats[2]; out[9] = gstats[3];
    }
}
// start of a pass attempt: the device scalars (from kernel arguments), an empty abundance histogram, zeroed statistics -- one launch where a
// copy and two memsets were four (a memset of 80 008 bytes is two fill kernels)
struct ScalarSet { u32 v[SC_COUNT]; };
// (zero / nzero: the level-2 region fill counts, zeroed here as well when the pass takes the fixed-capacity regions)
__global__ __launch_bounds__(256) void k_setup_pass(u32* __restrict__ sc, ScalarSet h, u64* __restrict__ ghist, u32 nh, u64* __restrict__ gstats, u32 nstats,
                                                    u32* __restrict__ zero, u64 nzero) {
    const u32 t = blockIdx.x * 256 + threadIdx.x;
    if (t < SC_COUNT) sc[t] = h.v[t];
    if (t < nstats) gstats[t] = 0ull;
    for (u32 i = t; i < nh; i += gridDim.x * 256) ghist[i] = 0ull;
    for (u64 i = t; i < nzero; i += (u64)gridDim.x * 256) zero[i] = 0u;
}
}  // namespace

namespace {

// Pinned host memory for the small read-backs a step waits on (a copy into pageable memory is staged by the runtime: ~10 us more of idle
// GPU per host round trip).  nullptr when the allocation fails or the request is larger: the caller then copies into its own buffer.
#define LAND_BYTES (64u << 10)
void* landing(dskgpu_ctx* ctx, size_t bytes) {
    if (bytes > LAND_BYTES) return nullptr;
    if (!ctx->land && hipHostMalloc(reinterpret_cast<void**>(&ctx->land), LAND_BYTES, hipHostMallocDefault) != hipSuccess) { ctx->land = nullptr; (void)hipGetLastError(); }
    return ctx->land;
}

// Is the all-ones key (the pad / empty-slot sentinel) the mixed form of a real canonical k-mer of this k?
// (It never is for k <= 32; for wider keys it is checked here once and the sentinel-based paths are switched off if so.)
bool sentinel_is_a_kmer(int W, unsigned k) {
    u64 v[4] = {0, 0, 0, 0};
    if (W == 1) v[0] = kunmix(~0ull);
    else if (W == 2) { KN<2> x; x.w[0] = x.w[1] = ~0ull; kunmixN(x); v[0] = x.w[0]; v[1] = x.w[1]; }
    else { KN<4> x; for (int i = 0; i < 4; ++i) x.w[i] = ~0ull; kunmixN(x); for (int i = 0; i < 4; ++i) v[i] = x.w[i]; }
    auto base = [&](const u64* a, unsigned i) { return (unsigned)((a[i >> 5] >> (2 * (i & 31))) & 3u); };   // base i counted from the LAST base
    for (unsigned i = k; i < 128; ++i) if (base(v, i)) return false;          // does not fit in 2k bits
    u64 r[4] = {0, 0, 0, 0};                                                  // reverse complement
    for (unsigned i = 0; i < k; ++i) { const unsigned c = base(v, i) ^ 2u, j = k - 1 - i; r[j >> 5] |= (u64)c << (2 * (j & 31)); }
    for (int x = 3; x >= 0; --x) if (v[x] != r[x]) return v[x] < r[x];        // canonical iff value <= its reverse complement
    return true;
}


// ---- K1 launcher
int run_encode(dskgpu_ctx* ctx, const uint8_t* d_bytes, u64 n, u64* nwords_out) {
    const u64 nwords = (n + 31) / 32;
    ctx->enc_fresh = false;
    CK(ctx->packed.ensure((nwords + 1) * 8));
    CK(ctx->inval.ensure((nwords + 1) * 4));
    if (const int rc = encode_into(ctx, d_bytes, n, ctx->packed.as<u64>(), ctx->inval.as<u32>())) return rc;
    *nwords_out = nwords;
    return DSKGPU_OK;
}

}  // namespace

// the 2-bit form of the context's current reads: encoded now, or kept from dskgpu_encode_reads (the ASCII bytes may be gone by then)
int encode_current(dskgpu_ctx* ctx, u64* nwords_out) {
    if (ctx->enc_keep) { *nwords_out = (ctx->n_bytes + 31) / 32; ctx->enc_fresh = false; return DSKGPU_OK; }
    if (!ctx->d_reads && ctx->n_bytes) return fail(ctx, DSKGPU_E_STATE, "the reads were released (dskgpu_encode_reads) and their 2-bit form has been overwritten: set the reads again");
    return run_encode(ctx, ctx->d_reads, ctx->n_bytes, nwords_out);
}

// ---- K1 into buffers of the caller's choice: the context's own (run_encode) or a query's (query.hip)
int encode_into(dskgpu_ctx* ctx, const uint8_t* d_bytes, u64 n, u64* packed, u32* inval) {
    const u64 nwords = (n + 31) / 32;
    if (!nwords) return DSKGPU_OK;
    const u64 nb = (nwords + 255) / 256;
    const unsigned grid = (unsigned)std::min<u64>(nb, (u64)ctx->num_cu * 16);
    if ((reinterpret_cast<uintptr_t>(d_bytes) & 15) == 0)
        hipLaunchKernelGGL(k_encode<true>, dim3(grid), dim3(256), 0, ctx->stream, d_bytes, n, packed, inval, nwords);
    else
        hipLaunchKernelGGL(k_encode<false>, dim3(grid), dim3(256), 0, ctx->stream, d_bytes, n, packed, inval, nwords);
    CKL("k_encode");
    return DSKGPU_OK;
}

// ---- scan launcher: exclusive scan of a[0..*d_len) in place, total -> a[*d_len]
int run_scan(dskgpu_ctx* ctx, u32* a, const u32* d_len, u64 max_len) {
    const u64 nb = std::max<u64>(1, (max_len + SCAN_BLK - 1) / SCAN_BLK);
    CK(ctx->sums.ensure((nb + 1) * 4));
    hipLaunchKernelGGL(k_scan_reduce, dim3((unsigned)nb), dim3(SCAN_NT), 0, ctx->stream, a, d_len, ctx->sums.as<u32>());
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, ctx->stream, ctx->sums.as<u32>(), d_len, a);
    hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nb), dim3(SCAN_NT), 0, ctx->stream, a, d_len, ctx->sums.as<u32>());
    CKL("k_scan");
    return DSKGPU_OK;
}

// Kernels that stage a whole tile need more dynamic LDS than the 64 KB default: raise the limit once per context
// (a context is bound to one device and driven by one thread, so no process-wide flag is involved).
int allow_big_lds(dskgpu_ctx* ctx, const void* fn, int bytes) {
    for (const void* f : ctx->big_lds_fns) if (f == fn) return DSKGPU_OK;
    CK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    ctx->big_lds_fns.push_back(fn);
    return DSKGPU_OK;
}

namespace {

size_t scatter_lds(int W, u32 P, bool opt = false) { return (size_t)SC_NT * (16 / W) * 8 * W + (size_t)P * (opt ? 20 : 16) + 4 + 17 * 4 + 16 + (opt ? 8 + L0_MAX_PASSES * 8 : 0); }   // opt: + the slice ends (+ the region bases of a level-0 sweep)

template <int W, int SRC, int MODE>
int launch_hist_m(dskgpu_ctx* ctx, const typename KeyT<W>::T* keys, const ChunkDesc* descs, const u32* d_nch,
                  u64 max_chunks, u32* matrix, DigitSpec ds, u32 P) {
    const unsigned grid = (unsigned)std::max<u64>(1, std::min<u64>(max_chunks, (u64)ctx->num_cu));
    hipLaunchKernelGGL((k_hist<W, SRC, MODE>), dim3(grid), dim3(SC_NT), 0, ctx->stream, ctx->packed.as<u64>(),
                       ctx->inval.as<u32>(), keys, descs, d_nch, matrix, (int)ctx->cfg.kmer_size, ds, P);
    CKL("k_hist");
    return DSKGPU_OK;
}
// digit modes in use: reads -> owner (0) or level 1 (1); key array -> level 1 (1, multi-GPU receive side) or level 2 (2)
template <int W, int SRC>
int launch_hist(dskgpu_ctx* ctx, const typename KeyT<W>::T* keys, const ChunkDesc* descs, const u32* d_nch,
                u64 max_chunks, u32* matrix, DigitSpec ds, u32 P) {
    const bool mp = ds.mode == 1 && ds.npass > 1;     // level 1 of a multi-pass count: instantiation with the pass filter
    if (SRC == 0) return ds.mode == 0 ? launch_hist_m<W, 0, 0>(ctx, keys, descs, d_nch, max_chunks, matrix, ds, P)
                       : mp ? launch_hist_m<W, 0, 3>(ctx, keys, descs, d_nch, max_chunks, matrix, ds, P)
                            : launch_hist_m<W, 0, 1>(ctx, keys, descs, d_nch, max_chunks, matrix, ds, P);
    return ds.mode == 2 ? launch_hist_m<W, 1, 2>(ctx, keys, descs, d_nch, max_chunks, matrix, ds, P)
                   : mp ? launch_hist_m<W, 1, 3>(ctx, keys, descs, d_nch, max_chunks, matrix, ds, P)
                        : launch_hist_m<W, 1, 1>(ctx, keys, descs, d_nch, max_chunks, matrix, ds, P);
}

unsigned scatter_grid(const dskgpu_ctx* ctx, int W, u32 P, u64 max_chunks, bool opt = false) {
    const size_t lds = scatter_lds(W, P, opt);
    const u64 per_cu = std::max<u64>(1, std::min<u64>(2048 / SC_NT, (160 * 1024) / lds));   // resident blocks per CU
    return (unsigned)std::max<u64>(1, std::min<u64>(max_chunks, (u64)ctx->num_cu * per_cu));
}
// SRC 0: the encoded reads; 1: a key array; 2: super-k-mer records (ctx->rec_src: the histogram-free level 1 of one- and two-word keys)
template <int W, int SRC, int MODE, bool OPT = false, bool HEAVY = false>
int launch_scatter_m(dskgpu_ctx* ctx, const typename KeyT<W>::T* keys, const ChunkDesc* descs, const u32* d_nch,
                     u64 max_chunks, const u32* scanned, typename KeyT<W>::T* out, DigitSpec ds, u32 P, Opt1Spec o1 = Opt1Spec{nullptr, 0u, 0u, nullptr, nullptr, 0u, nullptr, nullptr, nullptr, 0u, nullptr, 0ull, {0ull, 0ull, 0ull, 0ull}, 0u}) {
    const size_t lds = scatter_lds(W, P, OPT && !o1.uslice);
    const unsigned grid = scatter_grid(ctx, W, P, max_chunks, OPT && !o1.uslice);
    { const int e = allow_big_lds(ctx, reinterpret_cast<const void*>(&k_scatter<W, SRC, MODE, OPT, HEAVY>)); if (e) return e; }
    hipLaunchKernelGGL((k_scatter<W, SRC, MODE, OPT, HEAVY>), dim3(grid), dim3(SC_NT), lds, ctx->stream, SRC == 2 ? ctx->rec_src : ctx->packed.as<u64>(),
                       SRC == 2 ? nullptr : ctx->inval.as<u32>(), keys, descs, d_nch, scanned, out, (int)ctx->cfg.kmer_size, ds, P, o1);
    CKL("k_scatter");
    return DSKGPU_OK;
}
// key-array source with aligned write-out (k_scatter_al) when its LDS footprint fits one CU
template <int W, int MODE, bool OPT = false, bool SLICED = false>
int launch_scatter_al(dskgpu_ctx* ctx, const typename KeyT<W>::T* keys, const ChunkDesc* descs, const u32* d_nch,
                      u64 max_chunks, const u32* scanned, typename KeyT<W>::T* out, DigitSpec ds, u32 P, OptSpec os = OptSpec{0u, nullptr, nullptr, nullptr, 0u, 0u, 0ull, 0u, 0u, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}) {
    const size_t lds = ascatter_lds(W, P);
    const unsigned grid = (unsigned)std::max<u64>(1, std::min<u64>(max_chunks, (u64)ctx->num_cu));
    { const int e = allow_big_lds(ctx, reinterpret_cast<const void*>(&k_scatter_al<W, MODE, OPT, SLICED>)); if (e) return e; }
    hipLaunchKernelGGL((k_scatter_al<W, MODE, OPT, SLICED>), dim3(grid), dim3(SC_NT), lds, ctx->stream, keys, descs, d_nch, scanned, out, ds, P, os);
    CKL("k_scatter_al");
    return DSKGPU_OK;
}

template <int W, int SRC>
int launch_scatter(dskgpu_ctx* ctx, const typename KeyT<W>::T* keys, const ChunkDesc* descs, const u32* d_nch,
                   u64 max_chunks, const u32* scanned, typename KeyT<W>::T* out, DigitSpec ds, u32 P) {
    const bool mp = ds.mode == 1 && ds.npass > 1;
    if (SRC == 1 && ascatter_lds(W, P) <= 160 * 1024 && !ctx->tune.no_aligned)
        return ds.mode == 2 ? launch_scatter_al<W, 2>(ctx, keys, descs, d_nch, max_chunks, scanned, out, ds, P)
                       : mp ? launch_scatter_al<W, 3>(ctx, keys, descs, d_nch, max_chunks, scanned, out, ds, P)
                            : launch_scatter_al<W, 1>(ctx, keys, descs, d_nch, max_chunks, scanned, out, ds, P);
    if (SRC == 0) return ds.mode == 0 ? launch_scatter_m<W, 0, 0>(ctx, keys, descs, d_nch, max_chunks, scanned, out, ds, P)
                       : mp ? launch_scatter_m<W, 0, 3>(ctx, keys, descs, d_nch, max_chunks, scanned, out, ds, P)
                            : launch_scatter_m<W, 0, 1>(ctx, keys, descs, d_nch, max_chunks, scanned, out, ds, P);
    return ds.mode == 2 ? launch_scatter_m<W, 1, 2>(ctx, keys, descs, d_nch, max_chunks, scanned, out, ds, P)
                   : mp ? launch_scatter_m<W, 1, 3>(ctx, keys, descs, d_nch, max_chunks, scanned, out, ds, P)
                        : launch_scatter_m<W, 1, 1>(ctx, keys, descs, d_nch, max_chunks, scanned, out, ds, P);
}

// fixed-capacity regions or exact offsets: a compile-time switch of the count kernels (k_count1 / k_count_mw)
inline void launch_count_impl(dskgpu_ctx* ctx, unsigned grid, u64* keys, u64* solid_keys, u32* solid_ab, u32* ovf, const CountParams& cp) {
    if (cp.cap && cp.cap <= CNT_V3_KEYS * CNT_NT) {      // regions: the list-free kernel
        hipLaunchKernelGGL((k_count1v3<CNT_NT, CNT_KPT, CNT_V3_KEYS>), dim3(grid), dim3(CNT_NT), 0, ctx->stream, keys, solid_keys, solid_ab,
                           ctx->nsolid.as<u32>(), ctx->ghist.as<u64>(), ctx->gstats.as<u64>(), ovf, cp, cp.subcnt);
        return;
    }
    if (cp.cap) hipLaunchKernelGGL(k_count1<true>, dim3(grid), dim3(CNT_NT), 0, ctx->stream, keys, solid_keys, ctx->fstart.as<u32>(), solid_ab,
                                   ctx->nsolid.as<u32>(), ctx->ghist.as<u64>(), ctx->gstats.as<u64>(), ovf, cp, cp.subcnt);
    else hipLaunchKernelGGL(k_count1<false>, dim3(grid), dim3(CNT_NT), 0, ctx->stream, keys, solid_keys, ctx->fstart.as<u32>(), solid_ab,
                            ctx->nsolid.as<u32>(), ctx->ghist.as<u64>(), ctx->gstats.as<u64>(), ovf, cp, (const u32*)ctx->fstart.as<u32>());
}
template <int W>
inline void launch_count_impl(dskgpu_ctx* ctx, unsigned grid, KN<W>* keys, KN<W>* solid_keys, u32* solid_ab, u32* ovf, const CountParams& cp) {
    if constexpr (W == 2) {
        if (cp.cap && cp.cap <= C2V_NKEYS * CNT_NT && !ctx->mw_v3_off) {      // regions: the table keyed by the mixed top word
            CountParams c2 = cp; c2.maxload = std::min<u32>(cp.maxload, C2V_MAXLOAD);
            hipLaunchKernelGGL((k_count2v3<CNT_NT, C2V_KPT, C2V_NKEYS>), dim3(grid), dim3(CNT_NT), 0, ctx->stream, (const K2*)keys, solid_keys, solid_ab,
                               ctx->nsolid.as<u32>(), ctx->ghist.as<u64>(), ctx->gstats.as<u64>(), ovf, c2, cp.subcnt);
            return;
        }
    }
    if (cp.cap) hipLaunchKernelGGL((k_count_mw<W, true>), dim3(grid), dim3(CNT_NT), 0, ctx->stream, keys, solid_keys, ctx->fstart.as<u32>(), solid_ab,
                                   ctx->nsolid.as<u32>(), ctx->ghist.as<u64>(), ctx->gstats.as<u64>(), ovf, cp);
    else hipLaunchKernelGGL((k_count_mw<W, false>), dim3(grid), dim3(CNT_NT), 0, ctx->stream, keys, solid_keys, ctx->fstart.as<u32>(), solid_ab,
                            ctx->nsolid.as<u32>(), ctx->ghist.as<u64>(), ctx->gstats.as<u64>(), ovf, cp);
}
template <int W>
inline void launch_count(dskgpu_ctx* ctx, unsigned grid, typename KeyT<W>::T* keys, typename KeyT<W>::T* solid_keys, u32* solid_ab, u32* ovf, const CountParams& cp) {
    launch_count_impl(ctx, grid, keys, solid_keys, solid_ab, ovf, cp);
}

#ifndef OPT_GROUPS4
#define OPT_GROUPS4 OPT_GROUPS
#endif
#define CH2 65536u            // keys per level-2 chunk
#define OPT_GROUPS 545u
#define OPT_GROUPS2 1023u     // two-word keys: regions of 1023 groups of 64 B = 4092 keys (the count kernels are paced by their two barriers per
                              // sub-partition, not by its keys: half as many sub-partitions of twice the size -- see NOTEBOOK.md section 6 "k = 63")
inline u32 opt_groups(int W) { return W == 2 ? (AL_G2 == 8 ? 1022u : OPT_GROUPS2) : (W == 1 && AL_G1 == 16) ? 546u : W == 4 ? OPT_GROUPS4 : OPT_GROUPS; }      // (AL_G2 == 8, experiments: 511 groups of 128 B)
#define OPT_CAP 4360u          // segment-owned level-2 scatter: keys per sub-partition region (mean <= TARGET_KEYS).
                              // 545 groups of 64 B -- an ODD number, so the region starts (and the write fronts that advance
                              // through all regions in step) spread over every HBM channel instead of camping on a few

// (make_plan: planning.h)

// Build level-1 chunk descriptors on the host (ranges are static).
// unit = tile granularity of the source (Tile<W>::WORDS words or Tile<W>::KEYS keys).
void build_descs1(dskgpu_ctx* ctx, u64 n_units_total, u64 tile, u64 max_chunks, u32* nch_out) {
    u64 tpc; const u64 nch = chunks1(n_units_total, tile, max_chunks, &tpc);      // (planning.h)
    ctx->h_descs1.resize(nch);
    for (u64 c = 0; c < nch; ++c) ctx->h_descs1[c] = chunk_desc1(c, nch, tpc, tile, n_units_total);
    *nch_out = (u32)nch;
}

// the same for records that arrive in slices (ctx->rec_slice_end): every slice gets its own chunks (a launch per slice walks
// them); h_slice_chunk[s] = first chunk of slice s
void build_descs1_slices(dskgpu_ctx* ctx, u64 tile, u64 max_chunks, u32* nch_out) {
    const size_t S = ctx->rec_slice_end.size();
    ctx->h_descs1.clear(); ctx->h_slice_chunk.assign(S + 1, 0);
    const u64 per_slice = std::max<u64>(1, max_chunks / S);
    u64 rb = 0;
    for (size_t sl = 0; sl < S; ++sl) {
        const u64 re = ctx->rec_slice_end[sl];
        ctx->h_slice_chunk[sl] = (u32)ctx->h_descs1.size();
        if (re > rb) {
            const u64 ntiles = (re - rb + tile - 1) / tile;
            u64 nch = std::min<u64>(ntiles, per_slice);
            const u64 tpc = (ntiles + nch - 1) / nch;
            nch = (ntiles + tpc - 1) / tpc;
            for (u64 c = 0; c < nch; ++c) {
                ChunkDesc d;
                d.begin = rb + c * tpc * tile; d.end = std::min<u64>(re, rb + (c + 1) * tpc * tile);
                d.flat_base = 0; d.stride = 0;                      // (only the histogram-free scatter reads these chunks)
                ctx->h_descs1.push_back(d);
            }
        }
        rb = re;
    }
    ctx->h_slice_chunk[S] = (u32)ctx->h_descs1.size();
    for (auto& d : ctx->h_descs1) d.stride = (u32)ctx->h_descs1.size();
    *nch_out = (u32)ctx->h_descs1.size();
}

// k-mers per chunk of received records (k_sk_count) -> chunk bases for the expansion, and the total.  Needed up front only when
// the caller did not pass the total (dskgpu_mg_count); otherwise only by paths that expand the records.
#define REC_RESIZE 1001            // expand_records: the k-mer total the pipeline was sized with was an estimate and is off -- ctx->rec_hint holds the real one
// the stream waits for the arrival of the slices up to `upto` (exclusive) -- in order, each once
// -> DSKGPU_OK, or DSKGPU_E_STATE once a gate has failed (the caller enqueues nothing that reads the records)
int rec_gate_upto(dskgpu_ctx* ctx, u32 upto) {
    if (!ctx->rec_gate) return DSKGPU_OK;
    const u32 n = (u32)ctx->rec_slice_end.size();
    for (; ctx->rec_gated < std::min(upto, n); ++ctx->rec_gated)
        if (ctx->rec_gate(ctx->rec_gate_user, ctx->rec_gated) != 0) ctx->rec_gate_failed = true;
    return ctx->rec_gate_failed ? fail(ctx, DSKGPU_E_STATE, "a slice of the exchange did not arrive (the caller's gate failed)") : DSKGPU_OK;
}
int rec_gate_all(dskgpu_ctx* ctx) { return rec_gate_upto(ctx, 0xFFFFFFFFu); }

int sk_sizes(dskgpu_ctx* ctx, u64* total_out) {
    const u64 nrec = ctx->rec_n; const u32 R = ctx->sender.sp.R;
    { const int e = rec_gate_all(ctx); if (e) return e; }      // (a sliced receive: every record has to be there)
    u64 nch = std::min<u64>((nrec + SKX_NT - 1) / SKX_NT, (u64)ctx->num_cu * 16);
    u64 rpc = (nrec + nch - 1) / nch;
    rpc = (rpc + SKX_NT - 1) / SKX_NT * SKX_NT;
    nch = (nrec + rpc - 1) / rpc;
    if (rpc * SK_MAXN >= 0xFFFFFFFFull) return fail(ctx, DSKGPU_E_ARG, "too many records per chunk");
    CK(ctx->sk_sums.ensure(nch * 4)); CK(ctx->sk_cbase.ensure(nch * 8));
    ctx->h_sk_sums.assign(nch, 0); ctx->h_sk_cbase.assign(nch, 0);
    hipLaunchKernelGGL(k_sk_count, dim3((unsigned)nch), dim3(SKX_NT), 0, ctx->stream, ctx->rec_src, nrec, R, (u32)rpc, ctx->sk_sums.as<u32>());
    CKL("k_sk_count");
    CK(hipMemcpyAsync(ctx->h_sk_sums.data(), ctx->sk_sums.p, nch * 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    u64 total = 0;
    for (u64 c = 0; c < nch; ++c) { ctx->h_sk_cbase[c] = total; total += ctx->h_sk_sums[c]; }
    CK(hipMemcpyAsync(ctx->sk_cbase.p, ctx->h_sk_cbase.data(), nch * 8, hipMemcpyHostToDevice, ctx->stream));
    ctx->rec_nch = nch; ctx->rec_rpc = rpc; ctx->rec_sized = true;
    *total_out = total;
    return DSKGPU_OK;
}

// records -> dense key array (only when the level-1 scatter cannot read the records itself: exact / multi-pass path)
template <int W>
int expand_records(dskgpu_ctx* ctx, u64 total) {
    typedef typename KeyT<W>::T Key;
    if (ctx->rec_expanded) return DSKGPU_OK;
    if (!ctx->rec_sized) {
        u64 real = 0;
        const int e = sk_sizes(ctx, &real);
        if (e) return e;
        if (real != total && ctx->rec_hint_est) { ctx->rec_hint = real; return REC_RESIZE; }      // the estimate sized the fast path only: once more with the real figure
        if (real != total) return fail(ctx, DSKGPU_E_ARG, "dskgpu_mg_count_sized: n_kmers does not match the k-mers inside the records");
    }
    { const int e = rec_gate_all(ctx); if (e) return e; }
    CK(ctx->sk_keys.ensure((total + 1) * sizeof(Key)));
    hipLaunchKernelGGL(k_sk_expand<W>, dim3((unsigned)ctx->rec_nch), dim3(SKX_NT), 0, ctx->stream, ctx->rec_src, ctx->rec_n, ctx->sender.sp.R,
                       (int)ctx->cfg.kmer_size, (u32)ctx->rec_rpc, ctx->sk_cbase.as<u64>(), ctx->sk_keys.as<Key>());
    CKL("k_sk_expand");
    ctx->rec_expanded = true;
    ctx->mark("mg_expand");
    return DSKGPU_OK;
}
template <> int expand_records<4>(dskgpu_ctx*, u64) { return DSKGPU_E_STATE; }      // records carry k <= 64 only

// Heavy k-mers of a pass (one-word keys): level-1 bins whose sampled load stands 20 % above the median hold a k-mer that alone is a
// large share of a bin.  k_collect_heavy gathers about HV_COLLECT sampled keys of up to HV_SLOTS such bins; a k-mer that makes up
// >= 5 % of a bin's collected keys is heavy: the HV_KEYS heaviest go to hv_buf = [keys | counts | rows], and the level-1
// scatter counts them apart.  `load` is reduced by what they take away (slice sizes, order of the level-2 segments).
// hv_buf (u64 words): [keys: HV_KEYS x W][counts: HV_KEYS][rows, word x of row r at (W + 1 + x) * HV_KEYS + r][abundances: HV_KEYS x u32]
template <int W> struct HvLayout { static constexpr size_t keys = 0, counts = (size_t)HV_KEYS * W, rows = (size_t)HV_KEYS * (W + 1), ab = (size_t)HV_KEYS * (2 * W + 1), words = (size_t)HV_KEYS * (2 * W + 2); };
template <int W>
int find_heavy(dskgpu_ctx* ctx, bool from_reads, const typename KeyT<W>::T* d_keys_in, u32 nts, const Plan& pl, std::vector<double>& load, u32* nheavy_out) {
    typedef typename KeyT<W>::T Key;
    struct HK { u64 w[W]; bool operator<(const HK& o) const { for (int x = W - 1; x >= 0; --x) if (w[x] != o.w[x]) return w[x] < o.w[x]; return false; }
                bool operator==(const HK& o) const { for (int x = 0; x < W; ++x) if (w[x] != o.w[x]) return false; return true; } };
    static_assert(sizeof(HK) == sizeof(Key), "host mirror of a device key");
    *nheavy_out = 0;
    const u32 P1 = pl.P1;
    std::vector<double> sorted(load);
    std::nth_element(sorted.begin(), sorted.begin() + P1 / 2, sorted.end());
    const double median = sorted[P1 / 2];
    std::vector<u32> flagged;
    for (u32 b = 0; b < P1; ++b) if (load[b] > 1.2 * median + 4096.0) flagged.push_back(b);
    if (ctx->tune.verbose) fprintf(stderr, "[dskgpu] find_heavy: median load %.0f, %zu bins above 1.2 x\n", median, flagged.size());
    if (flagged.empty()) return DSKGPU_OK;
    std::sort(flagged.begin(), flagged.end(), [&](u32 a, u32 b) { return load[a] > load[b]; });
    if (flagged.size() > HV_SLOTS) flagged.resize(HV_SLOTS);
    ctx->h_hv_lut.assign(P1, 0xFF);
    for (size_t f = 0; f < flagged.size(); ++f) ctx->h_hv_lut[flagged[f]] = (unsigned char)f;
    const size_t nf = flagged.size();
    CK(ctx->hv_lut.ensure(P1));
    const unsigned grid = (unsigned)std::min<u64>(nts, (u64)ctx->num_cu * 2);
    const size_t per_slot = (size_t)grid * HV_BLOCK_KEYS;
    CK(ctx->hv_collect.ensure((size_t)HV_SLOTS * per_slot * sizeof(Key) + (size_t)HV_SLOTS * grid * 4 + HV_SLOTS * 4));
    u32* d_kept = reinterpret_cast<u32*>(ctx->hv_collect.as<Key>() + (size_t)HV_SLOTS * per_slot);
    u32* d_step = d_kept + (size_t)HV_SLOTS * grid;
    // keep every step-th sampled key of a bin, so that about HV_COLLECT are collected (h_mom: the bin's keys in the sample)
    ctx->h_hv_step.assign(HV_SLOTS, 1);
    for (size_t f = 0; f < flagged.size(); ++f) ctx->h_hv_step[f] = (u32)std::max<u64>(1, ctx->h_mom[2 * (size_t)flagged[f]] / HV_COLLECT);
    CK(hipMemcpyAsync(ctx->hv_lut.p, ctx->h_hv_lut.data(), P1, hipMemcpyHostToDevice, ctx->stream));
    CK(hipMemcpyAsync(d_step, ctx->h_hv_step.data(), HV_SLOTS * 4, hipMemcpyHostToDevice, ctx->stream));
    u32* sc = ctx->scalars.as<u32>();
    const bool mp = pl.d1.npass > 1;
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(SC_NT), 0, ctx->stream, (const u64*)ctx->packed.as<u64>(), (const u32*)ctx->inval.as<u32>(), d_keys_in,
                           (const ChunkDesc*)ctx->smp_descs.as<ChunkDesc>(), (const u32*)(sc + SC_NCH_S), (int)ctx->cfg.kmer_size, pl.d1, P1,
                           (const unsigned char*)ctx->hv_lut.as<unsigned char>(), d_kept, ctx->hv_collect.as<Key>(), (const u32*)d_step);
    };
    if (from_reads) { if (mp) launch(k_collect_heavy<W, 0, 3>); else launch(k_collect_heavy<W, 0, 1>); }
    else { if (mp) launch(k_collect_heavy<W, 1, 3>); else launch(k_collect_heavy<W, 1, 1>); }
    CKL("k_collect_heavy");
    ctx->h_hv_cnt.resize(nf * grid);
    ctx->h_hv_coll.resize(nf * per_slot * W);
    CK(hipMemcpyAsync(ctx->h_hv_cnt.data(), d_kept, nf * grid * 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(ctx->h_hv_coll.data(), ctx->hv_collect.p, nf * per_slot * sizeof(Key), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    // candidates over all flagged bins: (estimated occurrences, key, bin); the HV_KEYS largest are counted apart
    struct Cand { double est; HK key; u32 bin; };
    std::vector<Cand> cands;
    for (size_t f = 0; f < nf; ++f) {
        HK* kk = reinterpret_cast<HK*>(ctx->h_hv_coll.data()) + f * per_slot;       // the blocks' kept keys, made dense in place
        u32 n = 0;
        for (unsigned g = 0; g < grid; ++g) {
            const u32 c = std::min<u32>(ctx->h_hv_cnt[f * grid + g], HV_BLOCK_KEYS);
            for (u32 i = 0; i < c; ++i) kk[n++] = kk[(size_t)g * HV_BLOCK_KEYS + i];
        }
        if (n < 256) continue;
        std::sort(kk, kk + n);
        const u32 bin = flagged[f];
        u32 found = 0;
        for (u32 i = 0; i < n;) {
            u32 j = i + 1;
            while (j < n && kk[j] == kk[i]) ++j;
            if ((u64)(j - i) * 20 >= n) { cands.push_back({load[bin] * (double)(j - i) / (double)n, kk[i], bin}); ++found; }     // >= 5 % of the bin's collected keys
            i = j;
        }
        if (ctx->tune.verbose) fprintf(stderr, "[dskgpu]   bin %u load %.0f: %u keys collected, %u dominant\n", bin, load[bin], n, found);
    }
    std::sort(cands.begin(), cands.end(), [](const Cand& a, const Cand& b) { return a.est > b.est; });
    if (cands.size() > HV_KEYS) cands.resize(HV_KEYS);
    ctx->h_hv_keys.assign((size_t)HV_KEYS * W, DSK_EMPTY);
    for (size_t x = 0; x < cands.size(); ++x) {
        for (int y = 0; y < W; ++y) ctx->h_hv_keys[x * W + y] = cands[x].key.w[y];
        load[cands[x].bin] -= cands[x].est;            // they never reach the bin: slices and the order of the level-2 segments follow
    }
    u32 nheavy = (u32)cands.size();
    if (nheavy) {      // keys all-ones (= unused), counts zero, then the heavy keys
        CK(ctx->hv_buf.ensure(HvLayout<W>::words * 8));
        u64* hvb = ctx->hv_buf.as<u64>();
        CK(hipMemsetAsync(hvb + HvLayout<W>::keys, 0xFF, (size_t)HV_KEYS * W * 8, ctx->stream));
        CK(hipMemsetAsync(hvb + HvLayout<W>::counts, 0, HV_KEYS * 8, ctx->stream));
        CK(hipMemcpyAsync(hvb + HvLayout<W>::keys, ctx->h_hv_keys.data(), (size_t)HV_KEYS * W * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    *nheavy_out = nheavy;
    return DSKGPU_OK;
}

// ---------------- one pass, stage by stage
// A pass's key source: the encoded reads, a key array, or (multi-GPU receive side) super-k-mer records that the histogram-free
// level-1 scatter reads directly; any other path expands them to a key array first, once for all attempts of the pass.
template <int W> struct KeySource { bool from_reads, from_rec; const typename KeyT<W>::T* keys; u64 nkeys, nwords; };

// What the stages of one attempt of a pass share
template <int W>
struct PassState {
    typedef typename KeyT<W>::T Key;
    KeySource<W>& src;
    u32 pass, npass; u64 cap;        // which pass of how many; the keys it may hold
    u64 nvalid;                      // keys of all passes: the valid k-mer windows of the reads, or the key array's length
    u32* sc;                         // the device scalars (Scalar)
    Plan pl{};
    u32 opt_cap = 0, max_ext = 0; u64 nregions = 0;      // level 2: keys per sub-partition region (0 = exact offsets); extension regions behind them
    bool opt1 = false; Opt1Spec o1{}; unsigned grid1 = 0;  // level 1 without a histogram pass (block-owned slices)
    u32 nch1 = 0, nheavy = 0;        // level-1 chunks; k-mers the level-1 scatter counts apart (find_heavy)
    std::vector<double> load, spread;   // level-1 keys per bin (sampled or mean) and how far a block's share of them may stray
    Key* fkeys = nullptr;            // the keys after the last scatter, grouped by sub-partition
    DevBuf* scratch = nullptr;       // the free ping-pong buffer
    Key* solid_keys = nullptr; u32* solid_ab = nullptr;      // where the count kernels put the solid rows
    // the count's read-back (k_gather_back): overflow flags, solid rows, keys of the pass (exact paths), slice / region overflows,
    // extension regions used, gstats (distinct, heavy rows, keys level 1 placed, ..)
    u32 flags = 0, nsolid = 0, nkeys = 0, ovf2 = 0, ovf1 = 0, ext = 0; u64 stats[4] = {0, 0, 0, 0};
    bool too_big = false; u64 rows = 0;      // the exact level 1 counted more than `cap` keys (nkeys); rows the pass left
};

template <int W>
int upload_descs1(dskgpu_ctx* ctx, PassState<W>& ps) {
    const KeySource<W>& src = ps.src;
    const u64 max_chunks1 = (u64)ctx->num_cu * 8;
    if (src.from_reads) build_descs1(ctx, src.nwords, Tile<W>::WORDS, max_chunks1, &ps.nch1);
    else if (src.from_rec && ctx->rec_slice_end.size() > 1) build_descs1_slices(ctx, RecTile<W>::NR, max_chunks1, &ps.nch1);
    else if (src.from_rec) build_descs1(ctx, ctx->rec_n, RecTile<W>::NR, max_chunks1, &ps.nch1);
    else build_descs1(ctx, src.nkeys, Tile<W>::KEYS, max_chunks1, &ps.nch1);
    CK(ctx->descs1.ensure(ctx->h_descs1.size() * sizeof(ChunkDesc)));
    CK(hipMemcpyAsync(ctx->descs1.p, ctx->h_descs1.data(), ctx->h_descs1.size() * sizeof(ChunkDesc), hipMemcpyHostToDevice, ctx->stream));
    return DSKGPU_OK;
}

// leave the records path: expand once, then it is a key array
template <int W>
int records_to_keys(dskgpu_ctx* ctx, PassState<W>& ps) {
    const int e = expand_records<W>(ctx, ps.src.nkeys);
    if (e) return e;
    ps.src.keys = ctx->sk_keys.template as<typename KeyT<W>::T>(); ps.src.from_rec = false;
    return upload_descs1(ctx, ps);
}

// A positional sample: the digit histogram of <= 1024 tiles spread evenly over `units` (hist(descs, d_nch, n, matrix) launches it),
// reduced to (sum, sum of squares) of every bin over the tiles in ctx->h_mom.  -> tiles of the source, tiles sampled, sampled keys
template <class Hist>
int positional_sample(dskgpu_ctx* ctx, u64 units, u64 tile, u32 P, Hist&& hist, u64* ntiles_out, u64* nts_out, u64* stot_out) {
    u32* sc = ctx->scalars.as<u32>();
    const u64 ntiles = std::max<u64>(1, (units + tile - 1) / tile);
    const u64 nts = std::min<u64>(ntiles, 1024);
    ctx->h_descs_s.resize(nts);
    for (u64 i = 0; i < nts; ++i) {
        const u64 t = i * ntiles / nts;
        ChunkDesc d; d.begin = t * tile; d.end = std::min<u64>(units, (t + 1) * tile); d.flat_base = (u32)i; d.stride = (u32)nts;
        ctx->h_descs_s[i] = d;
    }
    const u64 Ms = (u64)P * nts;
    CK(ctx->smp_descs.ensure(nts * sizeof(ChunkDesc)));
    CK(ctx->smp_mat.ensure((Ms + 4) * 4 + (size_t)P * 16));
    CK(hipMemcpyAsync(ctx->smp_descs.p, ctx->h_descs_s.data(), nts * sizeof(ChunkDesc), hipMemcpyHostToDevice, ctx->stream));
    ctx->h_sc[SC_NCH_S] = (u32)nts;
    CK(hipMemcpyAsync(sc + SC_NCH_S, &ctx->h_sc[SC_NCH_S], 4, hipMemcpyHostToDevice, ctx->stream));
    { const int e = hist(ctx->smp_descs.as<ChunkDesc>(), (const u32*)(sc + SC_NCH_S), nts, ctx->smp_mat.as<u32>()); if (e) return e; }
    u64* mom = reinterpret_cast<u64*>(ctx->smp_mat.as<u32>() + ((Ms + 2) & ~(u64)1));
    hipLaunchKernelGGL(k_bin_moments, dim3((P + 3) / 4), dim3(256), 0, ctx->stream, (const u32*)ctx->smp_mat.as<u32>(), (u32)nts, P, mom);
    CKL("k_bin_moments");
    ctx->h_mom.resize((size_t)P * 2);
    void* lz = landing(ctx, (size_t)P * 16);
    CK(hipMemcpyAsync(lz ? lz : (void*)ctx->h_mom.data(), mom, (size_t)P * 16, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    if (lz) std::memcpy(ctx->h_mom.data(), lz, (size_t)P * 16);
    u64 stot = 0;
    for (u32 b = 0; b < P; ++b) stot += ctx->h_mom[2 * b];
    *ntiles_out = ntiles; *nts_out = nts; *stot_out = stot;
    return DSKGPU_OK;
}

// Stage 1, plan and region sizing.  One-word keys straight from the reads, one pass, two levels: both scatters run without a
// histogram pass (block-owned slices at level 1, segment-owned regions at level 2); any overflow sends the whole attempt back
// through the exact histogram + scan path.
template <int W>
int pass_plan(dskgpu_ctx* ctx, PassState<W>& ps, int extra_bits) {
    typedef typename KeyT<W>::T Key;
    Plan& pl = ps.pl;
    // keys the plan is sized for: the exact number of valid windows of a single pass from the reads; of several passes its share
    // + 2 % (cap holds 6 % head-room: sized for it, 7 passes of 200 M reads needed 1792 level-1 bins, more than the LDS of the
    // histogram-free level 1 holds)
    const u64 plan_n = (ps.src.from_reads && ctx->have_nvalid) ? std::min<u64>(ps.cap, ps.npass == 1 ? ps.nvalid + 1 : ps.nvalid / ps.npass + ps.nvalid / ps.npass / 50 + 4096) : ps.cap;
    if (!make_plan(plan_n, extra_bits, W, (u32)ctx->num_cu, &pl))
        return fail(ctx, DSKGPU_E_OVERFLOW, "cannot partition finer (table overflow persists)");
    pl.d1.world = pl.d2.world = ctx->cfg.world_size; pl.d1.npass = pl.d2.npass = ps.npass; pl.d1.pass = pl.d2.pass = ps.pass;
    pl.d1.ones_is_key = pl.d2.ones_is_key = ctx->sentinel_ok ? 0u : 1u;      // (k = 64, 128: no key array of this pass is padded, and the all-ones key in one is the k-mer)
    { const int e = upload_descs1(ctx, ps); if (e) return e; }
    if (pl.levels == 2 && ctx->sentinel_ok && !ctx->opt2_off && !ctx->tune.no_opt2 && ascatter_lds(W, pl.P2) <= 160 * 1024)
        ps.opt_cap = opt_groups(W) * (8u / W);                                                 // 545 (two-word keys: 1091) groups of 64 B
    if (ps.opt_cap && ctx->tune.opt_cap) ps.opt_cap = ctx->tune.opt_cap;                       // experiments / tests
    if (W > 1 && (u64)pl.F * ps.opt_cap >= 0xFFFF0000ull) ps.opt_cap = 0;                      // k_count<W> keeps 32-bit offsets
    const u32 opt_cap = ps.opt_cap;
    // extension regions behind the home regions (region chains, kernels.h): an eighth of the home regions + 4096; their offsets
    // inside the pool stay below 2^31.  Two-word keys (k_count_mw / k_count_chained_mw index keys with 32 bits): home regions
    // and pool together below 2^32 keys.  Four-word keys: none (tiles of 4096 keys: the scan over the bins dominates anyway).
    if (opt_cap && W <= 2) {
        u64 want = std::min<u64>((u64)pl.F / 8 + 4096, 0x7FFFFFFFull / opt_cap - 1);
        if (ctx->tune.max_ext >= 0) want = (u64)ctx->tune.max_ext;                                 // tests
        if (W > 1) { const u64 room = 0xFFFF0000ull / opt_cap; want = room > (u64)pl.F + 1 ? std::min<u64>(want, room - pl.F - 1) : 0; }
        ps.max_ext = (u32)want;
    }
    ps.nregions = (u64)pl.F + ps.max_ext;
    if (!opt_cap) { CK(ctx->bufA.ensure((ps.cap + 1) * sizeof(Key))); CK(ctx->bufB.ensure((ps.cap + 1) * sizeof(Key))); }      // exact offsets: the keys of the pass, twice
    if (opt_cap) {
        // the rows of the solid k-mers land at the region offsets too: abundances (one-word keys: in bufA, the free
        // ping-pong buffer) or keys + abundances (multi-word keys: bufA + abund2).  Size everything BEFORE level 1 writes bufA.
        const u64 slots = (u64)pl.F * opt_cap + ATile<W>::KEYS + 16;
        CK(ctx->bufA.ensure(std::max<u64>(W == 1 ? slots * 4 : slots * sizeof(Key), (ps.cap + 1) * sizeof(Key))));
        if (W > 1) CK(ctx->abund2.ensure(slots * 4));
    }
    ps.opt1 = opt_cap && !ctx->opt1_off && !ctx->tune.no_opt1 && (ps.npass == 1 || ps.src.from_reads || W <= 2);   // several passes over records / a key array (the multi-GPU receive side): one- and two-word keys
    if (ps.src.from_rec && (!ps.opt1 || W > 2 || ctx->tune.no_recsrc)) { const int e = records_to_keys(ctx, ps); if (e) return e; }
    if (ps.opt1 && scatter_lds(W, pl.P1, false) > 160 * 1024) ps.opt1 = false;
    return DSKGPU_OK;
}

// Stage 2, level-1 sample and slice layout (histogram-free level 1 only)
template <int W>
int pass_layout1(dskgpu_ctx* ctx, PassState<W>& ps) {
    typedef typename KeyT<W>::T Key;
    const KeySource<W>& src = ps.src;
    const Plan& pl = ps.pl;
    Opt1Spec& o1 = ps.o1;
    o1 = Opt1Spec{nullptr, 0u, 0u, ps.sc + SC_OVF1, nullptr, ctx->sender.sp.R, ctx->gstats.as<u64>() + 2, nullptr, nullptr, 0u, nullptr, 0ull, {0ull, 0ull, 0ull, 0ull}, 0u};
    // (the per-bin slice ends need 4 more bytes of LDS per bin: plans above 1634 level-1 bins keep UNIFORM slices, mean-sized, no sample)
    const bool uniform1 = scatter_lds(W, pl.P1, true) > 160 * 1024;
    if (ps.opt1) {
        const u32 nch1 = ps.nch1;
        const unsigned grid1 = ps.grid1 = scatter_grid(ctx, W, pl.P1, nch1, !uniform1);
        // a block's share of the input: it walks chunks blockIdx, blockIdx + grid, .. -- the busiest block's units over all units, from the
        // descriptors upload_descs1 has just built, nch1 of them (busiest_share1, planning.h: the last chunk may be short, so this is not
        // ceil(nch / grid) / nch)
        double share = busiest_share1(ctx->h_descs1.data(), nch1, grid1);
        if (src.from_rec && ctx->rec_slice_end.size() > 1) {      // a launch per slice: the busiest block's chunks of every slice add up
            share = 0.0;
            u64 rb = 0;
            for (size_t sl = 0; sl < ctx->rec_slice_end.size(); ++sl) {
                const u64 re = ctx->rec_slice_end[sl], nc = ctx->h_slice_chunk[sl + 1] - ctx->h_slice_chunk[sl];
                if (nc) share += (double)((nc + grid1 - 1) / grid1) / (double)nc * (double)(re - rb) / (double)ctx->rec_n;
                rb = re;
            }
        }
        // ---- level-1 loads of this pass, per bin ("PartiInfo" before the spill): a positional sample -- the level-1 digit
        // histogram of <= 1024 tiles spread over the source -- scaled to the pass.  Every bin's slices are sized from ITS load,
        // so a bin that holds a repeat family (or poly-A) gets longer slices instead of overflowing the mean-sized ones.
        // Records (multi-GPU receive side) have no histogram kernel: uniform loads.
        const double pass_keys = (double)(ps.nvalid / ps.npass);
        ps.load.assign(pl.P1, pass_keys / pl.P1);
        ps.spread.assign(pl.P1, 0.0);
        bool sampled = false;
        // records (the multi-GPU receive side, the passes of a record-based multi-pass count): a positional sample of the records is
        // expanded into a key array with pads (k_sk_sample_keys: SK_MAXN slots per candidate record) and sampled like any key array.
        // Records that arrive in slices: the sample comes from the first slice (the slices are positional cuts of every sender's
        // reads: alike), so only that slice has to have arrived.
        const Key* d_keys_s = src.keys;              // the key array the sample kernels read
        double smp_density = 1.0;                    // records: real keys per slot of the sample array (a level-1 tile is full, a sample tile is not)
        bool rec_sample_ok = ctx->sentinel_ok;       // (the sample array is padded with the all-ones key, which the key-array kernels skip: only when it is no k-mer of this k)
        u64 rec_units = 0;
        if constexpr (W <= 2) {
          if (src.from_rec && !ctx->tune.no_sample && !uniform1) {
            const u64 nrec_s = ctx->rec_slice_end.size() > 1 ? ctx->rec_slice_end[0] : ctx->rec_n;
            const u64 NR = RecTile<W>::NR;
            const u64 nchk_all = (nrec_s + NR - 1) / NR;
            const u64 nchk = std::min<u64>(nchk_all, 256);
            if (nchk == 0) rec_sample_ok = false;
            else {
                { const int e = rec_gate_upto(ctx, 1); if (e) return e; }
                std::vector<u64>& cbeg = ctx->h_cbeg;        // (the context's: it outlives the asynchronous copy below; the next use is behind this pass's next synchronisation)
                cbeg.resize(nchk);
                for (u64 i = 0; i < nchk; ++i) cbeg[i] = (i * nchk_all / nchk) * NR;
                rec_units = nchk * NR * SK_MAXN;
                CK(ctx->smp_keys.ensure(rec_units * sizeof(Key) + nchk * 8 + 64));
                u64* d_cbeg = reinterpret_cast<u64*>(ctx->smp_keys.as<char>() + rec_units * sizeof(Key));
                CK(hipMemcpyAsync(d_cbeg, cbeg.data(), nchk * 8, hipMemcpyHostToDevice, ctx->stream));
                hipLaunchKernelGGL(k_sk_sample_keys<W>, dim3((unsigned)nchk), dim3(SKX_NT), 0, ctx->stream, ctx->rec_src, ctx->rec_n, ctx->sender.sp.R, (int)ctx->cfg.kmer_size,
                                   (const u64*)d_cbeg, (u32)NR, ctx->smp_keys.as<Key>());
                CKL("k_sk_sample_keys");
                d_keys_s = ctx->smp_keys.as<Key>();
            }
          }
        }
        const bool smp_rec = src.from_rec && rec_units != 0;
        if ((!src.from_rec || smp_rec) && rec_sample_ok && !ctx->tune.no_sample && !uniform1) {
            const u64 units = src.from_reads ? src.nwords : smp_rec ? rec_units : src.nkeys, tile = src.from_reads ? Tile<W>::WORDS : Tile<W>::KEYS;
            auto hist = [&](const ChunkDesc* dd, const u32* d_nch, u64 n, u32* mat) {
                return src.from_reads ? launch_hist<W, 0>(ctx, nullptr, dd, d_nch, n, mat, pl.d1, pl.P1) : launch_hist<W, 1>(ctx, d_keys_s, dd, d_nch, n, mat, pl.d1, pl.P1);
            };
            u64 ntiles = 0, nts = 0, stot = 0;
            { const int e = positional_sample(ctx, units, tile, pl.P1, hist, &ntiles, &nts, &stot); if (e) return e; }
            if (stot >= (u64)pl.P1 * 64) {        // enough sampled keys to say something per bin
                // one pass from the reads: scaled so that the loads add up to the exact number of valid k-mers; otherwise by position
                const double scale = (src.from_reads && ps.npass > 1) ? (double)ntiles / (double)nts : pass_keys / (double)stot;
                // tiles a block walks (the busiest one), and how far a bin's keys on those tiles may be from share * load:
                //   the block's own spread: 5 sigma of the sum over its tiles of the per-tile count (variance measured on the sample),
                //   the estimate's error  : 4 sigma of the sampled sum, scaled to the block's share
                // (records: a level-1 tile is full, a tile of the sample array holds smp_density of its slots: the block walks
                //  pass_keys * share / KEYS full tiles, each with 1 / density times the variance of a sample tile)
                if (smp_rec) smp_density = std::max(0.05, (double)stot / ((double)nts * (double)Tile<W>::KEYS));
                const double tiles_per_block = smp_rec ? pass_keys * share / (double)Tile<W>::KEYS : (double)ntiles * share;
                for (u32 b = 0; b < pl.P1; ++b) {
                    const double sum = (double)ctx->h_mom[2 * b], sq = (double)ctx->h_mom[2 * b + 1];
                    const double mean = sum / (double)nts, var = std::max(mean, sq / (double)nts - mean * mean);      // (at least Poisson)
                    ps.load[b] = sum * scale;
                    ps.spread[b] = 5.0 * std::sqrt(tiles_per_block * var / smp_density) + 4.0 * std::sqrt((double)nts * var) * scale * share;
                }
                sampled = true;
            }
            // ---- a k-mer that alone is a large share of a level-1 bin (poly-A reads, a satellite: millions of occurrences):
            // its bin stands far above the others.  Collect sampled keys of those bins, find the dominant k-mer(s) on the host
            // and let the level-1 scatter count them apart (k_scatter<.., HEAVY>) -- everything lighter is what the region
            // chains are for.
            if constexpr (W <= 2) {
                if (sampled && ps.opt_cap && !ctx->tune.no_heavy) { const int e = find_heavy<W>(ctx, src.from_reads, d_keys_s, (u32)nts, pl, ps.load, &ps.nheavy); if (e) return e; }
            }
            ctx->mark("sample1");
        }
        // slice of bin b = the busiest block's share of its load + the spread above + 1 % + 64 keys; without a sample: + 6 % + 160
        // (what uniform reads need), in whole groups of 8 keys
        ctx->h_boff.resize(pl.P1 + 1);
        u64 area = 0;
        if (uniform1) o1.uslice = 1u;          // (set below)
        for (u32 b = 0; b < pl.P1; ++b) {
            double sl = ps.load[b] * share;
            // (records: the senders' zero-length pad records sit at the ends of their slices, so a level-1 chunk holds anything from
            //  no pads to ~10 % -- a block that walks only a few chunks does not average that out: more room there)
            const double few = (src.from_rec && share * (double)nch1 < 16.0) ? 0.08 : 0.0;
            sl += sampled ? ps.spread[b] + sl * 0.01 + 64.0 : sl * (0.06 + few) + 160.0;
            u64 slice = ((u64)sl + 8) & ~7ull;
            if (uniform1) o1.uslice = (u32)slice;
            if (ctx->tune.opt_slice) slice = ctx->tune.opt_slice;                                        // experiments / tests
            ctx->h_boff[b] = (u32)std::min<u64>(area, 0xFFFFFFFFull); area += slice;
        }
        ctx->h_boff[pl.P1] = (u32)std::min<u64>(area, 0xFFFFFFFFull);
        const u64 tail = 2 * Tile<W>::KEYS;                         // the dump zone behind the last slice (a tile's keys of a bin that outgrew its slice land there)
        const u64 cells = (u64)pl.P1 * grid1;
        if (ctx->tune.verbose) fprintf(stderr, "[dskgpu] pass %u/%u: P1 %u P2 %u, %u level-1 blocks, area %llu keys per block (%.2f GB of slices), sampled %d, keys %llu, %u chunks, share %.6f, %zu slices\n", ps.pass, ps.npass, pl.P1, pl.P2, grid1,
                                       (unsigned long long)area, (double)area * grid1 * sizeof(Key) * 1e-9, (int)sampled, (unsigned long long)ps.nvalid, nch1, share, ctx->rec_slice_end.size());
        if (area < 8 || area * grid1 + tail >= 0xFFFF0000ull) ps.opt1 = false;
        else {
            o1.area = (u32)area; o1.dump = (u32)(area * grid1);
            CK(ctx->boff.ensure(((size_t)pl.P1 + 1) * 4));
            CK(hipMemcpyAsync(ctx->boff.p, ctx->h_boff.data(), ((size_t)pl.P1 + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
            o1.boff = ctx->boff.as<u32>();
            CK(ctx->mat1.ensure((cells + 1) * 4));                      // here: keys per (bin, block) slice
            o1.fill = ctx->mat1.as<u32>();
            if (grid1 + 1 > SLICED_MAX) ps.opt1 = false;                // the level-2 loader keeps the slice bounds in LDS
            CK(ctx->bufA.ensure((area * grid1 + tail + 1) * sizeof(Key)));
        }
    }
    if (src.from_rec && !ps.opt1) { const int e = records_to_keys(ctx, ps); if (e) return e; }
    return DSKGPU_OK;
}

// The histogram-free level-1 scatter: one launch, on (source, one or several passes, k-mers counted apart or not).  Records and
// heavy k-mers are one- and two-word keys only; so are several passes over a key array.
template <int W, int SRC, int MODE, bool HEAVY>
int scatter1_m(dskgpu_ctx* ctx, const PassState<W>& ps, const ChunkDesc* dd1, const u32* d_nch) {
    return launch_scatter_m<W, SRC, MODE, true, HEAVY>(ctx, SRC == 1 ? ps.src.keys : nullptr, dd1, d_nch, ps.nch1, nullptr, ctx->bufA.template as<typename KeyT<W>::T>(),
                                                       ps.pl.d1, ps.pl.P1, ps.o1);
}
template <int W>
int launch_scatter1(dskgpu_ctx* ctx, const PassState<W>& ps, const ChunkDesc* dd1, const u32* d_nch) {
    const bool mp = ps.npass > 1, heavy = ps.nheavy != 0, rec = ps.src.from_rec, reads = ps.src.from_reads;
    if constexpr (W <= 2) {
        if (rec && heavy) return mp ? scatter1_m<W, 2, 3, true>(ctx, ps, dd1, d_nch) : scatter1_m<W, 2, 1, true>(ctx, ps, dd1, d_nch);
        if (rec) return mp ? scatter1_m<W, 2, 3, false>(ctx, ps, dd1, d_nch) : scatter1_m<W, 2, 1, false>(ctx, ps, dd1, d_nch);
        if (heavy && reads) return mp ? scatter1_m<W, 0, 3, true>(ctx, ps, dd1, d_nch) : scatter1_m<W, 0, 1, true>(ctx, ps, dd1, d_nch);
        if (heavy) return mp ? scatter1_m<W, 1, 3, true>(ctx, ps, dd1, d_nch) : scatter1_m<W, 1, 1, true>(ctx, ps, dd1, d_nch);
        if (!reads && mp) return scatter1_m<W, 1, 3, false>(ctx, ps, dd1, d_nch);
    } else if (rec || heavy || (!reads && mp)) return DSKGPU_E_STATE;
    if (reads) return mp ? scatter1_m<W, 0, 3, false>(ctx, ps, dd1, d_nch) : scatter1_m<W, 0, 1, false>(ctx, ps, dd1, d_nch);
    return scatter1_m<W, 1, 1, false>(ctx, ps, dd1, d_nch);
}

// Stage 3, level-1 scatter: the pass's scalars, then the histogram-free scatter or the exact histogram + scan + scatter
// (which, for one of several passes, first checks that the pass fits its buffers: ps.too_big)
template <int W>
int pass_scatter1(dskgpu_ctx* ctx, PassState<W>& ps) {
    typedef typename KeyT<W>::T Key;
    const KeySource<W>& src = ps.src;
    const Plan& pl = ps.pl;
    const u32 nch1 = ps.nch1;
    const u64 M1 = (u64)pl.P1 * nch1;
    u32* h_sc = ctx->h_sc;
    std::memset(h_sc, 0, sizeof(ctx->h_sc));
    h_sc[SC_NCH1] = nch1; h_sc[SC_MLEN1] = (u32)M1; h_sc[SC_F] = pl.F;
    if (ps.opt1) h_sc[SC_NCH2] = pl.P1;                    // level-2 chunks = the level-1 bin regions
    h_sc[SC_WORK2] = (u32)std::min<u64>(pl.P1, (u64)ctx->num_cu);   // work counter of the segment-owned level-2 scatter: first segment not taken in the first round
    // (with them: histogram / distinct counters of THIS pass attempt -- a table-overflow retry must not double count)
    {
        static_assert(sizeof(ctx->h_sc) == sizeof(ScalarSet), "scalar block");
        ScalarSet hs; std::memcpy(hs.v, h_sc, sizeof hs.v);
        const u32 nh = ctx->cfg.histo_max + 1;
        u64 nzero = 0;
        if (pl.levels == 2 && ps.opt_cap) { nzero = ps.nregions + 1; CK(ctx->mat2.ensure((size_t)nzero * 4)); }      // level 2's keys per region (home regions, then the extension pool)
        const u64 work = std::max<u64>(nh, nzero);
        hipLaunchKernelGGL(k_setup_pass, dim3((unsigned)std::min<u64>(1024, (work + 255) / 256)), dim3(256), 0, ctx->stream, ps.sc, hs, ctx->ghist.as<u64>(), nh, ctx->gstats.as<u64>(), 4u,
                           nzero ? ctx->mat2.as<u32>() : (u32*)nullptr, nzero);
        CKL("k_setup_pass");
    }
    ctx->mark("setup");
    int rc;
    const ChunkDesc* dd1 = ctx->descs1.as<ChunkDesc>();
    if (ps.opt1) {
        Opt1Spec& o1 = ps.o1;
        if constexpr (W <= 2) { if (ps.nheavy) { o1.hv_keys = ctx->hv_buf.as<u64>() + HvLayout<W>::keys; o1.hv_cnt = reinterpret_cast<unsigned long long*>(ctx->hv_buf.as<u64>() + HvLayout<W>::counts); } }
        if (src.from_rec && ctx->rec_slice_end.size() > 1) {
            // the records arrive in slices: one launch per slice, each behind the arrival of its slice (rec_gate), the blocks'
            // write cursors parked in between
            const size_t S = ctx->rec_slice_end.size();
            CK(ctx->cur_state.ensure((size_t)ps.grid1 * pl.P1 * 4));
            o1.cur_state = ctx->cur_state.as<u32>();
            rc = DSKGPU_OK;
            for (size_t sl = 0; sl < S && rc == DSKGPU_OK; ++sl) {
                if ((rc = rec_gate_upto(ctx, (u32)sl + 1))) break;
                o1.g0 = ctx->h_slice_chunk[sl]; o1.gn = ctx->h_slice_chunk[sl + 1] - ctx->h_slice_chunk[sl];
                o1.resume = sl > 0 ? 1u : 0u; o1.last = sl + 1 == S ? 1u : 0u;
                rc = launch_scatter1<W>(ctx, ps, dd1, ps.sc + SC_NCH1);
            }
        }
        else if (src.from_rec) { if (!(rc = rec_gate_all(ctx))) rc = launch_scatter1<W>(ctx, ps, dd1, ps.sc + SC_NCH1); }
        else rc = launch_scatter1<W>(ctx, ps, dd1, ps.sc + SC_NCH1);
        if (rc) return rc;
        ctx->mark("scatter1");
        return DSKGPU_OK;
    }
    CK(ctx->mat1.ensure((M1 + 1) * 4));
    if (src.from_reads) rc = launch_hist<W, 0>(ctx, nullptr, dd1, ps.sc + SC_NCH1, nch1, ctx->mat1.as<u32>(), pl.d1, pl.P1);
    else rc = launch_hist<W, 1>(ctx, src.keys, dd1, ps.sc + SC_NCH1, nch1, ctx->mat1.as<u32>(), pl.d1, pl.P1);
    if (rc) return rc;
    ctx->mark("hist1");
    if ((rc = run_scan(ctx, ctx->mat1.as<u32>(), ps.sc + SC_MLEN1, M1))) return rc;
    ctx->mark("scan1");
    if (ps.npass > 1) {      // the pass must fit the buffers sized for it (skewed inputs can overfill one pass)
        CK(hipMemcpyAsync(&ps.nkeys, ctx->mat1.as<u32>() + M1, 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        if ((u64)ps.nkeys > ps.cap) { ps.too_big = true; return DSKGPU_OK; }
    }
    if (src.from_reads) rc = launch_scatter<W, 0>(ctx, nullptr, dd1, ps.sc + SC_NCH1, nch1, ctx->mat1.as<u32>(), ctx->bufA.as<Key>(), pl.d1, pl.P1);
    else rc = launch_scatter<W, 1>(ctx, src.keys, dd1, ps.sc + SC_NCH1, nch1, ctx->mat1.as<u32>(), ctx->bufA.as<Key>(), pl.d1, pl.P1);
    if (rc) return rc;
    ctx->mark("scatter1");
    return DSKGPU_OK;
}

// Stage 4, level 2 and the final offsets.  The fixed-capacity regions (k_scatter_al<.., OPT>): no histogram pass, every
// sub-partition gets a region of opt_cap keys (+ chains of extension regions); a pool that runs out (heavy repeats) sends the
// attempt back through the exact histogram + scan path, and the context remembers it for these reads.
template <int W>
int pass_scatter2(dskgpu_ctx* ctx, PassState<W>& ps) {
    const Plan& pl = ps.pl;
    int rc;
    ps.fkeys = ctx->bufA.as<typename KeyT<W>::T>();
    ps.scratch = &ctx->bufB;
    CK(ctx->fstart.ensure(((size_t)pl.F + 2) * 4));
    CK(ctx->nsolid.ensure(((size_t)pl.F + 2) * 4));
    if (pl.levels == 2 && ps.opt_cap) {
        CK(ctx->bufB.ensure((ps.nregions * ps.opt_cap + ATile<W>::KEYS + 16) * sizeof(typename KeyT<W>::T)));
        CK(ctx->descs2.ensure(((size_t)pl.P1 * 2 + 1) * sizeof(ChunkDesc)));
        CK(ctx->seg.ensure((size_t)pl.P1 * sizeof(SegInfo)));
        CK(ctx->mat2.ensure(((size_t)ps.nregions + 1) * 4));                  // here: keys per region (home regions, then the extension pool)
        CK(ctx->chain_next.ensure(((size_t)ps.nregions + 1 + ps.max_ext + 1) * 4));   // links (only read where subcnt has its chain bit set), then the list of chained sub-partitions
        // (zeroed by k_setup_pass)
        if (ps.opt1) {      // segments = the level-1 bin regions (slices + sentinel tails)
            ctx->h_descs2.resize(pl.P1);
            // heaviest segments first (the kernel hands them out by a work counter): a segment that holds a repeat family takes a
            // block longer than the others, so it must not be the last thing a block starts
            std::vector<u32> order(pl.P1);
            for (u32 sgm = 0; sgm < pl.P1; ++sgm) order[sgm] = sgm;
            // (in steps of 5 % of the mean, stable: the segments of uniform reads keep their natural order, neighbours in memory run together)
            double mean_work = 0.0; for (double w : ps.load) mean_work += w; mean_work = std::max(1.0, mean_work / pl.P1);
            auto wclass = [&](u32 a) { return (long long)(ps.load[a] / (0.05 * mean_work)); };
            std::stable_sort(order.begin(), order.end(), [&](u32 a, u32 b) { return wclass(a) > wclass(b); });
            for (u32 i = 0; i < pl.P1; ++i) {
                const u32 sgm = order[i];
                ChunkDesc d; d.begin = ctx->h_boff[sgm]; d.end = ctx->h_boff[sgm + 1]; d.flat_base = sgm * pl.P2; d.stride = 1;   // slice i of the segment: + i * area
                ctx->h_descs2[i] = d;
            }
            CK(hipMemcpyAsync(ctx->descs2.p, ctx->h_descs2.data(), (size_t)pl.P1 * sizeof(ChunkDesc), hipMemcpyHostToDevice, ctx->stream));
        } else {
            hipLaunchKernelGGL(k_plan, dim3(1), dim3(1024), 0, ctx->stream, ctx->mat1.as<u32>(), ps.nch1, pl.P1, 0x7FFFFFFFu, pl.P2,
                               ctx->seg.as<SegInfo>(), ctx->descs2.as<ChunkDesc>(), ps.sc + SC_NCH2, ps.sc + SC_MLEN2, 1u);
            CKL("k_plan");
        }
        ctx->mark("plan2");
        OptSpec os{ps.opt_cap, ctx->mat2.as<u32>(), ps.sc + SC_OVF2, ps.opt1 ? ps.o1.fill : nullptr, 0u, ps.grid1, (u64)ps.o1.area,
                   pl.F, ps.max_ext, ctx->chain_next.as<u32>(), ps.sc + SC_EXT, ctx->chain_next.as<u32>() + ps.nregions + 1, ps.sc + SC_NCHAINED,
                   ps.sc + SC_WORK2, nullptr};
        if (ctx->tune.verbose && ps.opt1) { CK(ctx->dbg.ensure((size_t)pl.P1 * 24)); os.dbg = ctx->dbg.as<unsigned long long>(); }
        if (ps.opt1) rc = launch_scatter_al<W, 2, true, true>(ctx, ctx->bufA.as<typename KeyT<W>::T>(), ctx->descs2.as<ChunkDesc>(), ps.sc + SC_NCH2, (u64)pl.P1 * 2, nullptr,
                                                              ctx->bufB.as<typename KeyT<W>::T>(), pl.d2, pl.P2, os);
        else rc = launch_scatter_al<W, 2, true, false>(ctx, ctx->bufA.as<typename KeyT<W>::T>(), ctx->descs2.as<ChunkDesc>(), ps.sc + SC_NCH2, (u64)pl.P1 * 2, nullptr,
                                                       ctx->bufB.as<typename KeyT<W>::T>(), pl.d2, pl.P2, os);
        if (rc) return rc;
        ctx->mark("scatter2");
        if (ctx->tune.verbose && ps.opt1) {      // per-segment times of the level-2 scatter, in hand-out order
            std::vector<unsigned long long> t((size_t)pl.P1 * 3);
            CK(hipMemcpyAsync(t.data(), ctx->dbg.p, t.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
            CK(hipStreamSynchronize(ctx->stream));
            unsigned long long t0 = ~0ull, t1 = 0; for (u32 i = 0; i < pl.P1; ++i) { t0 = std::min(t0, t[3 * i]); t1 = std::max(t1, t[3 * i + 1]); }
            fprintf(stderr, "[dskgpu] level 2: %u segments, %.3f ms first start -> last end\n", pl.P1, (t1 - t0) * 1e-5);
            for (u32 i = 0; i < pl.P1; ++i)
                if (i < 6 || i + 3 >= pl.P1 || t[3 * i + 1] + 20000 > t1)
                    fprintf(stderr, "[dskgpu]   desc %u (segment %u, load %.0f) block %llu: %.3f .. %.3f ms\n", i, (u32)(ctx->h_descs2[i].flat_base / pl.P2),
                            ps.load[ctx->h_descs2[i].flat_base / pl.P2], t[3 * i + 2], (t[3 * i] - t0) * 1e-5, (t[3 * i + 1] - t0) * 1e-5);
        }
        ps.fkeys = ctx->bufB.as<typename KeyT<W>::T>();
        ps.scratch = &ctx->bufA;
    } else if (pl.levels == 2) {
        const u64 max_chunks2 = ps.cap / CH2 + pl.P1 + 1;
        const u64 M2 = max_chunks2 * pl.P2;
        if (M2 >= 0xFFFFFFFFull) return fail(ctx, DSKGPU_E_ARG, "level-2 matrix too large");
        CK(ctx->descs2.ensure(max_chunks2 * sizeof(ChunkDesc)));
        CK(ctx->seg.ensure((size_t)pl.P1 * sizeof(SegInfo)));
        CK(ctx->mat2.ensure((M2 + 1) * 4));
        hipLaunchKernelGGL(k_plan, dim3(1), dim3(1024), 0, ctx->stream, ctx->mat1.as<u32>(), ps.nch1, pl.P1, CH2, pl.P2,
                           ctx->seg.as<SegInfo>(), ctx->descs2.as<ChunkDesc>(), ps.sc + SC_NCH2, ps.sc + SC_MLEN2, 0u);
        CKL("k_plan");
        ctx->mark("plan2");
        const ChunkDesc* dd2 = ctx->descs2.as<ChunkDesc>();
        if ((rc = launch_hist<W, 1>(ctx, ctx->bufA.as<typename KeyT<W>::T>(), dd2, ps.sc + SC_NCH2, max_chunks2, ctx->mat2.as<u32>(), pl.d2, pl.P2))) return rc;
        ctx->mark("hist2");
        if ((rc = run_scan(ctx, ctx->mat2.as<u32>(), ps.sc + SC_MLEN2, M2))) return rc;
        ctx->mark("scan2");
        if ((rc = launch_scatter<W, 1>(ctx, ctx->bufA.as<typename KeyT<W>::T>(), dd2, ps.sc + SC_NCH2, max_chunks2, ctx->mat2.as<u32>(), ctx->bufB.as<typename KeyT<W>::T>(), pl.d2, pl.P2))) return rc;
        ctx->mark("scatter2");
        ps.fkeys = ctx->bufB.as<typename KeyT<W>::T>();
        ps.scratch = &ctx->bufA;
        hipLaunchKernelGGL(k_final_offsets, dim3((pl.F + 256) / 256), dim3(256), 0, ctx->stream, ctx->mat2.as<u32>(),
                           ctx->seg.as<SegInfo>(), pl.P2, 0u, ps.sc + SC_MLEN2, ctx->fstart.as<u32>(), pl.F);
    } else {
        hipLaunchKernelGGL(k_final_offsets, dim3((pl.F + 256) / 256), dim3(256), 0, ctx->stream, ctx->mat1.as<u32>(),
                           (const SegInfo*)nullptr, pl.P1, ps.nch1, ps.sc + SC_MLEN1, ctx->fstart.as<u32>(), pl.F);
    }
    CKL("k_final_offsets");
    ctx->mark("offsets");
    return DSKGPU_OK;
}

// the count kernels (the sub-partitions, those that went on in extension regions, the k-mers counted apart), the scan of the
// solid rows per sub-partition, the sizes back to the host (one sync)
template <int W>
int count_and_sizes(dskgpu_ctx* ctx, PassState<W>& ps, const CountParams& cp) {
    typedef typename KeyT<W>::T Key;
    const Plan& pl = ps.pl;
    const unsigned cgrid = (unsigned)std::min<u64>(pl.F, (u64)ctx->num_cu * 2);
    launch_count<W>(ctx, cgrid, ps.fkeys, ps.solid_keys, ps.solid_ab, ps.sc + SC_OVERFLOW, cp);
    CKL("k_count");
    if constexpr (W <= 2) {
        if (ps.opt_cap && ps.max_ext) {      // the sub-partitions that went on in extension regions (none on repeat-free reads: the blocks leave at once)
            auto kern = [] { if constexpr (W == 1) return k_count_chained; else return k_count_chained_mw<2>; }();
            hipLaunchKernelGGL(kern, dim3((unsigned)std::min<u64>(ps.max_ext, (u64)ctx->num_cu * 2)), dim3(CNT_NT), 0, ctx->stream, ps.fkeys, ps.solid_keys, ps.solid_ab,
                               ctx->nsolid.as<u32>(), ctx->ghist.as<u64>(), ctx->gstats.as<u64>(), ps.sc + SC_OVERFLOW, cp, (const u32*)cp.subcnt,
                               (const u32*)ctx->chain_next.as<u32>(), (const u32*)(ctx->chain_next.as<u32>() + ps.nregions + 1), (const u32*)(ps.sc + SC_NCHAINED), ps.max_ext);
            CKL(W == 1 ? "k_count_chained" : "k_count_chained_mw");
        }
        if (ps.nheavy) {      // the k-mers the level-1 scatter counted apart: histogram, distinct count, rows (appended behind the compacted ones: pass_rows)
            const u32 slots = HV_KEYS;
            u64* hvb = ctx->hv_buf.as<u64>();
            hipLaunchKernelGGL(k_heavy_rows<W>, dim3((slots + 255) / 256), dim3(256), 0, ctx->stream, reinterpret_cast<const Key*>(hvb + HvLayout<W>::keys),
                               (const unsigned long long*)(hvb + HvLayout<W>::counts), slots, cp.amin, cp.amax, cp.histo_max, ctx->ghist.as<u64>(), ctx->gstats.as<u64>(),
                               hvb + HvLayout<W>::rows, reinterpret_cast<u32*>(hvb + HvLayout<W>::ab));
            CKL("k_heavy_rows");
        }
    }
    ctx->mark("count");
    if (int e = run_scan(ctx, ctx->nsolid.as<u32>(), ps.sc + SC_F, pl.F)) return e;
    ctx->mark("scan_solid");
    // (k-mers of the pass: the last sub-partition offset, or -- fixed-capacity regions -- the level-1 total; with block-owned slices
    //  the scatter's own count in gstats[2])
    CK(ctx->back_dev.ensure(16 * 8));
    if (!ctx->back_host) CK(hipHostMalloc(reinterpret_cast<void**>(&ctx->back_host), 16 * 8, hipHostMallocDefault));
    const u32* nkp = ps.opt1 ? nullptr : (ps.opt_cap ? ctx->mat1.as<u32>() + (u64)pl.P1 * ps.nch1 : ctx->fstart.as<u32>() + pl.F);
    hipLaunchKernelGGL(k_gather_back, dim3(1), dim3(64), 0, ctx->stream, (const u32*)ps.sc, (const u32*)(ctx->nsolid.as<u32>() + pl.F), nkp,
                       (const u64*)ctx->gstats.as<u64>(), ctx->back_dev.as<u64>());
    CKL("k_gather_back");
    CK(hipMemcpyAsync(ctx->back_host, ctx->back_dev.p, 10 * 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    const u64* bh = ctx->back_host;
    ps.flags = (u32)bh[0]; ps.nsolid = (u32)bh[1]; if (!ps.opt1) ps.nkeys = (u32)bh[2];
    ps.ovf2 = (u32)bh[3]; ps.ovf1 = (u32)bh[4]; ps.ext = (u32)bh[5];
    for (int x = 0; x < 4; ++x) ps.stats[x] = bh[6 + x];
    return DSKGPU_OK;
}

// Stage 5, count: one-word keys write solid rows in place (+ abundance into the free ping-pong buffer); two-word keys write rows
// into the free buffer (+ abund2), and may count twice (below)
template <int W>
int pass_count(dskgpu_ctx* ctx, PassState<W>& ps) {
    CountParams cp;
    cp.F = ps.pl.F;
    cp.maxload = W == 1 ? CNT_MAXLOAD : C2_MAXLOAD;
    if (ctx->tune.table_maxload) cp.maxload = std::min<u32>(cp.maxload, ctx->tune.table_maxload);
    cp.amin = ctx->cfg.abundance_min; cp.amax = ctx->cfg.abundance_max; cp.histo_max = ctx->cfg.histo_max;
    cp.cap = ps.opt_cap; cp.subcnt = ps.opt_cap ? ctx->mat2.as<u32>() : nullptr;
    ps.solid_keys = W == 1 ? ps.fkeys : ps.scratch->template as<typename KeyT<W>::T>();
    ps.solid_ab = W == 1 ? ps.scratch->template as<u32>() : ctx->abund2.as<u32>();
    if constexpr (W == 2) CK(hipMemcpyAsync(ctx->gstats.as<u64>() + 3, ctx->gstats.as<u64>() + 2, 8, hipMemcpyDeviceToDevice, ctx->stream));      // (the keys level 1 placed, before k_heavy_rows adds to them: see below)
    if (int e = count_and_sizes<W>(ctx, ps, cp)) return e;
    if constexpr (W == 2) {
        // k_count2v3 keys its table by the mixed top word alone and checks every key's low word afterwards.  Two different k-mers of the pass with
        // the same top word (birthday bound of a 64-bit hash: n^2 / 2^65 -- 0.5 % of the runs at 4 * 10^8 distinct k-mers), or one whose top word
        // is the empty-slot value: the count runs again with the index-table kernel (the keys are untouched: two-word rows go to the other
        // buffer), and the rest of the reads' passes use that kernel too.  Tests craft both cases.
        if ((ps.flags & (CNT_OVF_VERIFY | CNT_OVF_SENTINEL)) && !((ps.opt_cap && ps.ovf2) || (ps.opt1 && ps.ovf1))) {
            if (ctx->tune.verbose) fprintf(stderr, "[dskgpu] pass %u/%u: the top-word table met k-mers it cannot tell apart (flags %u): counting again with k_count_mw\n", ps.pass, ps.npass, ps.flags);
            ctx->mw_v3_off = true;
            ctx->stats.n_retries += 1;
            CK(hipMemsetAsync(ctx->ghist.p, 0, ((size_t)ctx->cfg.histo_max + 1) * 8, ctx->stream));
            CK(hipMemsetAsync(ctx->gstats.p, 0, 2 * 8, ctx->stream));
            CK(hipMemcpyAsync(ctx->gstats.as<u64>() + 2, ctx->gstats.as<u64>() + 3, 8, hipMemcpyDeviceToDevice, ctx->stream));
            CK(hipMemsetAsync(ps.sc + SC_OVERFLOW, 0, 4, ctx->stream));
            if (int e = count_and_sizes<W>(ctx, ps, cp)) return e;
        }
    }
    if (ps.opt1) ps.nkeys = (u32)ps.stats[2];
    return DSKGPU_OK;
}

// the solid rows of a pass where the count kernels left them (regions / exact ranges), with the rows of the k-mers counted apart as
// a dense tail (ro / rows_ab from row n_sparse on: already un-mixed)
template <int W>
SparseRows sparse_rows(dskgpu_ctx* ctx, const PassState<W>& ps, const RowsOut& ro, const u32* rows_ab, u32 n_tail) {
    SparseRows r;
    r.W = W; r.keys = ps.solid_keys; r.ab = (const u32*)ps.solid_ab; r.soff = ctx->nsolid.as<u32>(); r.fstart = ctx->fstart.as<u32>(); r.cap = ps.opt_cap; r.F = ps.pl.F;
    r.n_sparse = ps.nsolid; r.n_tail = W <= 2 ? n_tail : 0u;      // (four-word keys: no k-mers counted apart, no tail)
    if (r.n_tail) { for (int x = 0; x < W; ++x) r.tail_w.w[x] = ro.w[x] + r.n_sparse; r.tail_ab = rows_ab + r.n_sparse; }
    return r;
}

// Stage 6, the pass's rows: the heavy tail, then the hand-off to the row sort (sparse), the multi-pass partition order, or k_compact
template <int W>
int pass_rows(dskgpu_ctx* ctx, PassState<W>& ps) {
    typedef typename KeyT<W>::T Key;
    const Plan& pl = ps.pl;
    const u32 h_nsolid = ps.nsolid;
    const u64 nhs = ps.nheavy ? ps.stats[1] : 0;                    // solid rows of the k-mers counted apart
    const u64 ns = ps.rows = h_nsolid + nhs;
    // (a pass of a multi-pass job whose accumulators have room: the rows go there directly -- no copy of 0.7 GB per pass afterwards)
    const bool to_sink = ctx->sink.active && ctx->sink.rows + ns + 1 <= ctx->sink.cap;
    RowsOut ro{};
    u32* rows_ab = nullptr;
    if (to_sink) {
        rows_ab = ctx->sink.ab + ctx->sink.rows;
        for (int x = 0; x < W; ++x) ro.w[x] = ctx->sink.w[x] + ctx->sink.rows;
        ctx->sink.took = true;
    } else {
        CK(ctx->out_ab.ensure((ns + 1) * 4));
        rows_ab = ctx->out_ab.as<u32>();
        for (int x = 0; x < W; ++x) { CK(ctx->out_w[x].ensure((ns + 1) * 8)); ro.w[x] = ctx->out_w[x].as<u64>(); }
    }
    if constexpr (W <= 2) {
      if (nhs) {
        for (int x = 0; x < W; ++x)
            CK(hipMemcpyAsync(ro.w[x] + h_nsolid, ctx->hv_buf.as<u64>() + HvLayout<W>::rows + (size_t)x * HV_KEYS, nhs * 8, hipMemcpyDeviceToDevice, ctx->stream));
        CK(hipMemcpyAsync(rows_ab + h_nsolid, ctx->hv_buf.as<u64>() + HvLayout<W>::ab, nhs * 4, hipMemcpyDeviceToDevice, ctx->stream));
      }
    }
    ctx->stats.n_heavy += ps.nheavy;
    // Rows of a single pass that the hand-written MSD sort will order: its first step reads them where they lie (the regions /
    // exact ranges of the count kernel + the few rows of the k-mers counted apart as a dense tail) -- no dense copy is made first
    // (k_compact: 0.5 GB read + 0.5 GB written, 0.30 ms of a 14 ms step).  Several passes accumulate dense rows as before.
    // (two-word rows: the same, through rowsort2.h's sparse step A -- sort_rows2_msd is what sort_rows picks under these conditions)
    bool sparse_sort = false;
    if constexpr (W <= 2) {
        sparse_sort = ps.npass == 1 && ctx->job_passes == 1 && ns > 0 && ns <= rs_max_rows(ctx) && !(ctx->cfg.flags & DSKGPU_F_NO_SORT) &&
                      !ctx->tune.rs_slab_rows && !ctx->banks.job.active && (W == 1 || 2u * ctx->cfg.kmer_size > 64u);
    } else {
        // four-word rows: sparse only for DSKGPU_F_PARTITION_ORDER (k_part_sort4 reads them there and writes them dense into ro / rows_ab, which is
        // where the global sort of four-word rows, sort_rows4, wants them should a block give up); without the flag k_compact as before
        sparse_sort = (ctx->cfg.flags & DSKGPU_F_PARTITION_ORDER) && ps.npass == 1 && ctx->job_passes == 1 && ns > 0 && ns < 0xFFFF0000ull &&
                      !(ctx->cfg.flags & DSKGPU_F_NO_SORT) && !ctx->tune.rs_slab_rows && !ctx->banks.job.active;
    }
    if (sparse_sort) ctx->sp_rows = sparse_rows<W>(ctx, ps, ro, rows_ab, (u32)nhs);
    PartPasses& mp = ctx->rs.mp;
    bool mp_part = false;
    {      // DSKGPU_F_PARTITION_ORDER in a multi-pass count: the pass's rows ordered partition by partition on their way into the dense arrays
        mp_part = !sparse_sort && ctx->job_passes > 1 && mp.ok && ns > 0 && h_nsolid < 0xFFFF0000ull && (W == 1 || 2u * ctx->cfg.kmer_size > 64u);
        if (!sparse_sort && ctx->job_passes > 1 && ns > 0 && !mp_part) mp.ok = false;      // (one pass outside the scheme: the job keeps the global order)
        if (mp_part) {
            const SparseRows rows = sparse_rows<W>(ctx, ps, ro, rows_ab, (u32)nhs);
            if (mp.part_off.ensure_keep(((size_t)mp.off_used + part_sort_nparts(rows) + 2) * 4, (size_t)mp.off_used * 4, ctx->stream)) return fail(ctx, DSKGPU_E_NOMEM, "partition offsets");
            u32 np = 0;
            if (const int prc = launch_part_sort(ctx, rows, ro, rows_ab, mp.part_off.as<u32>() + mp.off_used, mp.flag.as<u32>(), &np)) return prc;
            mp.passes.push_back(PartPasses::Pass{mp.row_base, np, mp.off_used});
            mp.off_used += np + 1;
        }
    }
    if (!sparse_sort && !mp_part) {
        hipLaunchKernelGGL(k_compact<W>, dim3((pl.F + 3) / 4), dim3(256), 0, ctx->stream, (const Key*)ps.solid_keys, (const u32*)ps.solid_ab,
                           ctx->fstart.as<u32>(), ctx->nsolid.as<u32>(), pl.F, ro, rows_ab, ps.opt_cap);
        CKL("k_compact");
    }
    ctx->mark("compact");
    ctx->stats.n_ext_regions += std::min<u32>(ps.ext, ps.max_ext);
    return DSKGPU_OK;
}

// What a pass leaves for run_pipeline.  too_big: the pass holds more keys (keys_seen) than `cap`; nothing else is set then.
struct PassResult { u64 rows = 0, kmers = 0, distinct = 0, keys_seen = 0; Plan plan{}; bool too_big = false; };

// One pass: partition + count the keys of pass `pass` (of `npass`) and leave its solid rows (unsorted) in out_w[0]/out_w[1]/out_ab,
// the job's accumulators (ctx->sink) or where the count kernels put them (ctx->sp_rows).
// An overflow of a level-1 slice or the level-2 pool repeats the attempt on the exact path; a table overflow repeats it with a
// finer partition, at most three times.
template <int W>
int run_one_pass(dskgpu_ctx* ctx, bool from_reads, const typename KeyT<W>::T* d_keys_in, u64 nkeys_in, u64 nwords,
                 u32 pass, u32 npass, u64 cap, PassResult* res) {
    ctx->take_sparse_rows();
    KeySource<W> src{from_reads, !from_reads && d_keys_in == nullptr, d_keys_in, nkeys_in, nwords};
    const u64 nvalid = from_reads ? ctx->h_nvalid : nkeys_in;
    int extra_bits = 0, table_retries = 0;
    for (;;) {
        PassState<W> ps{src, pass, npass, cap, nvalid, ctx->scalars.as<u32>()};
        int e;
        if ((e = pass_plan<W>(ctx, ps, extra_bits)) || (e = pass_layout1<W>(ctx, ps)) || (e = pass_scatter1<W>(ctx, ps))) return e;
        if (ps.too_big) { ctx->resolve_marks(); res->too_big = true; res->keys_seen = ps.nkeys; return DSKGPU_OK; }
        if ((e = pass_scatter2<W>(ctx, ps)) || (e = pass_count<W>(ctx, ps))) return e;
        const bool ovf1 = ps.opt1 && ps.ovf1, ovf2 = ps.opt_cap && ps.ovf2;
        if (ovf1 || ovf2) {      // a slice / region overflowed: the attempt again with exact offsets (no table retry)
            ctx->resolve_marks();
            if (ctx->tune.verbose) fprintf(stderr, "[dskgpu] pass %u/%u: %s overflowed: the exact path takes over\n", pass, npass, ovf1 ? "a level-1 slice" : "the level-2 extension pool");
            if (ovf1) ctx->opt1_off = true;
            else { ctx->opt2_off = true; ctx->opt1_off = true; }     // the exact level 2 cannot read sentinel-padded slices
            ctx->stats.n_retries += 1;
            ctx->mark("start");
            continue;
        }
        if (ps.flags & 1u) {     // a count table overflowed: a finer partition
            ctx->resolve_marks();
            if (table_retries >= 3) return fail(ctx, DSKGPU_E_OVERFLOW, "hash table overflow after 3 retries");
            ++table_retries; extra_bits += 1;
            ctx->stats.n_retries += 1;
            ctx->mark("start");
            continue;
        }
        if ((e = pass_rows<W>(ctx, ps))) return e;
        res->rows = ps.rows; res->kmers = res->keys_seen = ps.nkeys; res->distinct = ps.stats[0]; res->plan = ps.pl;
        return DSKGPU_OK;
    }
}

// "Level 0" of a multi-pass count from reads (one-word keys): ONE sweep over the encoded reads writes the mixed keys of passes
// [lo, lo + G) of npass into ctx->l0buf, grouped by pass -- the histogram-free scatter with the pass as its digit (MODE 4): every
// (block, pass) pair owns a slice inside the pass's region, the unused tails are padded with the sentinel, so a region is one key
// array.  The passes of the group then run from those arrays (run_one_pass with a key source) instead of re-generating every k-mer
// once per pass -- the in-HBM counterpart of DSK writing every k-mer to its partition file ONCE (doc/paper.tex:65-67;
// README.md:126-130 asks for few passes because each one re-reads the input: a sweep here is what a pass is there).
// G = as many passes as the free HBM holds next to what a pass itself needs and `reserve_bytes` (rows still to come), at most
// L0_MAX_PASSES.  The slices of pass i are sized from ITS sampled load and its measured spread (a positional sample of <= 1024
// tiles, as at level 1): the pass that holds a k-mer with 10^8 occurrences (poly-A reads of a 30x human run) gets longer slices
// instead of sending its whole group back to the reads.
// -> region_keys[i]: keys (pads included) of pass lo + i's array; obase[i]: its offset in l0buf.  DSKGPU_OK with *G_out = 0: no room.
int level0_materialise(dskgpu_ctx* ctx, u64 nwords, u32 lo, u32 npass, u64 reserve_bytes, u32* G_out, u64 (&region_keys)[L0_MAX_PASSES], u64 (&obase)[L0_MAX_PASSES]) {
    *G_out = 0;
    const u64 nper = ctx->h_nvalid / npass + 1;
    u32 nch1 = 0;
    build_descs1(ctx, nwords, Tile<1>::WORDS, (u64)ctx->num_cu * 8, &nch1);
    // (k_level0 keeps nothing but its cursors in LDS: two blocks per CU, 32 waves, hide each other's atomics and stores)
    const unsigned grid = (unsigned)std::max<u64>(1, std::min<u64>(nch1, (u64)ctx->num_cu));
    const u64 cpb = (nch1 + grid - 1) / grid;
    const double share = (double)cpb / (double)nch1;                                // the busiest block's share of the chunks
    const u64 tail = 2 * Tile<1>::KEYS;
    const u64 uslice = (((u64)((double)nper * share * 1.02) + 4096) + 7) & ~7ull;   // hash-uniform passes: 2 % + 4096 over the busiest block's share
    const u64 uregion = uslice * grid + tail;                                       // keys; + the dump zone
    if (uregion >= 0xFFFF0000ull) return DSKGPU_OK;
    // how many passes fit beside what a pass itself needs (slices, regions + pool, rows): about 30 bytes per key of a pass
    size_t free_b = 0, total_b = 0;
    CK(hipMemGetInfo(&free_b, &total_b));
    const u64 have = ctx->bufA.cap + ctx->bufB.cap + ctx->l0buf.cap;
    const u64 need = nper * 30ull + (4ull << 30) + reserve_bytes;
    const u64 room = free_b + have > need ? free_b + have - need : 0;
    u32 G = (u32)std::min<u64>(std::min<u64>(L0_MAX_PASSES, npass - lo), room / (uregion * 8));
    if (ctx->tune.l0_passes) G = std::min<u32>(std::min<u32>(ctx->tune.l0_passes, L0_MAX_PASSES), npass - lo);      // tests
    if (G < 2 && !(ctx->tune.l0_passes)) return DSKGPU_OK;                          // one pass at a time gains nothing over reading the reads
    if (G == 0) return DSKGPU_OK;
    CK(ctx->descs1.ensure(ctx->h_descs1.size() * sizeof(ChunkDesc)));
    CK(hipMemcpyAsync(ctx->descs1.p, ctx->h_descs1.data(), ctx->h_descs1.size() * sizeof(ChunkDesc), hipMemcpyHostToDevice, ctx->stream));
    u32* sc = ctx->scalars.as<u32>();
    DigitSpec ds{4u, G, 0u, ctx->cfg.world_size, npass, lo};
    // ---- the passes' loads in this sweep, sampled
    std::vector<u64> slice(G, uslice);
    if (!ctx->tune.no_sample) {
        auto hist = [&](const ChunkDesc* dd, const u32* d_nch, u64 n, u32* mat) { return launch_hist_m<1, 0, 4>(ctx, nullptr, dd, d_nch, n, mat, ds, G); };
        u64 ntiles = 0, nts = 0, stot = 0;
        { const int e = positional_sample(ctx, nwords, Tile<1>::WORDS, G, hist, &ntiles, &nts, &stot); if (e) return e; }
        if (stot >= (u64)G * 4096) {
            const double scale = (double)ntiles / (double)nts, tiles_per_block = (double)ntiles * share;
            for (u32 b = 0; b < G; ++b) {
                const double sum = (double)ctx->h_mom[2 * b], sq = (double)ctx->h_mom[2 * b + 1];
                const double mean = sum / (double)nts, var = std::max(mean, sq / (double)nts - mean * mean);
                const double sl = sum * scale * share * 1.01 + 5.0 * std::sqrt(tiles_per_block * var) + 4.0 * std::sqrt((double)nts * var) * scale * share + 64.0;
                slice[b] = ((u64)sl + 8) & ~7ull;
            }
        }
        ctx->mark("sample0");
    }
    // regions, largest G whose regions fit the room
    for (;;) {
        u64 tot = 0; bool ok = true;
        for (u32 b = 0; b < G; ++b) { const u64 region = slice[b] * grid + tail; if (region >= 0xFFFF0000ull) ok = false; obase[b] = tot; region_keys[b] = slice[b] * grid; tot += region; }
        if (ok && (tot * 8 <= room || ctx->tune.l0_passes)) { CK(ctx->l0buf.ensure(tot * 8 + 64)); break; }
        if (--G < 2) return DSKGPU_OK;
    }
    ds.pa = G;
    ctx->h_sc[SC_NCH1] = nch1; ctx->h_sc[SC_OVF1] = 0;
    CK(hipMemcpyAsync(sc + SC_NCH1, &ctx->h_sc[SC_NCH1], 4, hipMemcpyHostToDevice, ctx->stream));
    CK(hipMemsetAsync(sc + SC_OVF1, 0, 4, ctx->stream));
    // device arrays of the sweep: [slice length per bin: u32 x (L0_MAX_PASSES + 1)] [region base per bin: u64 x L0_MAX_PASSES]
    ctx->h_boff.assign(L0_MAX_PASSES + 1 + 3 + 2 * L0_MAX_PASSES, 0);
    u64 hob[L0_MAX_PASSES];
    for (u32 i = 0; i < L0_MAX_PASSES; ++i) { ctx->h_boff[i] = (u32)slice[std::min(i, G - 1)]; hob[i] = obase[std::min(i, G - 1)]; }
    std::memcpy(&ctx->h_boff[L0_MAX_PASSES + 4], hob, sizeof hob);          // (at byte 80: 8-byte aligned)
    CK(ctx->boff.ensure(ctx->h_boff.size() * 4));
    CK(hipMemcpyAsync(ctx->boff.p, ctx->h_boff.data(), ctx->h_boff.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    const u32* d_slen = ctx->boff.as<u32>();
    const u64* d_obase = reinterpret_cast<const u64*>(ctx->boff.as<u32>() + L0_MAX_PASSES + 4);
    hipLaunchKernelGGL(k_level0, dim3(grid), dim3(SC_NT), 0, ctx->stream, (const u64*)ctx->packed.as<u64>(), (const u32*)ctx->inval.as<u32>(), (const ChunkDesc*)ctx->descs1.as<ChunkDesc>(),
                       (const u32*)(sc + SC_NCH1), ctx->l0buf.as<u64>(), (int)ctx->cfg.kmer_size, ds, G, d_slen, d_obase, sc + SC_OVF1);
    CKL("k_level0");
    ctx->mark("level0");
    CK(hipMemcpyAsync(&ctx->h_ovf1, sc + SC_OVF1, 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    if (ctx->tune.verbose) {
        u64 tot = 0; for (u32 b = 0; b < G; ++b) tot += region_keys[b];
        fprintf(stderr, "[dskgpu] level 0: passes %u..%u of %u materialised, %.2f GB in all (%.2f GB free before)%s\n", lo, lo + G - 1, npass, (double)tot * 8e-9, (double)free_b * 1e-9,
                ctx->h_ovf1 ? " -- a slice overflowed: these passes read the reads" : "");
    }
    if (ctx->h_ovf1) return DSKGPU_OK;                                             // (a skewed key space beyond the sampled spread: the passes of this group re-generate their keys)
    *G_out = G;
    return DSKGPU_OK;
}

// The pipeline behind dskgpu_count / dskgpu_mg_count: encode once, then one or several passes over
// the key space (several when the input holds more k-mers than a pass may: < 2^32 offsets, and the
// ping-pong buffers must fit HBM -- the in-memory counterpart of DSK's disk passes), then the row sort.
template <int W>
int run_pipeline(dskgpu_ctx* ctx, bool from_reads, const typename KeyT<W>::T* d_keys_in, u64 nkeys_in) {
    typedef typename KeyT<W>::T Key;
    ctx->drop_result();
    ctx->sink = dskgpu_ctx::RowSink{};
    if (from_reads) { ctx->st_names.clear(); ctx->st_ms.clear(); }   // from keys: keep the mg_scatter stages of this step
    ctx->marks.clear(); ctx->ev_used = 0;
    const u64 n_upper = from_reads ? ctx->n_bytes : nkeys_in;
    u64 nwords = 0;
    ctx->mark("start");
    if (from_reads) {
        int rc = encode_current(ctx, &nwords);
        if (rc) return rc;
        ctx->mark("encode");
    }
    CK(ctx->scalars.ensure(SC_COUNT * 4));
    CK(ctx->ghist.ensure(((size_t)ctx->cfg.histo_max + 1 + 2) * 8));      // (+ 2: k_sort_back's words)
    CK(ctx->gstats.ensure(4 * 8));
    ctx->have_nvalid = false;
    if (from_reads && nwords) {
        // the exact number of valid k-mer windows (0.08 ms): the plan is sized from it (the byte count over-states the k-mers of
        // 150 bp reads by a quarter: 590 K sub-partitions of 2030 keys instead of 469 K of 2560), and so are the level-1 slices
        CK(hipMemsetAsync(ctx->gstats.p, 0, 4 * 8, ctx->stream));
        hipLaunchKernelGGL(k_count_valid, dim3((unsigned)std::min<u64>((nwords + 255) / 256, (u64)ctx->num_cu * 8)), dim3(256), 0, ctx->stream,
                           ctx->inval.as<u32>(), nwords, (int)ctx->cfg.kmer_size, ctx->gstats.as<u64>() + 3);
        CKL("k_count_valid");
        {
            void* lz = landing(ctx, 8);
            CK(hipMemcpyAsync(lz ? lz : (void*)&ctx->h_nvalid, ctx->gstats.as<u64>() + 3, 8, hipMemcpyDeviceToHost, ctx->stream));
            CK(hipStreamSynchronize(ctx->stream));
            if (lz) std::memcpy(&ctx->h_nvalid, lz, 8);
        }
        ctx->have_nvalid = true;
    }
    const u64 max_keys = ctx->max_keys_per_pass ? ctx->max_keys_per_pass : 0xD0000000ull;      // (3.49 G: level 1 then needs <= 1536 bins, what its LDS holds with the slice ends)
    // Passes over the key space: as few as hold the keys -- any number, not a power of two (key_in_pass maps a bit field of the
    // mixed key onto [0, npass)) -- counted from the EXACT number of valid k-mer windows when the keys come from reads: the byte
    // count over-states the k-mers of 150 bp reads by a quarter, which together with the doubling below once made 16 passes of
    // what 7 hold (200 M x 150 bp on one GPU: every pass re-generates all k-mers).  A pass that turns out too big (a skewed
    // key space) doubles the count.
    const u64 n_keys = (from_reads && ctx->have_nvalid) ? std::max<u64>(1, ctx->h_nvalid) : n_upper;
    // An input that needs several passes anyway (one-word keys from reads) takes SMALL ones -- 10^9 keys, the size of the bench
    // workload: a level-0 sweep then materialises up to 16 of them (what the free HBM holds: a pass of 10^9 keys works in 22 GB,
    // one of 3.5 * 10^9 in 75 GB, which left room for one or two key arrays beside it on a 90 Gbp input), and level 1 of a pass
    // has 512 bins instead of 1536 (its cost per key grows with the bin count: 3.8 against 5.9 ps).
    u64 pass_keys = max_keys;
    if (W == 1 && from_reads && ctx->have_nvalid && n_keys > max_keys && !ctx->max_keys_per_pass && !ctx->tune.no_level0)
        pass_keys = ctx->tune.mp_pass_mkeys ? (u64)ctx->tune.mp_pass_mkeys * 1000000ull : 1000000000ull;
    // two-word keys: a pass holds what 32-bit key indices address (regions of 2180 keys at <= 60 % fill)
    const u64 hard_max = W == 2 && !ctx->max_keys_per_pass ? std::min<u64>(max_keys, 2400000000ull) : max_keys;
    u32 npass = (u32)std::max<u64>(1, (n_keys + pass_keys - 1) / pass_keys);
    // Several passes from reads, 20 <= k <= 64: the passes are virtual OWNERS and a sweep materialises super-k-mer records (sender.hip: rec_l0_*).
    bool rec_l0 = W <= 2 && from_reads && ctx->have_nvalid && ctx->sk_mode && ctx->cfg.world_size == 1 && !ctx->tune.no_level0 && !ctx->tune.l0_keys && !ctx->rec_l0_off &&
                  (npass > 1 || n_keys > hard_max);
    RecL0 rl;
    // The level 0 has a Sender of its own (owners = passes, a table for that many) and leaves the exchange's alone.  Only scratch is shared: the
    // passes overwrite ctx->packed / mat1, so a send layout or an encoding kept for the exchange is void from here on, however this function is left.
    // Clearing the two flags once, here, covers every exit below: only sk_prepare and dskgpu_mg_sample set them, and nothing in this function calls either.
    if (rec_l0) {
        ctx->sender.prepared = false; ctx->enc_fresh = false;
        u64 want = ctx->max_keys_per_pass ? max_keys : ctx->tune.mp_pass_mkeys ? (u64)ctx->tune.mp_pass_mkeys * 1000000ull : (W == 1 ? 1200000000ull : 1000000000ull);
        u64 G = (n_keys + want - 1) / want;
        if (G < 2) G = 2;
        if (G > SK_MAX_OWNERS) G = SK_MAX_OWNERS;
        // (owners are balanced to a few per cent by the repartition table: 15 % head-room under what a pass may hold)
        if (n_keys / G + n_keys / G / 7 > hard_max && !ctx->max_keys_per_pass) rec_l0 = false;
        else {
            const int rc = rec_l0_prepare(ctx, ctx->l0_sender, nwords, (u32)G, &rl);
            if (rc == REC_L0_NO) rec_l0 = false; else if (rc) return rc;
            else npass = (u32)G;
        }
    }
    u64 cap_floor = 0;       // keys the largest pass seen so far really holds (a k-mer with millions of occurrences sits in ONE pass whatever their number)
    for (;;) {
        if (npass > 4096) return fail(ctx, DSKGPU_E_OVERFLOW, "too many passes (one k-mer alone exceeds a pass)");
        // buffers of one pass: every position could yield a key when there is a single pass; with several, the hash spreads
        // the keys evenly: 6 % + 1 M head-room, checked after the level-1 histogram (exact path) or by the slices (sampled path)
        const u64 cap = npass == 1 ? n_upper : std::min<u64>(n_upper, std::max<u64>(cap_floor, n_keys / npass + n_keys / npass / 16 + (1u << 20)));
        if (cap >= 0xFFFF0000ull) { npass *= 2; cap_floor = 0; continue; }
        // (bufA / bufB are sized by the pass itself: the histogram-free path wants slices and regions, not `cap` keys)
        if (W > 1) CK(ctx->abund2.ensure((cap + 1) * 4));
        ctx->hist.assign((size_t)ctx->cfg.histo_max + 1, 0);
        std::vector<u64> pass_hist(ctx->hist.size());
        u64 tot_rows = 0, tot_kmers = 0, tot_distinct = 0;
        Plan pl{};
        bool too_big = false; u64 seen = 0;      // a pass that held more keys than its buffers: how many
        u32 l0_lo = 0, l0_n = 0; u64 l0_keys[L0_MAX_PASSES] = {0}; u64 l0_base[L0_MAX_PASSES] = {0};       // passes materialised by the last level-0 sweep
        bool l0_try = W == 1 && from_reads && npass > 1 && ctx->have_nvalid && !ctx->tune.no_level0 && !rec_l0;
        u32 r_hi = 0; u64 r_base[SK_MAX_OWNERS] = {0};     // record-based level 0: owners materialised by the last sweep, first word of each one's region
        bool restart = false;
        u64 sweeps = 0;          // times the encoded reads were walked to generate k-mers (DSK's notion of a pass: README.md:126-130)
        bool rows_sized = false; // the row accumulators are sized for all passes (known after the first one)
        ctx->job_passes = npass;
        PartPasses& mp = ctx->rs.mp;
        mp.passes.clear(); mp.off_used = 0;
        mp.ok = npass > 1 && (ctx->cfg.flags & DSKGPU_F_PARTITION_ORDER) && !(ctx->cfg.flags & DSKGPU_F_NO_SORT) && !ctx->banks.job.active;
        if (mp.ok) { CK(mp.flag.ensure(256)); CK(hipMemsetAsync(mp.flag.p, 0, 4, ctx->stream)); }
        for (u32 p = 0; p < npass; ++p) {
            PassResult r{};
            r.plan = pl;                   // (a pass without keys leaves the plan of the one before)
            int rc;
            mp.row_base = tot_rows;      // (where this pass's rows start in the job)
            ctx->sink = dskgpu_ctx::RowSink{};
            if (npass > 1 && rows_sized) {      // the pass compacts its rows straight behind the job's (when they fit: run_one_pass)
                ctx->sink.active = true; ctx->sink.rows = tot_rows; ctx->sink.ab = ctx->acc_ab.as<u32>();
                u64 cap_rows = ctx->acc_ab.cap / 4;
                for (int x = 0; x < W; ++x) { ctx->sink.w[x] = ctx->acc_w[x].as<u64>(); cap_rows = std::min<u64>(cap_rows, ctx->acc_w[x].cap / 8); }
                ctx->sink.cap = cap_rows;
            }
            if (npass > 1) { ctx->opt1_off = false; ctx->opt2_off = false; ctx->mw_v3_off = false; }      // an overflow is a property of ONE pass (the one that holds a k-mer with 10^8 occurrences): the others keep the fast path
            if (rec_l0) {
                if (p >= r_hi) {       // the next sweep: as many owners as HBM holds beside a pass's own buffers and the rows still to come
                    size_t free_b = 0, total_b = 0;
                    CK(hipMemGetInfo(&free_b, &total_b));
                    const u64 nper = n_keys / npass + 1;
                    const u64 have = ctx->bufA.cap + ctx->bufB.cap + ctx->l0buf.cap;
                    const u64 rows_have = ctx->acc_ab.cap + ctx->acc_w[0].cap + (W > 1 ? ctx->acc_w[1].cap : 0);
                    const u64 rows_want = rows_sized ? 0 : n_keys / 16 * (8ull * W + 4);
                    const u64 need = nper * (W == 1 ? 30ull : 50ull) + (4ull << 30) + (rows_want > rows_have ? rows_want - rows_have : 0);
                    const u64 room = free_b + have > need ? free_b + have - need : 0;
                    const u64 R8 = (u64)ctx->l0_sender.sp.R * 8;
                    u64 left = 0; for (u32 o = p; o < npass; ++o) left += rl.region[o] * R8;
                    const u64 nsw = std::max<u64>(1, (left + std::max<u64>(room, 1) - 1) / std::max<u64>(room, 1));      // sweeps still needed: equal shares
                    const u64 target = (left + nsw - 1) / nsw;
                    u64 acc = 0; u32 hi = p;
                    while (hi < npass && (hi == p || (acc + rl.region[hi] * R8 <= room && acc < target))) { acc += rl.region[hi] * R8; ++hi; }
                    if (ctx->tune.l0_passes) hi = std::min<u32>(npass, p + ctx->tune.l0_passes);      // tests
                    rc = rec_l0_sweep(ctx, ctx->l0_sender, rl, p, hi, r_base);
                    if (rc == REC_L0_NO) { restart = true; break; }
                    if (rc) return rc;
                    r_hi = hi; ++sweeps;
                }
                const u64 nk_in = ctx->l0_sender.h_sent[p];
                ctx->rec_src = ctx->l0buf.as<u64>() + r_base[p]; ctx->rec_n = rl.region[p]; ctx->rec_expanded = false; ctx->rec_sized = false;
                ctx->rec_hint = 0; ctx->rec_hint_est = false; ctx->rec_slice_end.clear(); ctx->rec_gate = nullptr;
                if (nk_in == 0) { rc = DSKGPU_OK; CK(hipMemsetAsync(ctx->ghist.p, 0, ((size_t)ctx->cfg.histo_max + 1) * 8, ctx->stream)); }
                else rc = run_one_pass<W>(ctx, false, nullptr, nk_in, 0, 0u, 1u, nk_in, &r);
                ctx->rec_src = nullptr;
            } else
            if (l0_try && p >= l0_lo + l0_n) {       // the next group of passes: one sweep over the reads writes their keys
                // (until the first pass has told how many rows a pass leaves, room is kept for one solid row per sixteen k-mers -- what
                //  20x coverage leaves; should the rows need more, the group's remaining key arrays give way: below)
                const u64 reserve = rows_sized ? 0 : n_keys / 16 * 12;
                if constexpr (W == 1) { if ((rc = level0_materialise(ctx, nwords, p, npass, reserve, &l0_n, l0_keys, l0_base))) return rc; }
                l0_lo = p;
                if (l0_n == 0) l0_try = false;       // no room (or a skewed key space): every pass reads the reads
                else ++sweeps;
            }
            if (rec_l0) { /* done above */ }
            else if (l0_try && p < l0_lo + l0_n) {
                const u64 nk_in = l0_keys[p - l0_lo];
                rc = run_one_pass<W>(ctx, false, reinterpret_cast<const Key*>(ctx->l0buf.as<u64>() + l0_base[p - l0_lo]), nk_in, 0, 0u, 1u, nk_in, &r);
            } else { rc = run_one_pass<W>(ctx, from_reads, d_keys_in, nkeys_in, nwords, p, npass, cap, &r); if (from_reads) ++sweeps; }
            if (rc) return rc;
            if (r.too_big) { too_big = true; seen = r.keys_seen; break; }
            pl = r.plan;
            const u64 ns = r.rows;
            tot_kmers += r.kmers; tot_distinct += r.distinct;
            if (npass > 1) {      // append this pass's rows and histogram to the job's
                CK(hipMemcpyAsync(pass_hist.data(), ctx->ghist.p, pass_hist.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
                // grow once: the passes hold similar numbers of rows (hash-uniform), so size for all of them after the first
                const u64 want_rows = std::max<u64>(tot_rows + ns + 1, p == 0 ? (ns + ns / 8 + 1024) * npass : 0);
                const bool took = ctx->sink.took;                        // (the rows are in the accumulators already)
                const u64 keep_rows = tot_rows + (took ? ns : 0);
                ctx->sink = dskgpu_ctx::RowSink{};
                auto grow_rows = [&]() {
                    bool ok = ctx->acc_ab.ensure_keep(want_rows * 4, keep_rows * 4, ctx->stream) == 0;
                    for (int x = 0; x < W && ok; ++x) ok = ctx->acc_w[x].ensure_keep(want_rows * 8, keep_rows * 8, ctx->stream) == 0;
                    return ok;
                };
                if (!grow_rows()) {      // the rows need more than was kept for them: the key arrays of the group's remaining passes give way (those passes get a sweep of their own)
                    (void)hipGetLastError();
                    if (l0_n && ctx->l0buf.p) { ctx->l0buf.release(); l0_n = p + 1 - l0_lo; }
                    if (rec_l0 && ctx->l0buf.p) { ctx->l0buf.release(); r_hi = p + 1; }
                    if (!grow_rows()) return fail(ctx, DSKGPU_E_NOMEM, "row accumulation");
                }
                rows_sized = true;
                if (ns && !took) {
                    CK(hipMemcpyAsync(ctx->acc_ab.as<u32>() + tot_rows, ctx->out_ab.p, ns * 4, hipMemcpyDeviceToDevice, ctx->stream));
                    for (int x = 0; x < W; ++x)
                        CK(hipMemcpyAsync(ctx->acc_w[x].as<u64>() + tot_rows, ctx->out_w[x].p, ns * 8, hipMemcpyDeviceToDevice, ctx->stream));
                }
                CK(hipStreamSynchronize(ctx->stream));
                for (size_t i = 0; i < pass_hist.size(); ++i) ctx->hist[i] += pass_hist[i];
                ctx->resolve_marks();
                ctx->mark("start");
            }
            tot_rows += ns;
        }
        if (rec_l0) { ctx->sender.prepared = false; ctx->enc_fresh = false; }      // (packed / mat1 were the passes' scratch)
        if (restart) {          // the record layout did not hold for these reads: the same count on the key-array path
            ctx->rec_l0_off = true;
            ctx->resolve_marks();
            return run_pipeline<W>(ctx, from_reads, d_keys_in, nkeys_in);
        }
        if (too_big) {
            // the pass holds more keys than its buffers: give the passes that capacity (more passes would not make THAT pass
            // smaller); only when it exceeds what 32-bit offsets address, more passes
            if (seen + (1u << 20) < 0xFFFF0000ull && seen > cap_floor) cap_floor = seen + (1u << 20); else { npass *= 2; cap_floor = 0; }
            continue;
        }
        // ---------------- row order over all passes
        if (npass > 1) {      // make the accumulated rows the sort input
            std::swap(ctx->out_ab, ctx->acc_ab);
            for (int x = 0; x < W; ++x) std::swap(ctx->out_w[x], ctx->acc_w[x]);
        }
        if (const int rc = order_rows(ctx, tot_rows, npass)) return rc;
        ctx->resolve_marks();
        ctx->n_rows = tot_rows;
        ctx->stats.n_bytes = from_reads ? ctx->n_bytes : 0;
        ctx->stats.n_kmers = tot_kmers;
        ctx->stats.n_distinct = tot_distinct;
        ctx->stats.n_solid = tot_rows;
        ctx->stats.n_levels = (u32)pl.levels;
        ctx->stats.n_final_bins = pl.F;
        ctx->stats.n_passes = npass;
        ctx->stats.n_read_sweeps = npass > 1 ? sweeps : (from_reads ? 1 : 0);
        if (from_reads) ctx->last_rows = tot_rows;
        if (npass > 1) {      // the names go back: acc_* stays the job-sized buffer (it holds the result now), out_* the pass-sized one --
            std::swap(ctx->out_ab, ctx->acc_ab);      // left swapped, the next count grew the small one to job size again (10 GB of hipMalloc + hipFree per call)
            for (int x = 0; x < W; ++x) std::swap(ctx->out_w[x], ctx->acc_w[x]);
        }
        ctx->stats.n_partitions = rows_partitions(ctx);
        ctx->have_result = true;
        return DSKGPU_OK;
    }
}

template <int W>
int mg_scatter_impl(dskgpu_ctx* ctx, void* d_send, uint64_t* send_words) {
    typedef typename KeyT<W>::T Key;
    ctx->st_names.clear(); ctx->st_ms.clear(); ctx->marks.clear(); ctx->ev_used = 0;
    ctx->mark("start");
    u64 nwords = 0;
    int rc = encode_current(ctx, &nwords);
    if (rc) return rc;
    ctx->mark("encode");
    const u32 G = ctx->cfg.world_size;
    u32 nch1 = 0;
    build_descs1(ctx, nwords, Tile<W>::WORDS, (u64)ctx->num_cu * 8, &nch1);
    const u64 M1 = (u64)G * nch1;
    CK(ctx->scalars.ensure(SC_COUNT * 4));
    CK(ctx->descs1.ensure(ctx->h_descs1.size() * sizeof(ChunkDesc)));
    CK(hipMemcpyAsync(ctx->descs1.p, ctx->h_descs1.data(), ctx->h_descs1.size() * sizeof(ChunkDesc), hipMemcpyHostToDevice, ctx->stream));
    u32* h_sc = ctx->h_sc;
    std::memset(h_sc, 0, sizeof(ctx->h_sc));
    h_sc[SC_NCH1] = nch1; h_sc[SC_MLEN1] = (u32)M1;
    u32* sc = ctx->scalars.as<u32>();
    CK(hipMemcpyAsync(sc, h_sc, sizeof(ctx->h_sc), hipMemcpyHostToDevice, ctx->stream));
    CK(ctx->mat1.ensure((M1 + 1) * 4));
    const DigitSpec owner = DigitSpec{0u, G, 0u, G, 1u, 0u};
    if ((rc = launch_hist<W, 0>(ctx, nullptr, ctx->descs1.as<ChunkDesc>(), sc + SC_NCH1, nch1, ctx->mat1.as<u32>(), owner, G))) return rc;
    ctx->mark("mg_hist");
    if ((rc = run_scan(ctx, ctx->mat1.as<u32>(), sc + SC_MLEN1, M1))) return rc;
    if ((rc = launch_scatter<W, 0>(ctx, nullptr, ctx->descs1.as<ChunkDesc>(), sc + SC_NCH1, nch1, ctx->mat1.as<u32>(), static_cast<Key*>(d_send), owner, G))) return rc;
    ctx->mark("mg_scatter");
    ctx->h_starts.assign(G + 1, 0);
    for (u32 o = 0; o <= G; ++o)
        CK(hipMemcpyAsync(&ctx->h_starts[o], ctx->mat1.as<u32>() + (u64)o * nch1, 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    ctx->resolve_marks();
    for (u32 o = 0; o < G; ++o) send_words[o] = (u64)(ctx->h_starts[o + 1] - ctx->h_starts[o]) * W;
    return DSKGPU_OK;
}

// Receiver: records -> dense mixed keys -> the ordinary partition + count over a key array.
template <int W>
int sk_count(dskgpu_ctx* ctx, const u64* d_rec, u64 recv_words, u64 n_kmers_hint, bool hint_is_estimate = false) {
    typedef typename KeyT<W>::T Key;
    const u32 R = ctx->sender.sp.R;
    if (recv_words % R) return fail(ctx, DSKGPU_E_ARG, "recv_words is not a whole number of super-k-mer records");
    const u64 nrec = recv_words / R;
    if (hint_is_estimate && ctx->marks.size() > 1) {      // a sliced step: the sender's marks are still open (its launches returned at once)
        CK(hipStreamSynchronize(ctx->stream));
        ctx->resolve_marks();
    }
    ctx->marks.clear(); ctx->ev_used = 0;
    ctx->mark("start");
    u64 total = 0;
    ctx->rec_hint = 0; ctx->rec_sized = false; ctx->rec_hint_est = hint_is_estimate;
    if (nrec) {
        ctx->rec_src = d_rec; ctx->rec_n = nrec; ctx->rec_expanded = false;
        if (n_kmers_hint) { total = n_kmers_hint; ctx->rec_hint = n_kmers_hint; }      // the senders counted while they wrote the records
        else { const int e = sk_sizes(ctx, &total); if (e) return e; }
    } else {
        ctx->rec_src = nullptr; ctx->rec_n = 0;
        CK(ctx->sk_keys.ensure(sizeof(Key)));
    }
    ctx->mark("mg_sizes");
    CK(hipStreamSynchronize(ctx->stream));
    ctx->resolve_marks();
    if (!ctx->rec_src) { const int e = rec_gate_all(ctx); if (e) return e; return run_pipeline<W>(ctx, false, ctx->sk_keys.as<Key>(), 0); }
    int rc = run_pipeline<W>(ctx, false, nullptr, total);      // nullptr: keys come from ctx->rec_src
    if (rc == REC_RESIZE) { ctx->rec_hint_est = false; rc = run_pipeline<W>(ctx, false, nullptr, ctx->rec_hint); ctx->rec_hint = 0; }
    ctx->rec_src = nullptr;
    if (rc == DSKGPU_OK && ctx->rec_hint && !ctx->rec_hint_est && ctx->stats.n_kmers != ctx->rec_hint) {
        ctx->drop_result();
        return fail(ctx, DSKGPU_E_ARG, "dskgpu_mg_count_sized: n_kmers does not match the k-mers inside the records");
    }
    return rc;
}

}  // namespace

int count_reads(dskgpu_ctx* ctx) { return ctx->W == 1 ? run_pipeline<1>(ctx, true, nullptr, 0) : ctx->W == 2 ? run_pipeline<2>(ctx, true, nullptr, 0) : run_pipeline<4>(ctx, true, nullptr, 0); }

// =============================================================== C-ABI
extern "C" {

const char* dskgpu_version(void) { return DSKGPU_VERSION; }

int dskgpu_device_count(void) { int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }

const char* dskgpu_last_error(const dskgpu_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int dskgpu_create(const dskgpu_config* cfg, dskgpu_ctx** out) {
    if (!cfg || !out) { g_create_err = "null argument"; return DSKGPU_E_ARG; }
    *out = nullptr;
    if (cfg->kmer_size < 1 || cfg->kmer_size > 128) { g_create_err = "kmer_size must be in 1..128"; return DSKGPU_E_ARG; }
    if (cfg->solidity_kind > DSKGPU_SOLIDITY_CUSTOM) { g_create_err = "unknown solidity_kind"; return DSKGPU_E_ARG; }
    if (g_place_k < 0) { const char* e = getenv("DSKGPU_PLACE"); g_place_k = e ? atoi(e) : 0; }
    if ((cfg->flags & DSKGPU_F_PLACE) && g_place_k < 2) g_place_k = 8;
    const u32 ws = cfg->world_size ? cfg->world_size : 1;
    if ((ws & (ws - 1)) != 0 || ws > 64 || cfg->rank >= ws) { g_create_err = "world_size must be a power of two <= 64 and rank < world_size"; return DSKGPU_E_ARG; }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) { g_create_err = std::string("no HIP device: ") + hipGetErrorString(e); return DSKGPU_E_DEVICE; }
    if (cfg->device < 0 || cfg->device >= ndev) { g_create_err = "bad device ordinal"; return DSKGPU_E_ARG; }
    e = hipSetDevice(cfg->device);
    if (e != hipSuccess) { g_create_err = std::string("hipSetDevice: ") + hipGetErrorString(e); return DSKGPU_E_DEVICE; }
    dskgpu_ctx* ctx = new dskgpu_ctx();
    ctx->cfg = *cfg;
    ctx->cfg.world_size = ws;
    if (ctx->cfg.histo_max == 0) ctx->cfg.histo_max = 10000;
    if (ctx->cfg.abundance_max == 0) ctx->cfg.abundance_max = 0x7FFFFFFFu;
    if (ctx->cfg.minimizer_size == 0) ctx->cfg.minimizer_size = 10;
    ctx->W = cfg->kmer_size <= 32 ? 1 : cfg->kmer_size <= 64 ? 2 : 4;     // device keys: 1, 2 or 4 words (three-word keys for 65 <= k <= 96 were built and measured in r06: slower than the four-word path)
    ctx->words_out = (int)((cfg->kmer_size + 31) / 32);
    ctx->sentinel_ok = !sentinel_is_a_kmer(ctx->W, cfg->kmer_size);                   // words of a k-mer at the ABI (3 for k <= 96)
    ctx->max_keys_per_pass = (u64)cfg->max_pass_mkeys * 1000000ull;
    ctx->tune.read();
    // super-k-mer records need >= 16 m-mers per window (superkmer.h); shorter k-mers travel as explicit keys
    // (world_size == 1 is the degenerate exchange: every record goes to owner 0; dskgpu_count never looks at sk_mode)
    ctx->sk_mode = cfg->kmer_size >= 20 && cfg->kmer_size <= 64 && !(cfg->flags & DSKGPU_F_MG_EXPLICIT);
    if (ctx->sk_mode) {
        SkParams& sp = ctx->sender.sp;
        sp.k = cfg->kmer_size; sp.G = ws;
        sp.m = std::min<u32>(std::min<u32>(ctx->cfg.minimizer_size, 16u), cfg->kmer_size - 15u);
        sp.R = sk_record_words(cfg->kmer_size);
        ctx->l0_sender.sp = sp;      // (the same k, m and R; its G is the passes of the count that uses it)
    }
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && cus > 0) ctx->num_cu = cus; }      // (one attribute, not the whole property block)
    if (ctx->tune.num_cu) ctx->num_cu = (int)ctx->tune.num_cu;      // DSKGPU_NUM_CU (tests): no kernel waits for another block, so a grid sized for more or fewer CUs than the device has only runs in more or fewer rounds
    e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { g_create_err = std::string("hipStreamCreate: ") + hipGetErrorString(e); delete ctx; return DSKGPU_E_DEVICE; }
    ctx->own_stream = true;
    *out = ctx;
    return DSKGPU_OK;
}

void dskgpu_destroy(dskgpu_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->cfg.device);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->release();              // every owner frees what it holds: the count path, then the structured concerns
    ctx->reads.release(); ctx->banks.release(); ctx->rs.release(); ctx->sender.release(); ctx->l0_sender.release();
    ctx->drop_result();          // (query, unitigs, threading, variants, readsum, colors, filtered: it releases each of them, and says so)
    for (hipEvent_t e : ctx->ev_pool) (void)hipEventDestroy(e);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int dskgpu_set_stream(dskgpu_ctx* ctx, void* hip_stream) {
    if (!ctx) return DSKGPU_E_ARG;
    CK(hipSetDevice(ctx->cfg.device));
    CK(hipStreamSynchronize(ctx->stream));
    if (hip_stream) {
        if (ctx->own_stream) { (void)hipStreamDestroy(ctx->stream); ctx->own_stream = false; }
        ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
    } else if (!ctx->own_stream) {
        CK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        ctx->own_stream = true;
    }
    return DSKGPU_OK;
}

int dskgpu_reserve_work(dskgpu_ctx* ctx, uint64_t nbytes) {
    if (!ctx) return DSKGPU_E_ARG;
    CK(hipSetDevice(ctx->cfg.device));
    // upper bounds from the byte count (every byte could end a k-mer): the encoded stream, the level-1 slices / the keys of a pass
    // (bufA), the level-2 regions + extension pool (bufB); DevBuf only ever grows, so dskgpu_count finds them in place
    const u64 max_keys = ctx->max_keys_per_pass ? ctx->max_keys_per_pass : 0xD0000000ull;
    const u64 n = std::min<u64>(nbytes + 1, max_keys + max_keys / 4);
    const u64 key = 8ull * (u64)ctx->W;
    const u64 nwords = (nbytes + 31) / 32;
    const u64 target = target_keys(ctx->W);
    const u64 F = n / target + 2, cap = opt_groups(ctx->W) * (8u / (u64)ctx->W);
    const u64 regions = F + (ctx->W == 1 ? F / 8 + 4096 : 0);
    {   // a reservation is a convenience: never more than 60 % of what is free (the sizes are upper bounds from a byte count; ranks that
        // share a device and DSKGPU_PLACE's candidates need room too) -- beyond that dskgpu_count sizes the buffers itself
        size_t free_b = 0, total_b = 0;
        const u64 want = (nwords + 1) * 12 + std::max<u64>((n + n / 8 + (1u << 20)) * key, ctx->W == 1 ? F * cap * 4 : 0) + (regions * cap + (1u << 16)) * key;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const u64 have = ctx->packed.cap + ctx->inval.cap + ctx->bufA.cap + ctx->bufB.cap;
            if (want > have && want - have > (u64)free_b * 6 / 10) return fail(ctx, DSKGPU_NOT_RESERVED, "dskgpu_reserve_work: the reservation exceeds 60 % of the free device memory (nothing was reserved; dskgpu_count sizes its own buffers)");
        }
    }
    // (after dskgpu_encode_reads the encoded stream is the ONLY copy of the reads and DevBuf::ensure does not keep contents: it stays)
    if (!ctx->enc_keep) {
        CK(ctx->packed.ensure((nwords + 1) * 8));
        CK(ctx->inval.ensure((nwords + 1) * 4));
    }
    CK(ctx->bufA.ensure(std::max<u64>((n + n / 8 + (1u << 20)) * key, ctx->W == 1 ? F * cap * 4 : 0)));
    CK(ctx->bufB.ensure((regions * cap + (1u << 16)) * key));
    if (ctx->W > 1) CK(ctx->abund2.ensure((F * cap + (1u << 16)) * 4));
    return DSKGPU_OK;
}

int dskgpu_encode_reads(dskgpu_ctx* ctx) {
    if (!ctx) return DSKGPU_E_ARG;
    CK(hipSetDevice(ctx->cfg.device));
    RAW_SYNC(ctx);
    if (ctx->enc_keep) return DSKGPU_OK;
    if (!ctx->d_reads && ctx->n_bytes) return fail(ctx, DSKGPU_E_STATE, "no reads to encode");
    u64 nwords = 0;
    const int rc = run_encode(ctx, ctx->d_reads, ctx->n_bytes, &nwords);
    if (rc) return rc;
    CK(hipStreamSynchronize(ctx->stream));
    ctx->enc_keep = true;
    ctx->d_reads = nullptr;                    // the caller's buffer is never read again
    ctx->reads.own.release(); ctx->reads.len = 0;      // pushed reads: their ASCII copy in HBM goes too (a later push starts a new read set)
    return DSKGPU_OK;
}

int dskgpu_count(dskgpu_ctx* ctx) {
    if (!ctx) return DSKGPU_E_ARG;
    if (ctx->cfg.world_size != 1) return fail(ctx, DSKGPU_E_STATE, "dskgpu_count needs world_size == 1; use dskgpu_mg_scatter/_mg_count");
    CK(hipSetDevice(ctx->cfg.device));
    RAW_SYNC(ctx);
    ctx->stats = dskgpu_stats{};
    if (per_bank_job(ctx)) return run_banks(ctx);
    if (ctx->cfg.flags & DSKGPU_F_HISTO2D) ctx->banks.forget_hist2d();
    return count_reads(ctx);
}

uint64_t dskgpu_mg_send_capacity_words(dskgpu_ctx* ctx) {
    if (!ctx) return 0;
    if (ctx->reads.raw_pending && (hipSetDevice(ctx->cfg.device) != hipSuccess || raw_finish(ctx, nullptr) != DSKGPU_OK)) return 0;
    if (!ctx->sk_mode) return (ctx->n_bytes + 1) * (u64)ctx->W;
    if (hipSetDevice(ctx->cfg.device) != hipSuccess) return 0;
    return sk_send_capacity_words(ctx);
}

int dskgpu_mg_scatter(dskgpu_ctx* ctx, void* d_send, uint64_t capacity_words, uint64_t* send_words) {
    if (!ctx || !d_send || !send_words) return DSKGPU_E_ARG;
    CK(hipSetDevice(ctx->cfg.device));
    RAW_SYNC(ctx);
    if (ctx->sk_mode) return sk_scatter(ctx, d_send, capacity_words, send_words);
    // (explicit keys -- k < 20, k > 64 or DSKGPU_F_MG_EXPLICIT -- keep 32-bit key offsets in the send buffer: one key per byte at most)
    if (ctx->n_bytes >= 0xFFFF0000ull) return fail(ctx, DSKGPU_E_ARG, "explicit-key exchange: a rank's read shard must stay below 4.29 GB (super-k-mer records, 20 <= k <= 64, have no such limit)");
    if (capacity_words < dskgpu_mg_send_capacity_words(ctx)) return fail(ctx, DSKGPU_E_ARG, "send buffer too small");
    const int rc = ctx->W == 1 ? mg_scatter_impl<1>(ctx, d_send, send_words) : ctx->W == 2 ? mg_scatter_impl<2>(ctx, d_send, send_words) : mg_scatter_impl<4>(ctx, d_send, send_words);
    if (rc == DSKGPU_OK) for (u32 o = 0; o < ctx->cfg.world_size; ++o) ctx->sender.h_sent[o] = send_words[o] / (u64)ctx->W;
    return rc;
}

int dskgpu_mg_count(dskgpu_ctx* ctx, const void* d_recv, uint64_t recv_words) { return dskgpu_mg_count_sized(ctx, d_recv, recv_words, 0); }

int dskgpu_mg_count_sliced(dskgpu_ctx* ctx, const void* d_recv, uint32_t nslices, const uint64_t* slice_words, uint64_t n_kmers_est,
                           dskgpu_slice_gate gate, void* user) {
    if (!ctx || !nslices || !slice_words || !gate) return DSKGPU_E_ARG;
    if (!ctx->sk_mode) return fail(ctx, DSKGPU_E_STATE, "dskgpu_mg_count_sliced needs super-k-mer records (20 <= k <= 64, no DSKGPU_F_MG_EXPLICIT)");
    CK(hipSetDevice(ctx->cfg.device));
    ctx->stats = dskgpu_stats{};
    const u32 R = ctx->sender.sp.R;
    u64 words = 0;
    ctx->rec_slice_end.clear();
    for (u32 sl = 0; sl < nslices; ++sl) {
        if (slice_words[sl] % R) { ctx->rec_slice_end.clear(); return fail(ctx, DSKGPU_E_ARG, "a slice is not a whole number of super-k-mer records"); }
        words += slice_words[sl];
        ctx->rec_slice_end.push_back(words / R);
    }
    if (!d_recv && words) { ctx->rec_slice_end.clear(); return DSKGPU_E_ARG; }
    ctx->rec_gate = gate; ctx->rec_gate_user = user; ctx->rec_gated = 0; ctx->rec_gate_failed = false;
    int rc = ctx->W == 1 ? sk_count<1>(ctx, static_cast<const u64*>(d_recv), words, n_kmers_est, true)
                         : sk_count<2>(ctx, static_cast<const u64*>(d_recv), words, n_kmers_est, true);
    const std::string err = ctx->err;
    (void)rec_gate_all(ctx);                             // (an error path may have left early: the caller's gates are all passed when this returns)
    if (ctx->rec_gate_failed) { ctx->drop_result(); if (rc == DSKGPU_OK) rc = DSKGPU_E_STATE; else ctx->err = err; }
    ctx->rec_gate = nullptr; ctx->rec_gate_user = nullptr; ctx->rec_slice_end.clear();
    return rc;
}

int dskgpu_mg_count_sized(dskgpu_ctx* ctx, const void* d_recv, uint64_t recv_words, uint64_t n_kmers) {
    if (!ctx || (!d_recv && recv_words)) return DSKGPU_E_ARG;
    CK(hipSetDevice(ctx->cfg.device));
    ctx->stats = dskgpu_stats{};
    if (ctx->sk_mode)
        return ctx->W == 1 ? sk_count<1>(ctx, static_cast<const u64*>(d_recv), recv_words, n_kmers) : sk_count<2>(ctx, static_cast<const u64*>(d_recv), recv_words, n_kmers);
    if (n_kmers && n_kmers != recv_words / (u64)ctx->W) return fail(ctx, DSKGPU_E_ARG, "dskgpu_mg_count_sized: n_kmers does not match the k-mers received");
    if (recv_words % (u64)ctx->W) return fail(ctx, DSKGPU_E_ARG, "recv_words is not a whole number of k-mer records");
    if (!d_recv) { CK(ctx->sk_keys.ensure(64)); d_recv = ctx->sk_keys.p; }      // nothing received: a null key array would read as "keys come from records"
    if (ctx->W == 1) return run_pipeline<1>(ctx, false, static_cast<const u64*>(d_recv), recv_words);
    if (ctx->W == 2) return run_pipeline<2>(ctx, false, static_cast<const K2*>(d_recv), recv_words / 2);
    return run_pipeline<4>(ctx, false, static_cast<const KN<4>*>(d_recv), recv_words / 4);
}

int dskgpu_get_stats(const dskgpu_ctx* ctx, dskgpu_stats* out) {
    if (!ctx || !out) return DSKGPU_E_ARG;
    if (!ctx->have_result) return DSKGPU_E_STATE;
    *out = ctx->stats;
    return DSKGPU_OK;
}

int dskgpu_histogram(const dskgpu_ctx* ctx, uint64_t* out, uint32_t nbins) {
    if (!ctx || !out) return DSKGPU_E_ARG;
    if (!ctx->have_result) return DSKGPU_E_STATE;
    if (nbins != ctx->cfg.histo_max + 1) return DSKGPU_E_ARG;
    std::memcpy(out, ctx->hist.data(), (size_t)nbins * 8);
    return DSKGPU_OK;
}

int dskgpu_set_row_order(dskgpu_ctx* ctx, int partition_order) {
    if (!ctx) return DSKGPU_E_ARG;
    if (partition_order) ctx->cfg.flags |= DSKGPU_F_PARTITION_ORDER; else ctx->cfg.flags &= ~DSKGPU_F_PARTITION_ORDER;
    return DSKGPU_OK;
}

uint32_t dskgpu_num_partitions(const dskgpu_ctx* ctx) { return (ctx && ctx->have_result) ? ctx->stats.n_partitions : 0; }

uint64_t dskgpu_partition_size(const dskgpu_ctx* ctx, uint32_t p) {
    if (!ctx || !ctx->have_result || p >= ctx->stats.n_partitions) return 0;
    u64 b, e; rows_partition_range(ctx, p, &b, &e); return e - b;
}

int dskgpu_partition_offsets(const dskgpu_ctx* ctx, uint64_t* offsets) {
    if (!ctx || !offsets) return DSKGPU_E_ARG;
    if (!ctx->have_result) return DSKGPU_E_STATE;
    const u32 P = ctx->stats.n_partitions;
    for (u32 p = 0; p < P; ++p) { u64 b, e; rows_partition_range(ctx, p, &b, &e); offsets[p] = b; if (p + 1 == P) offsets[P] = e; }
    if (P == 0) offsets[0] = 0;
    return DSKGPU_OK;
}

int dskgpu_partition_copy(const dskgpu_ctx* cctx, uint32_t p, uint64_t* kmers, uint32_t* abundance) {
    dskgpu_ctx* ctx = const_cast<dskgpu_ctx*>(cctx);
    if (!ctx) return DSKGPU_E_ARG;
    if (!ctx->have_result) return DSKGPU_E_STATE;
    if (p >= ctx->stats.n_partitions) return DSKGPU_E_ARG;
    u64 b, e; rows_partition_range(ctx, p, &b, &e);
    const u64 n = e - b;
    if (n == 0) return DSKGPU_OK;
    CK(hipSetDevice(ctx->cfg.device));
    if (kmers) {
        if (ctx->W == 1) CK(hipMemcpy(kmers, ctx->res_w[0] + b, n * 8, hipMemcpyDeviceToHost));
        else {
            // the device keeps one array per word; rows are words_out consecutive words on the host side
            const int wo = ctx->words_out;
            std::vector<u64> col(n);
            for (int x = 0; x < wo; ++x) {
                CK(hipMemcpy(col.data(), ctx->res_w[x] + b, n * 8, hipMemcpyDeviceToHost));
                for (u64 i = 0; i < n; ++i) kmers[(u64)wo * i + x] = col[i];
            }
        }
    }
    if (abundance) CK(hipMemcpy(abundance, ctx->res_ab + b, n * 4, hipMemcpyDeviceToHost));
    return DSKGPU_OK;
}

int dskgpu_result_device(const dskgpu_ctx* ctx, const void** d_kmers, const void** d_abundance, uint64_t* n_rows) {
    if (!ctx) return DSKGPU_E_ARG;
    if (!ctx->have_result) return DSKGPU_E_STATE;
    if (d_kmers) *d_kmers = ctx->res_w[0];
    if (d_abundance) *d_abundance = ctx->res_ab;
    if (n_rows) *n_rows = ctx->n_rows;
    return DSKGPU_OK;
}

int dskgpu_stage_times(const dskgpu_ctx* ctx, const char** names, float* ms, int cap) {
    if (!ctx) return DSKGPU_E_ARG;
    const int n = (int)ctx->st_names.size();
    for (int i = 0; i < n && i < cap; ++i) { if (names) names[i] = ctx->st_names[i]; if (ms) ms[i] = ctx->st_ms[i]; }
    return n;
}

int dskgpu_k_encode(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, void* d_packed, void* d_invalid) {
    if (!ctx || !d_packed || !d_invalid) return DSKGPU_E_ARG;
    CK(hipSetDevice(ctx->cfg.device));
    u64 nwords = 0;
    if (ctx->enc_keep) { ctx->enc_keep = false; }      // (a test hook that encodes other bytes: the kept 2-bit form of the reads is overwritten)
    int rc = run_encode(ctx, static_cast<const uint8_t*>(d_bytes), nbytes, &nwords);
    if (rc) return rc;
    CK(hipMemcpyAsync(d_packed, ctx->packed.p, nwords * 8, hipMemcpyDeviceToDevice, ctx->stream));
    CK(hipMemcpyAsync(d_invalid, ctx->inval.p, nwords * 4, hipMemcpyDeviceToDevice, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return DSKGPU_OK;
}

int dskgpu_k_enumerate(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, void* d_kmers, void* d_valid) {
    if (!ctx || !d_kmers || !d_valid) return DSKGPU_E_ARG;
    CK(hipSetDevice(ctx->cfg.device));
    u64 nwords = 0;
    if (ctx->enc_keep) { ctx->enc_keep = false; }      // (a test hook that encodes other bytes: the kept 2-bit form of the reads is overwritten)
    int rc = run_encode(ctx, static_cast<const uint8_t*>(d_bytes), nbytes, &nwords);
    if (rc) return rc;
    if (nwords) {
        const unsigned grid = (unsigned)((nwords * 2 + 255) / 256);
        if (ctx->W == 1)
            hipLaunchKernelGGL(k_enumerate<1>, dim3(grid), dim3(256), 0, ctx->stream, ctx->packed.as<u64>(), ctx->inval.as<u32>(),
                               nwords, (u64)nbytes, (int)ctx->cfg.kmer_size, static_cast<u64*>(d_kmers), static_cast<uint8_t*>(d_valid), 1);
        else if (ctx->W == 2)
            hipLaunchKernelGGL(k_enumerate<2>, dim3(grid), dim3(256), 0, ctx->stream, ctx->packed.as<u64>(), ctx->inval.as<u32>(),
                               nwords, (u64)nbytes, (int)ctx->cfg.kmer_size, static_cast<u64*>(d_kmers), static_cast<uint8_t*>(d_valid), ctx->words_out);
        else
            hipLaunchKernelGGL(k_enumerate<4>, dim3(grid), dim3(256), 0, ctx->stream, ctx->packed.as<u64>(), ctx->inval.as<u32>(),
                               nwords, (u64)nbytes, (int)ctx->cfg.kmer_size, static_cast<u64*>(d_kmers), static_cast<uint8_t*>(d_valid), ctx->words_out);
        CKL("k_enumerate");
    }
    CK(hipStreamSynchronize(ctx->stream));
    return DSKGPU_OK;
}

int dskgpu_k_minimizers(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, void* d_minim, void* d_valid) {
    if (!ctx || !d_minim || !d_valid) return DSKGPU_E_ARG;
    const int m = (int)ctx->cfg.minimizer_size, k = (int)ctx->cfg.kmer_size;
    if (m < 1 || m > 16 || m > k) return fail(ctx, DSKGPU_E_ARG, "minimizer_size must be in 1..16 and <= kmer_size");
    CK(hipSetDevice(ctx->cfg.device));
    u64 nwords = 0;
    if (ctx->enc_keep) { ctx->enc_keep = false; }      // (a test hook that encodes other bytes: the kept 2-bit form of the reads is overwritten)
    int rc = run_encode(ctx, static_cast<const uint8_t*>(d_bytes), nbytes, &nwords);
    if (rc) return rc;
    if (nbytes) {
        const u64 nthreads = (nbytes + 15) / 16;
        hipLaunchKernelGGL(k_minimizers, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, ctx->stream, ctx->packed.as<u64>(),
                           ctx->inval.as<u32>(), nwords, (u64)nbytes, k, m, static_cast<u32*>(d_minim), static_cast<uint8_t*>(d_valid));
        CKL("k_minimizers");
    }
    CK(hipStreamSynchronize(ctx->stream));
    return DSKGPU_OK;
}

}  // extern "C"
