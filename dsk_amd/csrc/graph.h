// graph.h -- HIP kernels of the de Bruijn neighbourhood of k-mers in the last result (gfx950 / MI355X, wave64):
// dskgpu_graph_adjacency / dskgpu_graph_neighbors (graph.hip).
//
// adj(x) is one byte: bit b (0..3) <=> canonical(succ_b(x)) is a row, bit 4 + b <=> canonical(pred_b(x)) is a row, with
//
//   succ_b(x) = s[1..k-1] . b = ((x << 2) | b) & (4^k - 1)            pred_b(x) = b . s[0..k-2] = (x >> 2) | (b << 2(k-1))
//
// The reverse complement is computed ONCE per value, with the word reversal gen_kmersN uses for the first window of a thread; the
// eight neighbours' reverse complements follow from it by the recurrences that gen_kmers* apply per base:
//
//   rc(succ_b(x)) = (rc(x) >> 2) | ((b ^ 2) << 2(k-1))                rc(pred_b(x)) = ((rc(x) << 2) | (b ^ 2)) & (4^k - 1)
//
// so a neighbour costs two multi-word shift-ors and one multi-word compare.  The eight canonical values of a value are probed as one
// batch of independent chains by q_lookup (query.h), the only probe of the index there is: nothing here touches the table itself.
//
//   k_graph_rows<W>       adj() of every row of the result (read coalesced from the struct-of-arrays rows) -> one byte per row and / or
//                         the 5 x 5 table "rows with i predecessors and o successors"
//   k_graph_neighbors<W>  adj() of the values in a caller's array (the layout of k_query_kmers)
//
// Both are loaders around graph_adj<W, R>.  Rows per thread follow QBatch's budget of 16 key-words in flight: R = 2 rows (16 keys)
// for one-word keys, one row (8 keys) for two-word keys; a four-word row is probed in two halves of 4 keys (successors, then
// predecessors) -- the choice between that and one batch of 8 is G_W4_HALVES, made by the resource report (profiles/graph_adjacency.md).
#pragma once
#include "query.h"

#ifndef G_W4_HALVES
#define G_W4_HALVES 1
#endif
template <int W> struct GBatch { static constexpr int R = W == 1 ? 2 : 1; static constexpr bool HALVES = W == 4 && G_W4_HALVES; };

#define G_DEG_CELLS 25                    // degrees[i * 5 + o]: i predecessors, o successors

// msk[i] = the bits of word i that belong to a k-mer of k bases (2k bits, word 0 least significant)
template <int W> __device__ __forceinline__ void g_masks(int k, u64 (&msk)[W]) {
#pragma unroll
    for (int i = 0; i < W; ++i) { const int bits = 2 * k - 64 * i; msk[i] = bits >= 64 ? ~0ull : bits <= 0 ? 0ull : ((1ull << bits) - 1); }
}

// reverse complement of x (< 4^k): reverse all 32 W pairs, shift right by 64 W - 2k bits, complement k pairs.  The shift is 0 at
// k = 32 W and reaches whole words for four-word keys with k <= 96: words first, then the bits left (never a 64-bit shift by 64)
template <int W> __device__ __forceinline__ KN<W> g_revcomp(const KN<W>& x, int k, const u64 (&msk)[W]) {
    KN<W> r;
#pragma unroll
    for (int i = 0; i < W; ++i) r.w[i] = rev_pairs(x.w[W - 1 - i]);
    const int sh = 64 * W - 2 * k;
    const int ws = sh >> 6, bs = sh & 63;
#pragma unroll
    for (int s = 0; s < W - 1; ++s)
        if (ws > s) {
#pragma unroll
            for (int i = 0; i < W - 1; ++i) r.w[i] = r.w[i + 1];
            r.w[W - 1] = 0ull;
        }
    if (bs) {
#pragma unroll
        for (int i = 0; i < W - 1; ++i) r.w[i] = (r.w[i] >> bs) | (r.w[i + 1] << (64 - bs));
        r.w[W - 1] >>= bs;
    }
#pragma unroll
    for (int i = 0; i < W; ++i) r.w[i] ^= 0xAAAAAAAAAAAAAAAAULL & msk[i];
    return r;
}

// (a << 2 | low) & 4^k - 1
template <int W> __device__ __forceinline__ KN<W> g_push_low(const KN<W>& a, u64 low, const u64 (&msk)[W]) {
    KN<W> o;
#pragma unroll
    for (int i = W - 1; i >= 1; --i) o.w[i] = ((a.w[i] << 2) | (a.w[i - 1] >> 62)) & msk[i];
    o.w[0] = ((a.w[0] << 2) | low) & msk[0];
    return o;
}
// (a >> 2) | top << 2(k-1): the base enters at bit tb of word tw (word 0 at k = 32, word 1 at k = 33, ...)
template <int W> __device__ __forceinline__ KN<W> g_push_top(const KN<W>& a, u64 top, int tw, int tb) {
    KN<W> o;
#pragma unroll
    for (int i = 0; i < W - 1; ++i) o.w[i] = (a.w[i] >> 2) | (a.w[i + 1] << 62);
    o.w[W - 1] = a.w[W - 1] >> 2;
#pragma unroll
    for (int i = 0; i < W; ++i) o.w[i] |= (i == tw) ? (top << tb) : 0ull;
    return o;
}
template <int W> __device__ __forceinline__ KN<W> g_min(const KN<W>& f, const KN<W>& r) {
    bool lt = false, decided = false;                        // f < r, most significant word first
#pragma unroll
    for (int i = W - 1; i >= 0; --i) { if (!decided && f.w[i] != r.w[i]) { lt = f.w[i] < r.w[i]; decided = true; } }
    KN<W> o;
#pragma unroll
    for (int i = 0; i < W; ++i) o.w[i] = lt ? f.w[i] : r.w[i];
    return o;
}

// c[0..3] = canonical(succ_b(x)), b = 0..3 (PRED: canonical(pred_b(x))), given r = rc(x)
template <int W, bool PRED>
__device__ __forceinline__ void g_four(const KN<W>& x, const KN<W>& r, int k, const u64 (&msk)[W], KN<W>* c) {
    const int top = 2 * k - 2, tw = top >> 6, tb = top & 63;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        if constexpr (PRED) c[b] = g_min<W>(g_push_top<W>(x, (u64)b, tw, tb), g_push_low<W>(r, (u64)(b ^ 2), msk));
        else c[b] = g_min<W>(g_push_low<W>(x, (u64)b, msk), g_push_top<W>(r, (u64)(b ^ 2), tw, tb));
    }
}

// adj[i] = adj(x[i]) for the values whose bit is set in `live`, 0 for the others
template <int W, int R>
__device__ __forceinline__ void graph_adj(const QTable& T, const KN<W> (&x)[R], u32 live, int k, u32 (&adj)[R]) {
    u64 msk[W];
    g_masks<W>(k, msk);
    if constexpr (GBatch<W>::HALVES) {
        static_assert(R == 1, "a row in two halves: one row per thread");
        const KN<W> r = g_revcomp<W>(x[0], k, msk);
        const u32 pend = (live & 1u) ? 0xFu : 0u;
        KN<W> c[4]; u32 res[4];
        adj[0] = 0u;
        g_four<W, false>(x[0], r, k, msk, c);
        q_lookup<W, 4>(T, c, pend, res);
#pragma unroll
        for (int b = 0; b < 4; ++b) adj[0] |= res[b] ? (1u << b) : 0u;
        g_four<W, true>(x[0], r, k, msk, c);
        q_lookup<W, 4>(T, c, pend, res);
#pragma unroll
        for (int b = 0; b < 4; ++b) adj[0] |= res[b] ? (16u << b) : 0u;
    } else {
        KN<W> c[8 * R]; u32 res[8 * R];
        u32 pend = 0;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const KN<W> r = g_revcomp<W>(x[i], k, msk);
            g_four<W, false>(x[i], r, k, msk, &c[8 * i]);
            g_four<W, true>(x[i], r, k, msk, &c[8 * i + 4]);
            if ((live >> i) & 1u) pend |= 0xFFu << (8 * i);
        }
        q_lookup<W, 8 * R>(T, c, pend, res);
#pragma unroll
        for (int i = 0; i < R; ++i) {
            adj[i] = 0u;
#pragma unroll
            for (int j = 0; j < 8; ++j) adj[i] |= res[8 * i + j] ? (1u << j) : 0u;
        }
    }
}

// the two bits of base j (0 = last base) of x, and the letter of a code: what unitigs.h and variants.h write sequences with
template <int W> __device__ __forceinline__ u32 u_base(const KN<W>& x, int j) {
    const int wi = (2 * j) >> 6;
    u64 word = x.w[0];
#pragma unroll
    for (int q = 1; q < W; ++q) word = (wi == q) ? x.w[q] : word;
    return (u32)(word >> ((2 * j) & 63)) & 3u;
}
__device__ __forceinline__ unsigned char u_letter(u32 code) { return (unsigned char)(0x47544341u >> (8u * code)); }      // "ACTG"

// A block takes 256 * R consecutive rows, thread t of it the rows t, t + 256, ...: a wave reads 64 neighbouring words of every word
// array and writes 64 neighbouring bytes.  d_adj may be null (degree table only), deg may be null (bytes only).  The degree table is
// counted per block in LDS and leaves as one vector atomic add per non-zero cell and block.
template <int W>
__global__ __launch_bounds__(256) void k_graph_rows(RowsIn rows, u64 n, int k, QTable T, unsigned char* __restrict__ d_adj, u64* __restrict__ deg) {
    constexpr int R = GBatch<W>::R;
    __shared__ u32 s_deg[G_DEG_CELLS];
    if (threadIdx.x < G_DEG_CELLS) s_deg[threadIdx.x] = 0u;
    __syncthreads();
    const u64 base = (u64)blockIdx.x * (256u * R) + threadIdx.x;
    KN<W> x[R];
    u32 live = 0;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const u64 r = base + (u64)i * 256u;
        const bool in = r < n;
#pragma unroll
        for (int q = 0; q < W; ++q) x[i].w[q] = in ? rows.w[q][r] : 0ull;
        if (in) live |= 1u << i;
    }
    u32 adj[R];
    graph_adj<W, R>(T, x, live, k, adj);
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const u64 r = base + (u64)i * 256u;
        if (r < n) {
            if (d_adj) d_adj[r] = (unsigned char)adj[i];
            if (deg) atomicAdd(&s_deg[__popc(adj[i] >> 4) * 5 + __popc(adj[i] & 15u)], 1u);
        }
    }
    if (deg) {
        __syncthreads();
        if (threadIdx.x < G_DEG_CELLS && s_deg[threadIdx.x]) atomicAdd(&deg[threadIdx.x], (u64)s_deg[threadIdx.x]);
    }
}

// keys[i * ow + q] = word q of value i (ow = ceil(k / 32) words at the ABI; the device key's words above them are zero).  A value with
// a bit at or above 2k in its ABI words is no k-mer: it answers 0 without a probe.
template <int W>
__global__ __launch_bounds__(256) void k_graph_neighbors(const u64* __restrict__ keys, u64 n, int ow, int k, QTable T, unsigned char* __restrict__ d_adj) {
    constexpr int R = GBatch<W>::R;
    const u64 base = (u64)blockIdx.x * (256u * R) + threadIdx.x;
    u64 msk[W];
    g_masks<W>(k, msk);
    KN<W> x[R];
    u32 live = 0;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const u64 v = base + (u64)i * 256u;
        const bool in = v < n;
        bool kmer = in;
#pragma unroll
        for (int q = 0; q < W; ++q) {
            x[i].w[q] = (in && q < ow) ? keys[v * (u64)ow + q] : 0ull;
            kmer = kmer && (x[i].w[q] & ~msk[q]) == 0ull;
        }
        if (kmer) live |= 1u << i;
    }
    u32 adj[R];
    graph_adj<W, R>(T, x, live, k, adj);
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const u64 v = base + (u64)i * 256u;
        if (v < n) d_adj[v] = (unsigned char)adj[i];
    }
}
