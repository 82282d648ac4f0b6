// thread.h -- HIP kernels that thread reads through the compacted de Bruijn graph (gfx950 / MI355X, wave64): dskgpu_thread_*
// (thread.hip; the definition is in include/dskgpu.h).
//
// The PLACEMENT of the window ending at byte p: its canonical k-mer is row r, read forward (s = 0) or as the reverse complement (s = 1);
// with unitig[r] = u and pos[r] = (i << 1) | s_r the window is letter j of the oriented unitig U: (2u, i) when s == s_r, else
// (2u + 1, L[u] - 1 - i).  A WALK is a maximal run of placed positions; its STEPS are U of its first position and of every later
// position with j == 0 (an edge step: the read left one unitig for the next over an edge of the graph).
//
//   k_thread_place<W>   the frame of k_query_reads<W>: the N = 16 / W windows of a thread probed as a batch for their ROW NUMBERS
//                       (q_lookup<W, N, true>), then two more batched levels: unitig[r] and pos[r] of every hit, then the two offsets that
//                       give L[u], only for the windows read against their row.  The generators (kmer_device.h) return canonical values
//                       only; the orientation is derived here: the forward value of a window is a funnel shift over the packed words the
//                       thread holds anyway, and s = 0 <=> it equals the canonical value (a palindrome: equal, forward)
//   k_thread_count      per block of T_BLOCK positions: the walk heads, the steps and the placed positions in it (scanned by the host side).  The flags are never
//                       stored: head(p) = placed(p) && !placed(p - 1), step(p) = placed(p) && (!placed(p - 1) || j(p) == 0)
//   k_thread_emit       the same flags again, ranked inside the block (DPP wave scan of the per-thread counts + the waves' totals in LDS,
//                       no LDS atomics) on top of the scanned block sums: steps[], the walks' offsets / first / last / ends; an edge step
//                       looks U(p) up among the at most 4 targets of U(p - 1) and adds 1 to that edge; the unitig support as the sum of
//                       (end - start) over the stretches between two steps: the step subtracts its position, the last position of the
//                       stretch adds its own + 1 -- two no-return 64-bit atomics per step, none per position, exact modulo 2^64
//   k_thread_maxsteps   the most steps of one walk: a max-reduce over the walk offsets
//
// Global atomics: as in k_query_build, this is not the count path.
#pragma once
#include "query.h"

#define T_NONE 0xFFFFFFFFu
#define T_PER 4                           // positions per thread of k_thread_count / k_thread_emit: one 16-byte load of U and of j
#define T_BLOCK (256 * T_PER)             // positions per block of the two

enum TStat { TS_VALID = 0, TS_MAXSTEPS, TS_BROKEN, TS_COUNT };

// what a placement reads of the compaction (Unitigs): per row the unitig and (position << 1 | s), per unitig the stream offset
struct TGraph { const u32* unitig; const u32* pos; const u64* offsets; u64 n_rows, n_unitigs; int k; };
// ... and what an edge step reads of the edges
struct TEdges { const u64* offsets; const u32* targets; u64 n_or, n_edges; };
struct TWalks { u64 *offsets, *first, *last; u32 *steps, *ends; u64 n_walks, n_steps; };

// add `mine` of every thread of the block to *counter (64 bits): LDS first, one atomic per block that has something
__device__ __forceinline__ void t_block_count(u32 mine, u64* counter) {
    __shared__ u32 s_cnt;
    if (threadIdx.x == 0) s_cnt = 0u;
    __syncthreads();
    if (mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) q_add64(counter, (u64)s_cnt);
}

// Thread t: the N windows ending at bases 32 * (t / TPW) + (t % TPW) * N + j of the encoded stream, as k_query_reads.  out_u / out_j: either
// may be null.  ALIGNED: both are 16-byte aligned and a lane's N results leave as 16-byte stores.  stat (may be null): TS_VALID += the valid
// windows at positions < nbytes.  t_base: the first thread of this launch (a stream of more blocks than one launch takes)
template <int W, bool ALIGNED>
__global__ __launch_bounds__(256) void k_thread_place(const u64* __restrict__ packed, const u32* __restrict__ inval, u64 nwords, u64 nbytes, u64 t_base,
                                                      QTable T, TGraph G, u32* __restrict__ out_u, u32* __restrict__ out_j, u64* __restrict__ stat) {
    constexpr int N = QBatch<W>::N, TPW = 32 / N;
    const u64 t = t_base + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 wi = t / TPW;
    u32 nvalid = 0;
    if (wi < nwords) {
        const int t0 = (int)(t % TPW) * N;
        const int k = G.k;
        KN<W> c[N];
        u32 vm;
        if constexpr (W == 1) {
            u64 cc[N];
            vm = gen_kmers1<N>(packed, inval, wi, t0, k, cc);
#pragma unroll
            for (int j = 0; j < N; ++j) c[j].w[0] = cc[j];
        } else if constexpr (W == 2) vm = gen_kmers2<N>(packed, inval, wi, t0, k, c);
        else vm = gen_kmersN<W, N>(packed, inval, wi, t0, k, c);
        const u64 p0 = wi * 32 + (u64)t0;
        if (p0 + N > nbytes) vm &= p0 < nbytes ? ((1u << (u32)(nbytes - p0)) - 1u) : 0u;      // (the pad of the last word is invalid anyway)
        nvalid = __popc(vm);
        // the orientation: word i of the forward value = the 32 bases ending at base t of word wi - i, cut to the k-mer's bits
        u64 pw[W + 1];
#pragma unroll
        for (int q = 0; q <= W; ++q) pw[q] = wi >= (u64)q ? packed[wi - q] : 0ull;
        u32 ori = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int tt = t0 + j;
            bool same = true;
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const int bits = 2 * k - 64 * i;
                const u64 m = bits >= 64 ? ~0ull : bits <= 0 ? 0ull : ((1ull << bits) - 1);
                const u64 f = tt == 31 ? pw[i] : ((pw[i + 1] << (2 * tt + 2)) | (pw[i] >> (62 - 2 * tt)));
                same = same && ((f & m) == c[j].w[i]);
            }
            if (!same) ori |= 1u << j;
        }
        u32 row[N];
        q_lookup<W, N, true>(T, c, vm, row);                                         // levels 1 and 2: the slot, the row's key
        u32 un[N], ps[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {                                                // level 3: where the row lies
            const bool hit = row[j] < G.n_rows;                                      // (Q_NO_ROW is above every row number)
            un[j] = hit ? G.unitig[row[j]] : T_NONE;
            ps[j] = hit ? G.pos[row[j]] : 0u;
        }
        u32 len[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {                                                // level 4: L[u], for the windows read against their row
            const bool need = un[j] < G.n_unitigs && (((ps[j] ^ (ori >> j)) & 1u) != 0u);
            len[j] = need ? (u32)(G.offsets[un[j] + 1u] - G.offsets[un[j]] - (u64)k) : 0u;
        }
        u32 ru[N], rj[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const bool placed = un[j] < G.n_unitigs;                                 // (a row always has a unitig: the same guard as level 4)
            const bool against = ((ps[j] ^ (ori >> j)) & 1u) != 0u;
            ru[j] = placed ? 2u * un[j] + (against ? 1u : 0u) : T_NONE;
            rj[j] = placed ? (against ? len[j] - 1u - (ps[j] >> 1) : (ps[j] >> 1)) : 0u;
        }
        if (ALIGNED && p0 + N <= nbytes) {
#pragma unroll
            for (int q = 0; q < N / 4; ++q) {                                        // (p0 is a multiple of N >= 4)
                if (out_u) reinterpret_cast<uint4*>(out_u + p0)[q] = make_uint4(ru[4 * q], ru[4 * q + 1], ru[4 * q + 2], ru[4 * q + 3]);
                if (out_j) reinterpret_cast<uint4*>(out_j + p0)[q] = make_uint4(rj[4 * q], rj[4 * q + 1], rj[4 * q + 2], rj[4 * q + 3]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j)
                if (p0 + j < nbytes) {
                    if (out_u) out_u[p0 + j] = ru[j];
                    if (out_j) out_j[p0 + j] = rj[j];
                }
        }
    }
    if (stat) t_block_count(nvalid, stat + TS_VALID);
}

// The placements of the T_PER positions p0 .. of a thread with one neighbour on either side: u[0] / j[0] = position p0 - 1, u[1 + q] = p0 + q,
// u[T_PER + 1] = p0 + T_PER; T_NONE outside the stream.  U and J are 16-byte aligned arrays of the library's own.
__device__ __forceinline__ void t_window(const u32* __restrict__ U, const u32* __restrict__ J, u64 n, u64 p0, u32 (&u)[T_PER + 2], u32 (&j)[T_PER + 2]) {
    static_assert(T_PER == 4, "one uint4 per thread");
    if (p0 + T_PER <= n) {
        const uint4 a = *reinterpret_cast<const uint4*>(U + p0), b = *reinterpret_cast<const uint4*>(J + p0);
        u[1] = a.x; u[2] = a.y; u[3] = a.z; u[4] = a.w; j[1] = b.x; j[2] = b.y; j[3] = b.z; j[4] = b.w;
    } else {
#pragma unroll
        for (int q = 0; q < T_PER; ++q) { const bool in = p0 + q < n; u[1 + q] = in ? U[p0 + q] : T_NONE; j[1 + q] = in ? J[p0 + q] : 0u; }
    }
    const bool before = p0 > 0 && p0 - 1 < n, after = p0 + T_PER < n;
    u[0] = before ? U[p0 - 1] : T_NONE; j[0] = before ? J[p0 - 1] : 0u;
    u[T_PER + 1] = after ? U[p0 + T_PER] : T_NONE; j[T_PER + 1] = after ? J[p0 + T_PER] : 0u;
}

// heads[b] / nsteps[b] / nplaced[b] = the walk heads / the steps / the placed positions among the positions of block b (three sums per block,
// no counter that every block adds to: 1.5 M atomics on one address took longer than the pass over the placements)
__global__ __launch_bounds__(256) void k_thread_count(const u32* __restrict__ U, const u32* __restrict__ J, u64 n, u64 b_base,
                                                      u64* __restrict__ heads, u64* __restrict__ nsteps, u64* __restrict__ nplaced) {
    __shared__ u32 s_pair[4], s_placed[4];
    const u64 b = b_base + blockIdx.x;
    const u64 p0 = b * T_BLOCK + (u64)threadIdx.x * T_PER;
    u32 u[T_PER + 2], j[T_PER + 2];
    t_window(U, J, n, p0, u, j);
    u32 pair = 0, placed = 0;                                                         // heads | steps << 16
#pragma unroll
    for (int q = 1; q <= T_PER; ++q) {
        if (u[q] == T_NONE) continue;
        const bool head = u[q - 1] == T_NONE;
        ++placed;
        pair += (head ? 1u : 0u) + ((head || j[q] == 0u) ? 0x10000u : 0u);
    }
    pair = wave_incl_scan(pair); placed = wave_incl_scan(placed);
    if ((threadIdx.x & 63) == 63) { s_pair[threadIdx.x >> 6] = pair; s_placed[threadIdx.x >> 6] = placed; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const u32 tp = s_pair[0] + s_pair[1] + s_pair[2] + s_pair[3], pl = s_placed[0] + s_placed[1] + s_placed[2] + s_placed[3];
        heads[b] = (u64)(tp & 0xFFFFu); nsteps[b] = (u64)(tp >> 16); nplaced[b] = (u64)pl;
    }
}

// hbase[b] / sbase[b] = the walks / the steps before block b (the exclusive scans of k_thread_count's sums)
__global__ __launch_bounds__(256) void k_thread_emit(const u32* __restrict__ U, const u32* __restrict__ J, u64 n, u64 b_base,
                                                     const u64* __restrict__ hbase, const u64* __restrict__ sbase, TEdges E, u64 n_unitigs, TWalks Wk,
                                                     u64* __restrict__ usup, u64* __restrict__ esup, u64* __restrict__ stat) {
    __shared__ u32 s_pair[4];
    const u64 b = b_base + blockIdx.x;
    const u64 p0 = b * T_BLOCK + (u64)threadIdx.x * T_PER;
    u32 u[T_PER + 2], j[T_PER + 2];
    t_window(U, J, n, p0, u, j);
    u32 mine = 0;
#pragma unroll
    for (int q = 1; q <= T_PER; ++q) {
        if (u[q] == T_NONE) continue;
        const bool head = u[q - 1] == T_NONE;
        mine += (head ? 1u : 0u) + ((head || j[q] == 0u) ? 0x10000u : 0u);
    }
    const u32 incl = wave_incl_scan(mine);
    if ((threadIdx.x & 63) == 63) s_pair[threadIdx.x >> 6] = incl;
    __syncthreads();
    u32 excl = incl - mine;
    const u32 wave = threadIdx.x >> 6;
#pragma unroll
    for (u32 w = 0; w < 3; ++w) excl += w < wave ? s_pair[w] : 0u;
    u64 hrank = hbase[b] + (u64)(excl & 0xFFFFu), srank = sbase[b] + (u64)(excl >> 16);      // walks / steps before this thread's positions
    if (p0 == 0) Wk.offsets[Wk.n_walks] = Wk.n_steps;
    u32 broken = 0;
#pragma unroll
    for (int q = 1; q <= T_PER; ++q) {
        if (u[q] == T_NONE) continue;
        const u64 p = p0 + (u64)(q - 1);
        const bool head = u[q - 1] == T_NONE, edge = !head && j[q] == 0u;
        const bool last = u[q + 1] == T_NONE, stretch_end = last || j[q + 1] == 0u;
        const u64 un = u[q] >> 1;
        if (head) {
            if (hrank < Wk.n_walks) { Wk.offsets[hrank] = srank; Wk.first[hrank] = p; Wk.ends[2 * hrank] = j[q]; }
            ++hrank;
        }
        if (head || edge) {
            if (srank < Wk.n_steps) Wk.steps[srank] = u[q];
            ++srank;
            if (un < n_unitigs) q_add64(usup + un, 0ull - p);
        }
        if (stretch_end && un < n_unitigs) q_add64(usup + un, p + 1ull);
        if (edge) {                                                                   // U(p) among the targets of U(p - 1)
            const u64 from = u[q - 1];
            u64 e = ~0ull;
            if (from < E.n_or) {
                const u64 lo = E.offsets[from], hi = E.offsets[from + 1];
#pragma unroll
                for (u64 i = 0; i < 4; ++i)
                    if (lo + i < hi && lo + i < E.n_edges && E.targets[lo + i] == u[q]) e = lo + i;
            }
            if (e != ~0ull) q_add64(esup + e, 1ull); else ++broken;
        }
        if (last && hrank >= 1 && hrank - 1 < Wk.n_walks) { Wk.last[hrank - 1] = p; Wk.ends[2 * (hrank - 1) + 1] = j[q]; }
    }
    if (broken) q_add64(stat + TS_BROKEN, (u64)broken);
}

__global__ __launch_bounds__(256) void k_thread_maxsteps(const u64* __restrict__ offsets, u64 n_walks, u64* __restrict__ stat) {
    __shared__ u32 s_max;
    if (threadIdx.x == 0) s_max = 0u;
    __syncthreads();
    const u64 stride = (u64)gridDim.x * blockDim.x;
    u64 mx = 0;
    for (u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x; w < n_walks; w += stride) mx = max(mx, offsets[w + 1] - offsets[w]);
    // (a walk of 2^32 steps or more: straight to the global maximum)
    if (mx >> 32) atomicMax(reinterpret_cast<unsigned long long*>(stat + TS_MAXSTEPS), (unsigned long long)mx);
    else if (mx) atomicMax(&s_max, (u32)mx);
    __syncthreads();
    if (threadIdx.x == 0 && s_max) atomicMax(reinterpret_cast<unsigned long long*>(stat + TS_MAXSTEPS), (unsigned long long)s_max);
}
