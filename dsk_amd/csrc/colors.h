// colors.h -- HIP kernels of the sample colours (gfx950 / MI355X, wave64): dskgpu_colors_begin / _colors_add / _colors_rows /
// _colors_unitigs (colors.hip; the definitions are in include/dskgpu.h).
//
// The MATRIX is u32 C[n_rows][n_colors], row-major, in result order: C[r][c] = the valid windows of colour c whose canonical k-mer is row r.
//
//   k_color_reads<W>   the frame of k_query_reads<W>: the N = 16 / W windows of a thread probed as one batch for their ROW NUMBERS
//                      (q_lookup<W, N, true>).  The bank ends travel as a kernel argument (COL_MAX u64); a thread's N positions are
//                      consecutive, so it finds the bank of its first position once and walks on from there.  A position behind the last
//                      end has no bank: its window is taken out of the batch before the probe.  After the probe a lane merges the RUNS of
//                      equal (row, colour) among its N results into one no-return add of the run length (a homopolymer otherwise sends N
//                      adds of one lane to one address; COL_NO_MERGE, an experiment switch, leaves one add per hit: profiles/colors.md).
//                      n_valid / n_placed: combined per block first (col_block_counts), one add each
//   k_color_mask<VEC>  one thread per row: its mask (bit c: C[r][c] >= min_count) and, when asked, the copy of its cells.  VEC: n_colors
//                      is a multiple of 4 and the copy's target is 16-byte aligned: 16-byte loads and stores
//   k_color_fill64     all[u] = the n_colors low bits
//   k_color_unitigs    one thread per row: its non-zero cells onto sum[unitig[r]], its mask into any / all.  Plain 64-bit agent-scope
//                      atomics, as k_unitig_number
//
// Global atomics: integer adds, ORs and ANDs only; they commute, so nothing that is reported depends on their order.
#pragma once
#include "query.h"

#define COL_MAX 64                        // colours of a matrix, and banks of one call, at the most: a mask is one u64
#define COL_NONE 0xFFFFFFFFu              // the colour of a position behind the last end

enum ColStat { COL_ST_VALID = 0, COL_ST_PLACED, COL_ST_COUNT };

// end[b], b < n: the non-decreasing ends of the call's banks; colour of bank b = first + b
struct ColBanks { u64 end[COL_MAX]; u32 n, first; };

__device__ __forceinline__ void col_add32(u32* at, u32 v) {
    (void)__hip_atomic_fetch_add(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// stat[i] += the sum over the block of mine[i], i < COL_ST_COUNT: LDS first, one add per counter and block that has something (as
// rs_block_counts of readsum.h, which only readsum.hip may include: its kernels are no templates).  Every thread of the block calls it, once
__device__ __forceinline__ void col_block_counts(const u32 (&mine)[COL_ST_COUNT], u64* stat) {
    __shared__ u32 s_cnt[COL_ST_COUNT];
    if (threadIdx.x < COL_ST_COUNT) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < COL_ST_COUNT; ++i) if (mine[i]) atomicAdd(&s_cnt[i], mine[i]);
    __syncthreads();
    if (threadIdx.x < COL_ST_COUNT && s_cnt[threadIdx.x]) q_add64(stat + threadIdx.x, (u64)s_cnt[threadIdx.x]);
}

// Thread t: the N windows ending at bases 32 * (t / TPW) + (t % TPW) * N + j of the encoded stream, as k_query_reads.  t_base: the first
// thread of this launch (a stream of more blocks than one launch takes).  C: n_rows * n_colors cells.  stat[COL_ST_VALID] += the valid
// windows that have a bank, stat[COL_ST_PLACED] += those of them that are rows
template <int W>
__global__ __launch_bounds__(256) void k_color_reads(const u64* __restrict__ packed, const u32* __restrict__ inval, u64 nwords, u64 nbytes, u64 t_base, int k,
                                                     QTable T, ColBanks B, u64 n_rows, u32 n_colors, u32* __restrict__ C, u64* __restrict__ stat) {
    constexpr int N = QBatch<W>::N, TPW = 32 / N;
    const u64 t = t_base + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 wi = t / TPW;
    u32 cnt[COL_ST_COUNT] = {0u, 0u};
    if (wi < nwords) {
        const int t0 = (int)(t % TPW) * N;
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
        // the bank of p0: the least b with p0 < end[b]; the later positions walk on from it (an empty bank is stepped over)
        u32 b = 0;
        while (b < B.n && p0 >= B.end[b]) ++b;
        u64 cur_end = b < B.n ? B.end[b] : 0ull;
        u32 col[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const u64 p = p0 + (u64)j;
            while (b < B.n && p >= cur_end) { ++b; cur_end = b < B.n ? B.end[b] : 0ull; }
            col[j] = b < B.n ? B.first + b : COL_NONE;
            if (col[j] >= n_colors) vm &= ~(1u << j);                                // (no bank; the host side keeps first + n <= n_colors)
        }
        cnt[COL_ST_VALID] = (u32)__popc(vm);
        u32 row[N];
        q_lookup<W, N, true>(T, c, vm, row);
        u32 run = 0, run_row = 0, run_col = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const bool hit = ((vm >> j) & 1u) && (u64)row[j] < n_rows;               // (Q_NO_ROW is above every row number)
            cnt[COL_ST_PLACED] += hit ? 1u : 0u;
#ifdef COL_NO_MERGE
            if (hit) col_add32(C + (u64)row[j] * n_colors + col[j], 1u);
#else
            if (hit && run && row[j] == run_row && col[j] == run_col) { ++run; continue; }
            if (run) col_add32(C + (u64)run_row * n_colors + run_col, run);
            run = hit ? 1u : 0u; run_row = row[j]; run_col = col[j];
#endif
        }
        if (run) col_add32(C + (u64)run_row * n_colors + run_col, run);
    }
    col_block_counts(cnt, stat);
}

// mask[r] (may be null) bit c: C[r][c] >= min_count; counts (may be null) = the copy of C
template <bool VEC>
__global__ __launch_bounds__(256) void k_color_mask(const u32* __restrict__ C, u64 n_rows, u32 n_colors, u32 min_count, u32* __restrict__ counts, u64* __restrict__ mask) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const u64 at = r * n_colors;
    u64 m = 0;
    if constexpr (VEC) {
        for (u32 c = 0; c < n_colors; c += 4) {                                      // (n_colors is a multiple of 4: 16-byte aligned both sides)
            const uint4 v = *reinterpret_cast<const uint4*>(C + at + c);
            if (counts) *reinterpret_cast<uint4*>(counts + at + c) = v;
            m |= (u64)((v.x >= min_count ? 1u : 0u) | (v.y >= min_count ? 2u : 0u) | (v.z >= min_count ? 4u : 0u) | (v.w >= min_count ? 8u : 0u)) << c;
        }
    } else {
        for (u32 c = 0; c < n_colors; ++c) {
            const u32 v = C[at + c];
            if (counts) counts[at + c] = v;
            m |= (u64)(v >= min_count ? 1u : 0u) << c;
        }
    }
    if (mask) mask[r] = m;
}

__global__ __launch_bounds__(256) void k_color_fill64(u64* __restrict__ out, u64 n, u64 value) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = value;
}

// sum[u][c] += C[r][c], any[u] |= mask(r), all[u] &= mask(r) for u = unitig[r]; any of the three may be null.  sum and any start as
// zeros, all as the n_colors low bits
__global__ __launch_bounds__(256) void k_color_unitigs(const u32* __restrict__ C, const u32* __restrict__ unitig, u64 n_rows, u64 n_unitigs, u32 n_colors, u32 min_count,
                                                       u64* __restrict__ sum, u64* __restrict__ all, u64* __restrict__ any) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const u64 u = unitig[r];
    if (u >= n_unitigs) return;                                                      // (a row always has a unitig)
    const u64 at = r * n_colors;
    u64 m = 0;
    for (u32 c = 0; c < n_colors; ++c) {
        const u32 v = C[at + c];
        if (v && sum) q_add64(sum + u * n_colors + c, (u64)v);
        m |= (u64)(v >= min_count ? 1u : 0u) << c;
    }
    if (any && m) (void)__hip_atomic_fetch_or(reinterpret_cast<unsigned long long*>(any + u), (unsigned long long)m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (all) (void)__hip_atomic_fetch_and(reinterpret_cast<unsigned long long*>(all + u), (unsigned long long)m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
