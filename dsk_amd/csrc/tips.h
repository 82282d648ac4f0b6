// tips.h -- HIP kernels of the tip rule on the compacted de Bruijn graph and of the row filter that takes the tips' rows out of a result
// (gfx950 / MI355X, wave64): dskgpu_graph_tips / dskgpu_clip_tips / dskgpu_filter_rows (tips.hip; the definition is in include/dskgpu.h).
//
// Unitig u has L[u] = offsets[u + 1] - offsets[u] - k rows and the abundance sum S[u]; its oriented readings are U = 2 u + t with the
// targets E(U) = e_targets[e_offsets[U] .. e_offsets[U + 1]) (unitigs.h).  Everything is exact integer arithmetic on these tables.
//
//   k_tip_candidates   per unitig: cand[u] <=> a chain of at most max_nodes rows with exactly one dead end whose mean abundance is at most
//                      max_abundance (S <= max_abundance * L; 0 = no limit).  Writes info[u] = cand | attached end t << 1 and len[u] = L[u],
//                      so that the next kernel gathers one byte and one word per sibling instead of two offsets
//   k_tip_decide       per candidate: E(A), A = 2 u + t the attached end (<= 4 targets V), then E(V ^ 1) of every V (<= 16 entries X), then
//                      info / S / len of the siblings w = X >> 1, w != u -- three levels of dependent gathers, each issued as one batch.
//                      tip[u] <=> some sibling is no candidate or is stronger: S[w] L[u] > S[u] L[w], or equal and L[w] > L[u] (products of
//                      two candidates: < 2^48 * 2^16).  Writes bits[u] = cand | tip << 1 | outranked << 2; counts candidates, tips,
//                      outranked tips and the rows of the tips per block in LDS, one atomic per counter and block
//   k_tip_rows         per row: the tip bit of its unitig -> row_tip[r] and / or keep[r] = !tip
//   k_rows_compact<W>  per row with keep[r] != 0: all W words and the abundance to position scan[r] (the exclusive scan of the keep flags)
//   k_filter_offsets   the scan read at the old partition offsets = the new ones; an old offset of n_rows reads as the kept total
//
// No loop on the device depends on the data; every index read from a table is checked against the table it is used on.
#pragma once
#include "layouts.h"

#define T_NONE 0xFFFFFFFFu                 // no oriented unitig, no sibling (U_NONE of unitigs.h, whose kernels only unitigs.hip may define)

#define T_CAND 1u
#define T_TIP 2u
#define T_OUTRANKED 4u
#define T_MAX_NODES 65535u                // the largest max_nodes: S * L of two candidates stays below 2^64

enum TStat { TS_CAND = 0, TS_TIPS, TS_OUTRANKED, TS_ROWS, TS_COUNT };

__global__ __launch_bounds__(256) void k_tip_candidates(const u64* __restrict__ offsets, const unsigned char* __restrict__ kind, const u64* __restrict__ ab_sum,
                                                        const u64* __restrict__ e_offsets, u64 n_unitigs, int k, u32 max_nodes, u32 max_abundance,
                                                        unsigned char* __restrict__ info, u32* __restrict__ len) {
    const u64 u = (u64)blockIdx.x * 256u + threadIdx.x;
    if (u >= n_unitigs) return;
    const u64 o0 = offsets[u], o1 = offsets[u + 1], S = ab_sum[u];
    const u64 e0 = e_offsets[2 * u], e1 = e_offsets[2 * u + 1], e2 = e_offsets[2 * u + 2];
    const u32 kd = kind[u];
    const u64 L = o1 - o0 - (u64)k;
    const bool dead0 = e1 == e0, dead1 = e2 == e1;
    const bool cand = kd == 0u && L <= (u64)max_nodes && dead0 != dead1 && (max_abundance == 0u || S <= (u64)max_abundance * L);
    info[u] = (unsigned char)((cand ? T_CAND : 0u) | (dead0 ? 2u : 0u));      // (dead0: reading 2u has no edges, the attached end is 2u + 1)
    len[u] = (u32)min(L, 0xFFFFFFFFull);
}

__global__ __launch_bounds__(256) void k_tip_decide(const unsigned char* __restrict__ info, const u32* __restrict__ len, const u64* __restrict__ ab_sum,
                                                    const u64* __restrict__ e_offsets, const u32* __restrict__ e_targets, u64 n_unitigs, u64 n_edges,
                                                    unsigned char* __restrict__ bits, u64* __restrict__ stat) {
    __shared__ u32 s_stat[TS_COUNT];
    if (threadIdx.x < TS_COUNT) s_stat[threadIdx.x] = 0u;
    __syncthreads();
    const u64 n_or = 2 * n_unitigs;
    const u64 u = (u64)blockIdx.x * 256u + threadIdx.x;
    const u32 mine = u < n_unitigs ? (u32)info[u] : 0u;
    if (mine & T_CAND) {
        const u64 A = 2 * u + ((mine >> 1) & 1u);
        const u64 Su = ab_sum[u], Lu = (u64)len[u];
        const u64 a0 = e_offsets[A], a1 = e_offsets[A + 1];
        const u32 dA = (u32)min(a1 - a0, 4ull);
        u32 V[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) V[i] = ((u32)i < dA && a0 + i < n_edges) ? e_targets[a0 + i] : T_NONE;
        u64 b0[4], b1[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const u64 X = (u64)(V[i] ^ 1u);
            const bool in = V[i] != T_NONE && X < n_or;
            b0[i] = in ? e_offsets[X] : 0ull; b1[i] = in ? e_offsets[X + 1] : 0ull;
        }
        u32 w[16];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const u32 d = (u32)min(b1[i] - b0[i], 4ull);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const u32 X = ((u32)j < d && b0[i] + j < n_edges) ? e_targets[b0[i] + j] : T_NONE;
                w[4 * i + j] = (X != T_NONE && (u64)(X >> 1) < n_unitigs && (u64)(X >> 1) != u) ? X >> 1 : T_NONE;
            }
        }
        u32 wi[16], wl[16]; u64 ws[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const bool in = w[j] != T_NONE;
            wi[j] = in ? (u32)info[w[j]] : 0u; wl[j] = in ? len[w[j]] : 0u; ws[j] = in ? ab_sum[w[j]] : 0ull;
        }
        bool solid = false, stronger = false;                                 // a sibling that is no candidate / a candidate that is stronger
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (w[j] == T_NONE) continue;
            if (!(wi[j] & T_CAND)) { solid = true; continue; }
            const u64 l = ws[j] * Lu, r = Su * (u64)wl[j];
            stronger = stronger || l > r || (l == r && (u64)wl[j] > Lu);
        }
        const bool tip = solid || stronger, outranked = tip && !solid;
        bits[u] = (unsigned char)(T_CAND | (tip ? T_TIP : 0u) | (outranked ? T_OUTRANKED : 0u));
        atomicAdd(&s_stat[TS_CAND], 1u);
        if (tip) { atomicAdd(&s_stat[TS_TIPS], 1u); atomicAdd(&s_stat[TS_ROWS], (u32)Lu); }      // (256 candidates of <= 65535 rows: 32 bits hold a block's sum)
        if (outranked) atomicAdd(&s_stat[TS_OUTRANKED], 1u);
    } else if (u < n_unitigs) {
        bits[u] = 0;
    }
    __syncthreads();
    if (threadIdx.x < TS_COUNT && s_stat[threadIdx.x]) atomicAdd(reinterpret_cast<unsigned long long*>(&stat[threadIdx.x]), (unsigned long long)s_stat[threadIdx.x]);
}

// either output may be null
__global__ __launch_bounds__(256) void k_tip_rows(const u32* __restrict__ unitig, const unsigned char* __restrict__ bits, u64 n, u64 n_unitigs,
                                                  unsigned char* __restrict__ row_tip, unsigned char* __restrict__ keep) {
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const u32 u = unitig[r];
    const u32 tip = (u64)u < n_unitigs ? ((u32)bits[u] >> 1) & 1u : 0u;      // (cannot be: k_unitig_number numbered every row; no index leaves an array)
    if (row_tip) row_tip[r] = (unsigned char)tip;
    if (keep) keep[r] = (unsigned char)(tip ^ 1u);
}

// the keep flag as the scan's input: non-zero = 1
struct TKeepFlag { __host__ __device__ u64 operator()(unsigned char c) const { return c ? 1ull : 0ull; } };

template <int W>
__global__ __launch_bounds__(256) void k_rows_compact(RowsIn rows, const u32* __restrict__ ab, const unsigned char* __restrict__ keep, const u64* __restrict__ scan,
                                                      u64 n, u64 n_kept, RowsOut out, u32* __restrict__ out_ab) {
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r >= n || keep[r] == 0) return;
    u64 x[W];
#pragma unroll
    for (int q = 0; q < W; ++q) x[q] = rows.w[q][r];
    const u32 a = ab[r];
    const u64 d = scan[r];
    if (d >= n_kept) return;                                                  // (cannot be: n_kept is the scan's total; the same guard)
#pragma unroll
    for (int q = 0; q < W; ++q) out.w[q][d] = x[q];
    out_ab[d] = a;
}

// new_off[i] = kept rows before old row old_off[i]; old_off[i] >= n: all the kept rows
__global__ __launch_bounds__(256) void k_filter_offsets(const u64* __restrict__ old_off, u64 n_off, const u64* __restrict__ scan, const unsigned char* __restrict__ keep,
                                                        u64 n, u64* __restrict__ new_off) {
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_off) return;
    const u64 o = old_off[i];
    new_off[i] = o < n ? scan[o] : scan[n - 1] + (keep[n - 1] ? 1ull : 0ull);      // (launched with n > 0 only)
}
