// connections.h -- HIP kernels of the erroneous-connection rule on the compacted de Bruijn graph (gfx950 / MI355X, wave64):
// dskgpu_graph_connections / dskgpu_remove_connections / dskgpu_simplify_all (connections.hip; the definition is in include/dskgpu.h).
// One thread per unitig.
//
// Notation of tips.h: L[u], S[u], the readings U = 2 u + t and their targets E(U).  A candidate is a short chain with edges at both ends,
// none of them on u itself.  The flank of an end A is what u runs into there (V >> 1 for V in E(A)) and what else runs into the same nodes
// (X >> 1 for X in E(V ^ 1)), without u.
//
//   k_conn_candidates  per unitig: cand[u] <=> kind 0, L <= max_nodes, an edge at each end, no target of either end on u, and a mean
//                      abundance of at most max_abundance (S <= max_abundance * L; 0 = no limit).  Writes info[u] = cand and len[u] = L[u],
//                      so that the next kernel gathers len and ab_sum per flank unitig instead of two offsets
//   k_conn_decide      per candidate, one end A after the other: E(A) (<= 4 targets V), then E(V ^ 1) of every V (<= 16 entries X), then
//                      len / S of the <= 20 flank unitigs -- three levels of dependent gathers, each issued as one batch.  weak(A) <=> some
//                      flank unitig w has S[w] L[u] > min_ratio S[u] L[w]: products up to 2^87, compared in 128 bits (ratio128.h).
//                      Writes bits[u] = cand | removed << 1 | weak(2u) << 2 | weak(2u + 1) << 3, removed <=> weak at both ends -- bit 1,
//                      so that k_tip_rows (tips.h) serves for the rows --; counts candidates, one-sided candidates (weak at exactly one end),
//                      removed unitigs and their rows per block in LDS, one atomic per counter and block
//
// No loop on the device depends on the data; every index read from a table is checked against the table it is used on.
#pragma once
#include "layouts.h"
#include "ratio128.h"

#define C_NONE 0xFFFFFFFFu                 // no oriented unitig, no flank unitig

#define C_CAND 1u
#define C_REMOVED 2u
#define C_WEAK0 4u                        // weak at the end 2u
#define C_WEAK1 8u                        // weak at the end 2u + 1
#define C_MAX_NODES 65535u                // the largest max_nodes: S of a candidate stays below 2^48, min_ratio * S below 2^56
#define C_MIN_RATIO 2u                    // from 2 on, two unitigs can never each be the reason the other is removed
#define C_MAX_RATIO 255u

enum CStat { CS_CAND = 0, CS_ONE_SIDED, CS_REMOVED, CS_ROWS, CS_COUNT };

__global__ __launch_bounds__(256) void k_conn_candidates(const u64* __restrict__ offsets, const unsigned char* __restrict__ kind, const u64* __restrict__ ab_sum,
                                                         const u64* __restrict__ e_offsets, const u32* __restrict__ e_targets, u64 n_unitigs, u64 n_edges, int k,
                                                         u32 max_nodes, u32 max_abundance, unsigned char* __restrict__ info, u32* __restrict__ len) {
    const u64 u = (u64)blockIdx.x * 256u + threadIdx.x;
    if (u >= n_unitigs) return;
    const u64 o0 = offsets[u], o1 = offsets[u + 1], S = ab_sum[u];
    const u64 e0 = e_offsets[2 * u], e1 = e_offsets[2 * u + 1], e2 = e_offsets[2 * u + 2];
    const u32 kd = kind[u];
    const u64 L = o1 - o0 - (u64)k;
    const bool shape = kd == 0u && L <= (u64)max_nodes && e1 > e0 && e2 > e1 && (max_abundance == 0u || S <= (u64)max_abundance * L);
    const u32 d0 = (u32)min(e1 - e0, 4ull), d1 = (u32)min(e2 - e1, 4ull);
    u32 T[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        T[i] = (shape && (u32)i < d0 && e0 + i < n_edges) ? e_targets[e0 + i] : C_NONE;
        T[4 + i] = (shape && (u32)i < d1 && e1 + i < n_edges) ? e_targets[e1 + i] : C_NONE;
    }
    bool on_itself = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) on_itself = on_itself || (T[i] != C_NONE && (u64)(T[i] >> 1) == u);
    info[u] = (unsigned char)((shape && !on_itself) ? C_CAND : 0u);
    len[u] = (u32)min(L, 0xFFFFFFFFull);
}

// weak(A) of candidate u, whose end A has the targets e_targets[a0 .. a1): rSu = min_ratio * S[u]
__device__ __forceinline__ bool conn_weak_at(u64 a0, u64 a1, u64 u, u64 Lu, u64 rSu, const u32* __restrict__ len, const u64* __restrict__ ab_sum,
                                             const u64* __restrict__ e_offsets, const u32* __restrict__ e_targets, u64 n_unitigs, u64 n_edges) {
    const u64 n_or = 2 * n_unitigs;
    const u32 dA = (u32)min(a1 - a0, 4ull);
    u32 V[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) V[i] = ((u32)i < dA && a0 + i < n_edges) ? e_targets[a0 + i] : C_NONE;
    u64 b0[4], b1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const u64 X = (u64)(V[i] ^ 1u);
        const bool in = V[i] != C_NONE && X < n_or;
        b0[i] = in ? e_offsets[X] : 0ull; b1[i] = in ? e_offsets[X + 1] : 0ull;
    }
    u32 w[20];                                                                // what u runs into, then what else runs into the same nodes
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        w[i] = (V[i] != C_NONE && (u64)(V[i] >> 1) < n_unitigs && (u64)(V[i] >> 1) != u) ? V[i] >> 1 : C_NONE;
        const u32 d = (u32)min(b1[i] - b0[i], 4ull);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const u32 X = ((u32)j < d && b0[i] + j < n_edges) ? e_targets[b0[i] + j] : C_NONE;
            w[4 + 4 * i + j] = (X != C_NONE && (u64)(X >> 1) < n_unitigs && (u64)(X >> 1) != u) ? X >> 1 : C_NONE;
        }
    }
    u32 wl[20]; u64 ws[20];
#pragma unroll
    for (int j = 0; j < 20; ++j) {
        const bool in = w[j] != C_NONE;
        wl[j] = in ? len[w[j]] : 0u; ws[j] = in ? ab_sum[w[j]] : 0ull;
    }
    bool weak = false;
#pragma unroll
    for (int j = 0; j < 20; ++j) weak = weak || (w[j] != C_NONE && ratio128_greater(ws[j], Lu, rSu, (u64)wl[j]));
    return weak;
}

__global__ __launch_bounds__(256) void k_conn_decide(const unsigned char* __restrict__ info, const u32* __restrict__ len, const u64* __restrict__ ab_sum,
                                                     const u64* __restrict__ e_offsets, const u32* __restrict__ e_targets, u64 n_unitigs, u64 n_edges, u32 min_ratio,
                                                     unsigned char* __restrict__ bits, u64* __restrict__ stat) {
    __shared__ u32 s_stat[CS_COUNT];
    if (threadIdx.x < CS_COUNT) s_stat[threadIdx.x] = 0u;
    __syncthreads();
    const u64 u = (u64)blockIdx.x * 256u + threadIdx.x;
    const u32 mine = u < n_unitigs ? (u32)info[u] : 0u;
    if (mine & C_CAND) {
        const u64 Su = ab_sum[u], Lu = (u64)len[u];
        const u64 e0 = e_offsets[2 * u], e1 = e_offsets[2 * u + 1], e2 = e_offsets[2 * u + 2];
        const u64 rSu = (u64)min_ratio * Su;                                  // (a candidate: S < 2^16 * 2^32, min_ratio < 2^8)
        const bool weak0 = conn_weak_at(e0, e1, u, Lu, rSu, len, ab_sum, e_offsets, e_targets, n_unitigs, n_edges);
        const bool weak1 = conn_weak_at(e1, e2, u, Lu, rSu, len, ab_sum, e_offsets, e_targets, n_unitigs, n_edges);
        const bool removed = weak0 && weak1;
        bits[u] = (unsigned char)(C_CAND | (removed ? C_REMOVED : 0u) | (weak0 ? C_WEAK0 : 0u) | (weak1 ? C_WEAK1 : 0u));
        atomicAdd(&s_stat[CS_CAND], 1u);
        if (weak0 != weak1) atomicAdd(&s_stat[CS_ONE_SIDED], 1u);
        if (removed) { atomicAdd(&s_stat[CS_REMOVED], 1u); atomicAdd(&s_stat[CS_ROWS], (u32)Lu); }      // (256 candidates of <= 65535 rows: 32 bits hold a block's sum)
    } else if (u < n_unitigs) {
        bits[u] = 0;
    }
    __syncthreads();
    if (threadIdx.x < CS_COUNT && s_stat[threadIdx.x]) atomicAdd(reinterpret_cast<unsigned long long*>(&stat[threadIdx.x]), (unsigned long long)s_stat[threadIdx.x]);
}
