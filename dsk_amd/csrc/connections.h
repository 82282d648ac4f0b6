// connections.h -- HIP kernels of the erroneous-connection rule on the compacted de Bruijn graph (gfx950 / MI355X, wave64):
// dskgpu_graph_connections / dskgpu_remove_connections / dskgpu_simplify_all (rules.hip; the definition is in include/dskgpu.h).
// One thread per unitig.
//
// Notation, gathers and counters of rules.h: L[u], S[u], the readings U = 2 u + t and their targets E(U).  A candidate is a short chain
// with edges at both ends, none of them on u itself.  The flank of an end A is what u runs into there (V >> 1 for V in E(A)) and what else
// runs into the same nodes (X >> 1 for X in E(V ^ 1)), without u.
//
//   k_conn_candidates  per unitig: cand[u] <=> kind 0, L <= max_nodes, an edge at each end, no target of either end on u, and a mean
//                      abundance of at most max_abundance (S <= max_abundance * L; 0 = no limit).  Writes info[u] = cand and len[u] = L[u],
//                      so that the next kernel gathers len and ab_sum per flank unitig instead of two offsets
//   k_conn_decide      per candidate, one end A after the other: its flank (r_flank: <= 4 targets V, <= 16 entries X), then len / S of the
//                      <= 20 flank unitigs -- three levels of dependent gathers, each issued as one batch.  weak(A) <=> some flank unitig w
//                      has S[w] L[u] > min_ratio S[u] L[w]: products up to 2^87, compared in 128 bits (ratio128.h).  Writes bits[u] =
//                      cand | removed << 1 | weak(2u) << 2 | weak(2u + 1) << 3, removed <=> weak at both ends; counts candidates, one-sided
//                      candidates (weak at exactly one end), removed unitigs and their rows
//
// No loop on the device depends on the data; every index read from a table is checked against the table it is used on.
#pragma once
#include "rules.h"
#include "ratio128.h"

#define C_WEAK0 4u                        // weak at the end 2u
#define C_WEAK1 8u                        // weak at the end 2u + 1
#define C_MIN_RATIO 2u                    // from 2 on, two unitigs can never each be the reason the other is removed
#define C_MAX_RATIO 255u                  // (with R_MAX_NODES: min_ratio * S of a candidate stays below 2^56)

enum ConnStat { CN_CAND = 0, CN_ONE_SIDED, CN_REMOVED, CN_ROWS, CN_COUNT };
static_assert(CN_COUNT == R_COUNTERS && CN_ROWS == R_ROWS, "the connection rule's counters are a rule's");

__global__ __launch_bounds__(256) void k_conn_candidates(const u64* __restrict__ offsets, const unsigned char* __restrict__ kind, const u64* __restrict__ ab_sum,
                                                         const u64* __restrict__ e_offsets, const u32* __restrict__ e_targets, u64 n_unitigs, u64 n_edges, int k,
                                                         u32 max_nodes, u32 max_abundance, unsigned char* __restrict__ info, u32* __restrict__ len) {
    const u64 u = (u64)blockIdx.x * 256u + threadIdx.x;
    if (u >= n_unitigs) return;
    const RShape s = r_shape<true>(offsets, kind, ab_sum, e_offsets, u, k);
    const bool shape = s.kind == 0u && s.L <= (u64)max_nodes && s.e1 > s.e0 && s.e2 > s.e1 && (max_abundance == 0u || s.S <= (u64)max_abundance * s.L);
    const u32 d0 = r_degree(s.e0, s.e1), d1 = r_degree(s.e1, s.e2);
    u32 T[8];                                                                 // the targets of both ends, as one batch; none when the shape is wrong
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        T[i] = r_target(shape, s.e0, d0, i, e_targets, n_edges);
        T[4 + i] = r_target(shape, s.e1, d1, i, e_targets, n_edges);
    }
    bool on_itself = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) on_itself = on_itself || (T[i] != R_NONE && (u64)(T[i] >> 1) == u);
    info[u] = (unsigned char)((shape && !on_itself) ? R_CAND : 0u);
    len[u] = r_len(s.L);
}

// weak(A) of candidate u, whose end A has the targets e_targets[a0 .. a1): rSu = min_ratio * S[u]
__device__ __forceinline__ bool conn_weak_at(u64 a0, u64 a1, u64 u, u64 Lu, u64 rSu, const u32* __restrict__ len, const u64* __restrict__ ab_sum,
                                             const u64* __restrict__ e_offsets, const u32* __restrict__ e_targets, u64 n_unitigs, u64 n_edges) {
    u32 V[4], X[16];
    r_flank(a0, a1, e_offsets, e_targets, n_unitigs, n_edges, V, X);
    u32 w[20];                                                                // what u runs into, then what else runs into the same nodes
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = r_other(V[i], u, n_unitigs);
#pragma unroll
    for (int j = 0; j < 16; ++j) w[4 + j] = r_other(X[j], u, n_unitigs);
    u32 wl[20]; u64 ws[20];
#pragma unroll
    for (int j = 0; j < 20; ++j) {
        const bool in = w[j] != R_NONE;
        wl[j] = in ? len[w[j]] : 0u; ws[j] = in ? ab_sum[w[j]] : 0ull;
    }
    bool weak = false;
#pragma unroll
    for (int j = 0; j < 20; ++j) weak = weak || (w[j] != R_NONE && ratio128_greater(ws[j], Lu, rSu, (u64)wl[j]));
    return weak;
}

__global__ __launch_bounds__(256) void k_conn_decide(const unsigned char* __restrict__ info, const u32* __restrict__ len, const u64* __restrict__ ab_sum,
                                                     const u64* __restrict__ e_offsets, const u32* __restrict__ e_targets, u64 n_unitigs, u64 n_edges, u32 min_ratio,
                                                     unsigned char* __restrict__ bits, u64* __restrict__ stat) {
    __shared__ u32 s_stat[R_COUNTERS];
    r_counters_zero(s_stat);
    const u64 u = (u64)blockIdx.x * 256u + threadIdx.x;
    const u32 mine = u < n_unitigs ? (u32)info[u] : 0u;
    if (mine & R_CAND) {
        const u64 Su = ab_sum[u], Lu = (u64)len[u];
        const u64 e0 = e_offsets[2 * u], e1 = e_offsets[2 * u + 1], e2 = e_offsets[2 * u + 2];
        const u64 rSu = (u64)min_ratio * Su;                                  // (a candidate: S < 2^16 * 2^32, min_ratio < 2^8)
        const bool weak0 = conn_weak_at(e0, e1, u, Lu, rSu, len, ab_sum, e_offsets, e_targets, n_unitigs, n_edges);
        const bool weak1 = conn_weak_at(e1, e2, u, Lu, rSu, len, ab_sum, e_offsets, e_targets, n_unitigs, n_edges);
        const bool removed = weak0 && weak1;
        bits[u] = (unsigned char)(R_CAND | (removed ? R_TAKEN : 0u) | (weak0 ? C_WEAK0 : 0u) | (weak1 ? C_WEAK1 : 0u));
        atomicAdd(&s_stat[CN_CAND], 1u);
        if (weak0 != weak1) atomicAdd(&s_stat[CN_ONE_SIDED], 1u);
        if (removed) { atomicAdd(&s_stat[CN_REMOVED], 1u); atomicAdd(&s_stat[CN_ROWS], (u32)Lu); }
    } else if (u < n_unitigs) {
        bits[u] = 0;
    }
    __syncthreads();
    r_counters_add(s_stat, stat);
}
