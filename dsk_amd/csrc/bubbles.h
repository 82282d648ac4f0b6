// bubbles.h -- HIP kernels of the bubble rule on the compacted de Bruijn graph (gfx950 / MI355X, wave64): dskgpu_graph_bubbles /
// dskgpu_pop_bubbles / dskgpu_simplify (bubbles.hip; the definition is in include/dskgpu.h).  One thread per unitig.
//
// Notation of tips.h: L[u], S[u], the readings U = 2 u + t and their targets E(U).  A candidate is a chain with exactly one edge at each
// end, out(u) = E(2u)[0] and in(u) = E(2u + 1)[0], neither on u itself: a simple path from P = in(u) ^ 1 to out(u).
//
//   k_bubble_candidates  per unitig: cand[u] <=> kind 0, L <= max_nodes, one edge at each end, no end on u.  Writes ends[u] = in(u) << 32 |
//                        out(u), or B_NO_ENDS when u is no candidate, and len[u] = L[u], so that the next kernel gathers one word plus len
//                        and ab_sum per sibling instead of three offsets and two targets
//   k_bubble_decide      per candidate: E(P) (<= 4 targets X), then ends / len / S of every w = X >> 1, w != u -- three levels of dependent
//                        gathers, each issued as one batch.  w is a sibling <=> cand[w], it has the ends of u read in the orientation in
//                        which P reaches it (X even: out(w) == out(u) and in(w) == in(u); X odd: in(w) == out(u) and out(w) == in(u)) and
//                        |L[w] - L[u]| <= max_diff.  pop[u] <=> some sibling is stronger: S[w] L[u] > S[u] L[w], or equal and L[w] > L[u]
//                        (products of two candidates: < 2^48 * 2^16).  Writes bits[u] = cand | pop << 1 | in_bubble << 2 -- bit 1, so that
//                        k_tip_rows (tips.h) serves for the rows --; counts candidates, unitigs in bubbles, popped unitigs and their rows per
//                        block in LDS, one atomic per counter and block
//
// No loop on the device depends on the data; every index read from a table is checked against the table it is used on.
#pragma once
#include "layouts.h"

#define B_NONE 0xFFFFFFFFu                 // no oriented unitig
#define B_NO_ENDS 0xFFFFFFFFFFFFFFFFull    // ends[u] of a unitig that is no candidate (both halves B_NONE: no oriented unitig has that number)

#define B_CAND 1u
#define B_POP 2u
#define B_IN_BUBBLE 4u
#define B_MAX_NODES 65535u                // the largest max_nodes: S * L of two candidates stays below 2^64

enum BStat { BS_CAND = 0, BS_IN_BUBBLES, BS_POPPED, BS_ROWS, BS_COUNT };

__global__ __launch_bounds__(256) void k_bubble_candidates(const u64* __restrict__ offsets, const unsigned char* __restrict__ kind, const u64* __restrict__ e_offsets,
                                                           const u32* __restrict__ e_targets, u64 n_unitigs, u64 n_edges, int k, u32 max_nodes,
                                                           u64* __restrict__ ends, u32* __restrict__ len) {
    const u64 u = (u64)blockIdx.x * 256u + threadIdx.x;
    if (u >= n_unitigs) return;
    const u64 o0 = offsets[u], o1 = offsets[u + 1];
    const u64 e0 = e_offsets[2 * u], e1 = e_offsets[2 * u + 1], e2 = e_offsets[2 * u + 2];
    const u32 kd = kind[u];
    const u64 L = o1 - o0 - (u64)k;
    const bool path = kd == 0u && L <= (u64)max_nodes && e1 - e0 == 1ull && e2 - e1 == 1ull && e1 < n_edges;      // (e0 < e1)
    const u32 out = path ? e_targets[e0] : B_NONE, in = path ? e_targets[e1] : B_NONE;
    const u64 n_or = 2 * n_unitigs;
    const bool cand = path && (u64)out < n_or && (u64)in < n_or && (u64)(out >> 1) != u && (u64)(in >> 1) != u;
    ends[u] = cand ? (u64)in << 32 | (u64)out : B_NO_ENDS;
    len[u] = (u32)min(L, 0xFFFFFFFFull);
}

__global__ __launch_bounds__(256) void k_bubble_decide(const u64* __restrict__ ends, const u32* __restrict__ len, const u64* __restrict__ ab_sum,
                                                       const u64* __restrict__ e_offsets, const u32* __restrict__ e_targets, u64 n_unitigs, u64 n_edges, u32 max_diff,
                                                       unsigned char* __restrict__ bits, u64* __restrict__ stat) {
    __shared__ u32 s_stat[BS_COUNT];
    if (threadIdx.x < BS_COUNT) s_stat[threadIdx.x] = 0u;
    __syncthreads();
    const u64 u = (u64)blockIdx.x * 256u + threadIdx.x;
    const u64 mine = u < n_unitigs ? ends[u] : B_NO_ENDS;
    if (mine != B_NO_ENDS) {
        const u32 in = (u32)(mine >> 32), out = (u32)mine;
        const u64 P = (u64)(in ^ 1u);                                         // (in < 2 n_unitigs, k_bubble_candidates checked it: so is its flip)
        const u64 Su = ab_sum[u], Lu = (u64)len[u];
        const u64 p0 = e_offsets[P], p1 = e_offsets[P + 1];
        const u32 dP = (u32)min(p1 - p0, 4ull);
        u32 X[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) X[i] = ((u32)i < dP && p0 + i < n_edges) ? e_targets[p0 + i] : B_NONE;
        u64 we[4], ws[4]; u32 wl[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const u64 w = (u64)(X[i] >> 1);
            const bool in_table = X[i] != B_NONE && w < n_unitigs && w != u;
            we[i] = in_table ? ends[w] : B_NO_ENDS; wl[i] = in_table ? len[w] : 0u; ws[i] = in_table ? ab_sum[w] : 0ull;
        }
        bool in_bubble = false, pop = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (we[i] == B_NO_ENDS) continue;                                 // (no target, u itself, or no candidate)
            const u32 wi = (u32)(we[i] >> 32), wo = (u32)we[i];
            const bool same_ends = (X[i] & 1u) ? (wi == out && wo == in) : (wo == out && wi == in);
            const u64 Lw = (u64)wl[i], diff = Lw > Lu ? Lw - Lu : Lu - Lw;
            if (!same_ends || diff > (u64)max_diff) continue;
            in_bubble = true;
            const u64 l = ws[i] * Lu, r = Su * Lw;
            pop = pop || l > r || (l == r && Lw > Lu);
        }
        bits[u] = (unsigned char)(B_CAND | (pop ? B_POP : 0u) | (in_bubble ? B_IN_BUBBLE : 0u));
        atomicAdd(&s_stat[BS_CAND], 1u);
        if (in_bubble) atomicAdd(&s_stat[BS_IN_BUBBLES], 1u);
        if (pop) { atomicAdd(&s_stat[BS_POPPED], 1u); atomicAdd(&s_stat[BS_ROWS], (u32)Lu); }      // (256 candidates of <= 65535 rows: 32 bits hold a block's sum)
    } else if (u < n_unitigs) {
        bits[u] = 0;
    }
    __syncthreads();
    if (threadIdx.x < BS_COUNT && s_stat[threadIdx.x]) atomicAdd(reinterpret_cast<unsigned long long*>(&stat[threadIdx.x]), (unsigned long long)s_stat[threadIdx.x]);
}
