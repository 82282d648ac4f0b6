// bubbles.h -- HIP kernels of the bubble rule on the compacted de Bruijn graph (gfx950 / MI355X, wave64): dskgpu_graph_bubbles /
// dskgpu_pop_bubbles / dskgpu_simplify (rules.hip; the definition is in include/dskgpu.h).  One thread per unitig.
//
// Notation, gathers and counters of rules.h: L[u], S[u], the readings U = 2 u + t and their targets E(U).  A candidate is a chain with
// exactly one edge at each end, out(u) = E(2u)[0] and in(u) = E(2u + 1)[0], neither on u itself: a simple path from P = in(u) ^ 1 to out(u).
//
//   k_bubble_candidates  per unitig: cand[u] <=> kind 0, L <= max_nodes, one edge at each end, no end on u.  Writes ends[u] = in(u) << 32 |
//                        out(u), or R_NO_ENDS when u is no candidate, and len[u] = L[u], so that the next kernel gathers one word plus len
//                        and ab_sum per sibling instead of three offsets and two targets
//   k_bubble_decide      per candidate: E(P) (<= 4 targets X), then ends / len / S of every w = X >> 1, w != u (r_siblings) -- three levels
//                        of dependent gathers, each issued as one batch.  w is a sibling <=> cand[w], it has the ends of u read in the
//                        orientation in which P reaches it (r_same_ends) and |L[w] - L[u]| <= max_diff.  pop[u] <=> some sibling is
//                        stronger: S[w] L[u] > S[u] L[w], or equal and L[w] > L[u] (products of two candidates: < 2^48 * 2^16).  Writes
//                        bits[u] = cand | pop << 1 | in_bubble << 2; counts candidates, unitigs in bubbles, popped unitigs and their rows
//
// No loop on the device depends on the data; every index read from a table is checked against the table it is used on.
#pragma once
#include "rules.h"

#define B_IN_BUBBLE 4u

enum BStat { BS_CAND = 0, BS_IN_BUBBLES, BS_POPPED, BS_ROWS, BS_COUNT };
static_assert(BS_COUNT == R_COUNTERS && BS_ROWS == R_ROWS, "the bubble rule's counters are a rule's");

__global__ __launch_bounds__(256) void k_bubble_candidates(const u64* __restrict__ offsets, const unsigned char* __restrict__ kind, const u64* __restrict__ e_offsets,
                                                           const u32* __restrict__ e_targets, u64 n_unitigs, u64 n_edges, int k, u32 max_nodes,
                                                           u64* __restrict__ ends, u32* __restrict__ len) {
    const u64 u = (u64)blockIdx.x * 256u + threadIdx.x;
    if (u >= n_unitigs) return;
    const RShape s = r_shape<false>(offsets, kind, nullptr, e_offsets, u, k);
    const bool path = s.kind == 0u && s.L <= (u64)max_nodes && s.e1 - s.e0 == 1ull && s.e2 - s.e1 == 1ull && s.e1 < n_edges;      // (e0 < e1)
    const u32 out = path ? e_targets[s.e0] : R_NONE, in = path ? e_targets[s.e1] : R_NONE;
    const u64 n_or = 2 * n_unitigs;
    const bool cand = path && (u64)out < n_or && (u64)in < n_or && (u64)(out >> 1) != u && (u64)(in >> 1) != u;
    ends[u] = cand ? (u64)in << 32 | (u64)out : R_NO_ENDS;
    len[u] = r_len(s.L);
}

__global__ __launch_bounds__(256) void k_bubble_decide(const u64* __restrict__ ends, const u32* __restrict__ len, const u64* __restrict__ ab_sum,
                                                       const u64* __restrict__ e_offsets, const u32* __restrict__ e_targets, u64 n_unitigs, u64 n_edges, u32 max_diff,
                                                       unsigned char* __restrict__ bits, u64* __restrict__ stat) {
    __shared__ u32 s_stat[R_COUNTERS];
    r_counters_zero(s_stat);
    const u64 u = (u64)blockIdx.x * 256u + threadIdx.x;
    const u64 mine = u < n_unitigs ? ends[u] : R_NO_ENDS;
    if (mine != R_NO_ENDS) {
        const u32 in = (u32)(mine >> 32), out = (u32)mine;
        const u64 P = (u64)(in ^ 1u);                                         // (in < 2 n_unitigs, k_bubble_candidates checked it: so is its flip)
        const u64 Su = ab_sum[u], Lu = (u64)len[u];
        const u64 p0 = e_offsets[P], p1 = e_offsets[P + 1];
        u32 X[4]; RSibling s[4];
        r_siblings<true>(p0, p1, u, ends, len, ab_sum, e_targets, n_unitigs, n_edges, X, s);
        bool in_bubble = false, pop = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (s[i].ends == R_NO_ENDS) continue;
            const bool same_ends = r_same_ends(X[i], s[i].ends, in, out);
            const u64 Lw = (u64)s[i].len, diff = Lw > Lu ? Lw - Lu : Lu - Lw;
            if (!same_ends || diff > (u64)max_diff) continue;
            in_bubble = true;
            const u64 l = s[i].S * Lu, r = Su * Lw;
            pop = pop || l > r || (l == r && Lw > Lu);
        }
        bits[u] = (unsigned char)(R_CAND | (pop ? R_TAKEN : 0u) | (in_bubble ? B_IN_BUBBLE : 0u));
        atomicAdd(&s_stat[BS_CAND], 1u);
        if (in_bubble) atomicAdd(&s_stat[BS_IN_BUBBLES], 1u);
        if (pop) { atomicAdd(&s_stat[BS_POPPED], 1u); atomicAdd(&s_stat[BS_ROWS], (u32)Lu); }
    } else if (u < n_unitigs) {
        bits[u] = 0;
    }
    __syncthreads();
    r_counters_add(s_stat, stat);
}
