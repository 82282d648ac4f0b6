// tips.h -- HIP kernels of the tip rule on the compacted de Bruijn graph (gfx950 / MI355X, wave64): dskgpu_graph_tips / dskgpu_clip_tips
// (rules.hip; the definition is in include/dskgpu.h).  One thread per unitig.
//
// Notation, gathers and counters of rules.h: L[u], S[u], the readings U = 2 u + t and their targets E(U).
//
//   k_tip_candidates   per unitig: cand[u] <=> a chain of at most max_nodes rows with exactly one dead end whose mean abundance is at most
//                      max_abundance (S <= max_abundance * L; 0 = no limit).  Writes info[u] = cand | attached end t << 1 and len[u] = L[u],
//                      so that the next kernel gathers one byte and one word per sibling instead of two offsets
//   k_tip_decide       per candidate: the flank of A = 2 u + t, the attached end (r_flank: <= 4 targets V, <= 16 entries X of the E(V ^ 1)),
//                      then info / S / len of the siblings w = X >> 1, w != u -- three levels of dependent gathers, each issued as one batch.
//                      tip[u] <=> some sibling is no candidate or is stronger: S[w] L[u] > S[u] L[w], or equal and L[w] > L[u] (products of
//                      two candidates: < 2^48 * 2^16).  Writes bits[u] = cand | tip << 1 | outranked << 2; counts candidates, tips,
//                      outranked tips and the rows of the tips
//
// No loop on the device depends on the data; every index read from a table is checked against the table it is used on.
#pragma once
#include "rules.h"

#define T_OUTRANKED 4u

enum TipStat { TP_CAND = 0, TP_TIPS, TP_OUTRANKED, TP_ROWS, TP_COUNT };
static_assert(TP_COUNT == R_COUNTERS && TP_ROWS == R_ROWS, "the tip rule's counters are a rule's");

__global__ __launch_bounds__(256) void k_tip_candidates(const u64* __restrict__ offsets, const unsigned char* __restrict__ kind, const u64* __restrict__ ab_sum,
                                                        const u64* __restrict__ e_offsets, u64 n_unitigs, int k, u32 max_nodes, u32 max_abundance,
                                                        unsigned char* __restrict__ info, u32* __restrict__ len) {
    const u64 u = (u64)blockIdx.x * 256u + threadIdx.x;
    if (u >= n_unitigs) return;
    const RShape s = r_shape<true>(offsets, kind, ab_sum, e_offsets, u, k);
    const bool dead0 = s.e1 == s.e0, dead1 = s.e2 == s.e1;
    const bool cand = s.kind == 0u && s.L <= (u64)max_nodes && dead0 != dead1 && (max_abundance == 0u || s.S <= (u64)max_abundance * s.L);
    info[u] = (unsigned char)((cand ? R_CAND : 0u) | (dead0 ? 2u : 0u));      // (dead0: reading 2u has no edges, the attached end is 2u + 1)
    len[u] = r_len(s.L);
}

__global__ __launch_bounds__(256) void k_tip_decide(const unsigned char* __restrict__ info, const u32* __restrict__ len, const u64* __restrict__ ab_sum,
                                                    const u64* __restrict__ e_offsets, const u32* __restrict__ e_targets, u64 n_unitigs, u64 n_edges,
                                                    unsigned char* __restrict__ bits, u64* __restrict__ stat) {
    __shared__ u32 s_stat[R_COUNTERS];
    r_counters_zero(s_stat);
    const u64 u = (u64)blockIdx.x * 256u + threadIdx.x;
    const u32 mine = u < n_unitigs ? (u32)info[u] : 0u;
    if (mine & R_CAND) {
        const u64 A = 2 * u + ((mine >> 1) & 1u);
        const u64 Su = ab_sum[u], Lu = (u64)len[u];
        const u64 a0 = e_offsets[A], a1 = e_offsets[A + 1];
        u32 V[4], X[16], w[16];
        r_flank(a0, a1, e_offsets, e_targets, n_unitigs, n_edges, V, X);
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = r_other(X[j], u, n_unitigs);
        u32 wi[16], wl[16]; u64 ws[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const bool in = w[j] != R_NONE;
            wi[j] = in ? (u32)info[w[j]] : 0u; wl[j] = in ? len[w[j]] : 0u; ws[j] = in ? ab_sum[w[j]] : 0ull;
        }
        bool solid = false, stronger = false;                                 // a sibling that is no candidate / a candidate that is stronger
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (w[j] == R_NONE) continue;
            if (!(wi[j] & R_CAND)) { solid = true; continue; }
            const u64 l = ws[j] * Lu, r = Su * (u64)wl[j];
            stronger = stronger || l > r || (l == r && (u64)wl[j] > Lu);
        }
        const bool tip = solid || stronger, outranked = tip && !solid;
        bits[u] = (unsigned char)(R_CAND | (tip ? R_TAKEN : 0u) | (outranked ? T_OUTRANKED : 0u));
        atomicAdd(&s_stat[TP_CAND], 1u);
        if (tip) { atomicAdd(&s_stat[TP_TIPS], 1u); atomicAdd(&s_stat[TP_ROWS], (u32)Lu); }
        if (outranked) atomicAdd(&s_stat[TP_OUTRANKED], 1u);
    } else if (u < n_unitigs) {
        bits[u] = 0;
    }
    __syncthreads();
    r_counters_add(s_stat, stat);
}
