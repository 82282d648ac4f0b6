// rules.h -- what the kernels of the graph rules share (gfx950 / MI355X, wave64): the tip rule (tips.h), the bubble rule (bubbles.h), the
// erroneous-connection rule (connections.h) and the variants read off the bubbles (variants.h).  Constants and __device__ __forceinline__
// helpers only, no kernel: any number of translation units may include it.
//
// Unitig u has L[u] = offsets[u + 1] - offsets[u] - k rows and the abundance sum S[u]; its oriented readings are U = 2 u + t with the
// targets E(U) = e_targets[e_offsets[U] .. e_offsets[U + 1]) (unitigs.h), at most 4 of them.  Everything is exact integer arithmetic on
// these tables.  A rule writes one byte per unitig: bit 0 = candidate, bit 1 = taken out (the tip, the popped branch, the removed
// connection) -- the bit k_tip_rows (rowfilter.h) turns into the rows' flags, whichever rule wrote it --, the bits above are the rule's
// own.  It counts four things per block in LDS, the last of them the rows it takes out, one atomic per counter and block.
//
// Every level of a gather is issued as one batch; every index read from a table is checked against the table it is used on.  The gathers
// take the offsets of an end (a0, a1), which the kernel loads itself, and the closing barrier of the counters stays in the kernel: in
// this form the compiler gives every kernel the registers, LDS and memory instructions it had before (profiles/graph_rules_unit.md).
#pragma once
#include "layouts.h"

#define R_NONE 0xFFFFFFFFu                 // no oriented unitig, no unitig (U_NONE of unitigs.h)
#define R_NO_ENDS 0xFFFFFFFFFFFFFFFFull    // ends[u] of a unitig that is no bubble candidate (both halves R_NONE: no oriented unitig has that number)
#define R_MAX_NODES 65535u                // the largest max_nodes: S of a candidate stays below 2^48, S * L of two candidates below 2^64

#define R_CAND 1u
#define R_TAKEN 2u
#define R_COUNTERS 4                      // counters of a rule; the last one, R_ROWS, is the rows it takes out
#define R_ROWS 3

// ---- the shape of a unitig, as the *_candidates kernels read it
struct RShape { u64 L, S, e0, e1, e2; u32 kind; };      // e0 .. e1: the targets of the reading 2u, e1 .. e2: those of 2u + 1

// WITH_S false: S = 0, ab_sum is not read
template <bool WITH_S>
__device__ __forceinline__ RShape r_shape(const u64* __restrict__ offsets, const unsigned char* __restrict__ kind, const u64* __restrict__ ab_sum,
                                          const u64* __restrict__ e_offsets, u64 u, int k) {
    const u64 o0 = offsets[u], o1 = offsets[u + 1], S = WITH_S ? ab_sum[u] : 0ull;
    const u64 e0 = e_offsets[2 * u], e1 = e_offsets[2 * u + 1], e2 = e_offsets[2 * u + 2];
    const u32 kd = kind[u];
    return RShape{o1 - o0 - (u64)k, S, e0, e1, e2, kd};
}

__device__ __forceinline__ u32 r_len(u64 L) { return (u32)min(L, 0xFFFFFFFFull); }      // len[u]: one word per sibling instead of two offsets

// ---- the gathers
// target i of the d = r_degree(a0, a1) targets e_targets[a0 .. a1) that are read, R_NONE where there is none; on false: no load
__device__ __forceinline__ u32 r_degree(u64 a0, u64 a1) { return (u32)min(a1 - a0, 4ull); }
__device__ __forceinline__ u32 r_target(bool on, u64 a0, u32 d, int i, const u32* __restrict__ e_targets, u64 n_edges) {
    return (on && (u32)i < d && a0 + i < n_edges) ? e_targets[a0 + i] : R_NONE;
}

// V[0 .. 4) = E(A)[0 .. 4) of the end A whose targets are e_targets[a0 .. a1), as one batch
__device__ __forceinline__ void r_targets(u64 a0, u64 a1, const u32* __restrict__ e_targets, u64 n_edges, u32* V) {
    const u32 d = r_degree(a0, a1);
#pragma unroll
    for (int i = 0; i < 4; ++i) V[i] = r_target(true, a0, d, i, e_targets, n_edges);
}

// the unitig of reading X when it is one of the table and not u itself, else R_NONE
__device__ __forceinline__ u32 r_other(u32 X, u64 u, u64 n_unitigs) {
    return (X != R_NONE && (u64)(X >> 1) < n_unitigs && (u64)(X >> 1) != u) ? X >> 1 : R_NONE;
}

// the flank of the end whose targets are e_targets[a0 .. a1): V = what it runs into, X[4 i .. 4 i + 4) = E(V[i] ^ 1), what runs into the same node
__device__ __forceinline__ void r_flank(u64 a0, u64 a1, const u64* __restrict__ e_offsets, const u32* __restrict__ e_targets, u64 n_unitigs, u64 n_edges,
                                        u32 (&V)[4], u32 (&X)[16]) {
    const u64 n_or = 2 * n_unitigs;
    r_targets(a0, a1, e_targets, n_edges, V);
    u64 b0[4], b1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const u64 F = (u64)(V[i] ^ 1u);
        const bool in = V[i] != R_NONE && F < n_or;
        b0[i] = in ? e_offsets[F] : 0ull; b1[i] = in ? e_offsets[F + 1] : 0ull;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) r_targets(b0[i], b1[i], e_targets, n_edges, X + 4 * i);
}

// the bubble rule's view of candidate u with ends[u] = in << 32 | out, a simple path from P = in ^ 1 to out, whose targets are
// e_targets[p0 .. p1): X = E(P)[0 .. 4), then ends / len / S of every w = X >> 1, w != u.  ends == R_NO_ENDS: no target, u itself, or no
// candidate.  WITH_S false: S = 0, ab_sum is not read
struct RSibling { u64 ends, S; u32 len; };

template <bool WITH_S>
__device__ __forceinline__ RSibling r_sibling(u32 X, u64 u, const u64* __restrict__ ends, const u32* __restrict__ len, const u64* __restrict__ ab_sum, u64 n_unitigs) {
    const u64 w = (u64)(X >> 1);
    const bool in_table = X != R_NONE && w < n_unitigs && w != u;
    RSibling s;
    s.ends = in_table ? ends[w] : R_NO_ENDS; s.len = in_table ? len[w] : 0u; s.S = (WITH_S && in_table) ? ab_sum[w] : 0ull;
    return s;
}

template <bool WITH_S>
__device__ __forceinline__ void r_siblings(u64 p0, u64 p1, u64 u, const u64* __restrict__ ends, const u32* __restrict__ len, const u64* __restrict__ ab_sum,
                                           const u32* __restrict__ e_targets, u64 n_unitigs, u64 n_edges, u32 (&X)[4], RSibling (&s)[4]) {
    r_targets(p0, p1, e_targets, n_edges, X);
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = r_sibling<WITH_S>(X[i], u, ends, len, ab_sum, n_unitigs);
}

// w, reached from P as the reading X, has the ends of u in that orientation (X even: out(w) == out(u) and in(w) == in(u); X odd: swapped)
__device__ __forceinline__ bool r_same_ends(u32 X, u64 w_ends, u32 in, u32 out) {
    const u32 wi = (u32)(w_ends >> 32), wo = (u32)w_ends;
    return (X & 1u) ? (wi == out && wo == in) : (wo == out && wi == in);
}

// ---- the four counters of a *_decide kernel, s_stat = its __shared__ u32[R_COUNTERS]; every thread of the block calls both.  Between
// them the kernel adds to s_stat with LDS atomics (a block's sum of rows: 256 candidates of <= 65535 rows, 32 bits hold it) and ends with
// a barrier
__device__ __forceinline__ void r_counters_zero(u32 (&s_stat)[R_COUNTERS]) {
    if (threadIdx.x < R_COUNTERS) s_stat[threadIdx.x] = 0u;
    __syncthreads();
}

// one atomic per counter and block that has something
__device__ __forceinline__ void r_counters_add(u32 (&s_stat)[R_COUNTERS], u64* stat) {
    if (threadIdx.x < R_COUNTERS && s_stat[threadIdx.x]) atomicAdd(reinterpret_cast<unsigned long long*>(&stat[threadIdx.x]), (unsigned long long)s_stat[threadIdx.x]);
}
