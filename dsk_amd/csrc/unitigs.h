// unitigs.h -- HIP kernels of the compaction of the rows' de Bruijn graph into unitigs (gfx950 / MI355X, wave64): dskgpu_unitigs*
// (unitigs.hip; the definition is in include/dskgpu.h).
//
// Row r gives two ORIENTED nodes o = 2 r + s: s = 0 reads the row's canonical value, s = 1 its reverse complement; flip(o) = o ^ 1.
// next(o) is the one successor of o when o has out-degree 1, that successor has in-degree 1, both are different rows and neither is its
// own reverse complement; links are symmetric, next(o) = p <=> next(flip(p)) = flip(o), so prev(o) = flip(next(flip(o))).
//
//   k_unitig_links<W>   next[] of both sides of every row from the adjacency bytes (k_graph_rows<W>, graph.h): a side whose nibble has one
//                       bit derives that neighbour (graph.h's g_* helpers), probes its ROW NUMBER (q_lookup<W, N, true>), reads the
//                       neighbour's byte for the in-degree; writes next[] and the start of the ranking, P[o] = (prev(o), 1) / head: (o, 0, done)
//   k_unitig_jump       one round of pointer jumping towards the head, in place: P[o] = (anc, dist, done) packed in ONE 64-bit word, so a
//                       reader always sees a pair that was true at some time -- a stale or a fresher P[anc] both give a valid longer jump.
//                       done <=> anc is a head.  Counts the nodes it resolved; a round that resolves none ends the phase (the host reads
//                       the counter), what is left lies on cycles
//   k_unitig_cyc_init / _cyc_min / _cyc_cut
//                       the nodes left: Q[o] = (mn, ptr) from (o, next(o)); a round takes mn = min(mn, mn[ptr]), ptr = ptr[ptr] -- mn[o] is
//                       always the minimum of the run of nodes from o up to ptr[o], whatever mixture of old and new words a round reads.  A
//                       round that lowers no mn has reached every cycle's minimum.  Of a cycle and its flip the one whose minimum is even
//                       (it holds 2 * the smallest row) is kept and cut in front of that node, the other is marked (anc = U_NONE);
//                       k_unitig_jump then ranks the kept ones like chains
//   k_unitig_first      per row: is it the first node of its unitig in the reported reading, and of how many nodes -> (1 << 32 | nodes) or 0;
//                       an exclusive scan of these words gives (unitig number << 32 | nodes before) at every first row
//   k_unitig_number     per row: unitig number and (position << 1 | s); the first node writes offsets[] and kind[]; abundance sums
//   k_unitig_stream<W>  the letters: every node its last one, the first node its k - 1 leading ones, the last node the '\n'
//
// The EDGES between the unitigs (dskgpu_unitig_edges*): an oriented unitig is U = 2 u + t, t = 1 reads unitig u backwards;
// first(2u) = o_0, last(2u) = o_{L-1}, first(2u + 1) = flip(o_{L-1}), last(2u + 1) = flip(o_0); U -> V <=> first(V) is in succ(last(U)).
//
//   k_unitig_ends       per row: the row at position 0 writes ends[2u + 1] = flip(its node), the one at position nodes - 1 ends[2u] = its
//                       node -- ends[U] = last(U), and first(V) = flip(ends[flip(V)])
//   k_unitig_edges<W>   per oriented unitig: the row of last(U), oriented; its four successors (g_* helpers) probed as one batch for their ROW
//                       NUMBERS; a hit (p, sp) is first(V) of exactly one V of unitig[p]: the one with ends[V ^ 1] = flip(2 p + sp).  Neither
//                       of the two: the edge would land inside a unitig, which the links exclude -- counted, the host turns it into an error.
//                       Writes four target slots (base order A, C, T, G; U_NONE = no edge) and the degree; counts edges, self edges, dead ends,
//                       the largest degree per block in LDS
//   k_unitig_edge_fill  per oriented unitig: its slots that hold a target, in order, to targets[] from offsets[U] (the scan of the degrees) on
//
// Every kernel is one pass over its nodes, rows or unitigs: no loop on the device depends on the data but q_lookup's probe run.
#pragma once
#include "graph.h"

#define U_NONE 0xFFFFFFFFu
#define U_DONE 0x8000000000000000ull
#define U_DIST 0x7FFFFFFFull              // dist < rows <= 2^31 - 1
#define U_QNONE 0xFFFFFFFFFFFFFFFFull     // Q[] of a node that is on no cycle
#define U_ROUNDS 33                       // 2^33 > 2 * the most rows: a phase that needs more rounds is broken
#define U_JUMP 4                          // nodes per thread of the jumping kernels: all their loads are issued before any is used

// rows per thread of k_unitig_links: two keys per row, 8 / 4 / 2 keys in flight (half of QBatch: the neighbour's byte is a third level)
template <int W> struct UBatch { static constexpr int R = W == 1 ? 4 : W == 2 ? 2 : 1; };

enum UStat { US_CYCLES = 0, US_SINGLE, US_MAX, US_COUNT };

// oriented unitigs per thread of k_unitig_edges: four keys each, 16 / 8 / 4 keys in flight (QBatch's budget: the probe is followed by two
// dependent levels of one word each, unitig[] and the ends, not by a neighbour's byte per key as in k_unitig_links)
template <int W> struct UEBatch { static constexpr int R = W == 1 ? 4 : W == 2 ? 2 : 1; };

enum UEStat { UE_EDGES = 0, UE_SELF, UE_DEAD, UE_BROKEN, UE_MAXDEG, UE_COUNT };

template <int W> __device__ __forceinline__ bool u_less(const KN<W>& a, const KN<W>& b) {
    bool lt = false, decided = false;
#pragma unroll
    for (int i = W - 1; i >= 0; --i) { if (!decided && a.w[i] != b.w[i]) { lt = a.w[i] < b.w[i]; decided = true; } }
    return lt;
}
template <int W> __device__ __forceinline__ bool u_same(const KN<W>& a, const KN<W>& b) {
    bool eq = true;
#pragma unroll
    for (int i = 0; i < W; ++i) eq = eq && a.w[i] == b.w[i];
    return eq;
}
template <int W>
__global__ __launch_bounds__(256) void k_unitig_links(RowsIn rows, u64 n, int k, QTable T, const unsigned char* __restrict__ adj,
                                                      u32* __restrict__ nxt, u64* __restrict__ P) {
    constexpr int R = UBatch<W>::R, N = 2 * R;
    const u64 base = (u64)blockIdx.x * (256u * R) + threadIdx.x;
    u64 msk[W];
    g_masks<W>(k, msk);
    const int top = 2 * k - 2, tw = top >> 6, tb = top & 63;
    KN<W> c[N];
    u32 pend = 0, flipped = 0;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const u64 r = base + (u64)i * 256u;
        const bool in = r < n;
        KN<W> x;
#pragma unroll
        for (int q = 0; q < W; ++q) x.w[q] = in ? rows.w[q][r] : 0ull;
        const u32 a = in ? adj[r] : 0u;
        const KN<W> rc = g_revcomp<W>(x, k, msk);
        const bool pal = u_same<W>(x, rc);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            // side 0: str(o) = x, successor base b = bit b of the low nibble.  Side 1: str(o) = rc(x); bit 4 + b says pred_b(x) is a row, which
            // is the reverse complement of rc(x)[1..] . (b ^ 2)
            const u32 nib = s ? a >> 4 : a & 15u;
            const u64 b = nib ? (u64)(__ffs(nib) - 1) : 0ull;
            const KN<W> f = s ? g_push_low<W>(rc, b ^ 2ull, msk) : g_push_low<W>(x, b, msk);            // the neighbour as o reads it
            const KN<W> v = s ? g_push_top<W>(x, b, tw, tb) : g_push_top<W>(rc, b ^ 2ull, tw, tb);      // its reverse complement
            const bool sp = u_less<W>(v, f);
#pragma unroll
            for (int q = 0; q < W; ++q) c[2 * i + s].w[q] = sp ? v.w[q] : f.w[q];
            if (in && __popc(nib) == 1 && !pal && !u_same<W>(v, f)) pend |= 1u << (2 * i + s);
            if (sp) flipped |= 1u << (2 * i + s);
        }
    }
    u32 prow[N];
    q_lookup<W, N, true>(T, c, pend, prow);
    u32 pa[N];
#pragma unroll
    for (int j = 0; j < N; ++j) pa[j] = prow[j] != Q_NO_ROW ? (u32)adj[prow[j]] : 0u;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const u64 r = base + (u64)i * 256u;
        u32 nx[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int j = 2 * i + s;
            const u32 sp = (flipped >> j) & 1u;
            const u32 indeg = __popc(sp ? pa[j] & 15u : pa[j] >> 4);          // out-degree of flip(p)
            nx[s] = (prow[j] != Q_NO_ROW && indeg == 1u && prow[j] != (u32)r) ? 2u * prow[j] + sp : U_NONE;
        }
        if (r < n) {
            reinterpret_cast<uint2*>(nxt)[r] = make_uint2(nx[0], nx[1]);
            const u32 o = 2u * (u32)r;
            ulonglong2 p;                                                      // prev(2r) = flip(next(2r + 1)) and the other way round
            p.x = nx[1] == U_NONE ? (U_DONE | o) : ((1ull << 32) | (nx[1] ^ 1u));
            p.y = nx[0] == U_NONE ? (U_DONE | (o + 1u)) : ((1ull << 32) | (nx[0] ^ 1u));
            reinterpret_cast<ulonglong2*>(P)[r] = p;
        }
    }
}

// add `mine` of every thread of the block to *counter: LDS first, one vector atomic per block that has something
__device__ __forceinline__ void u_block_count(u32 mine, u32* counter) {
    __shared__ u32 s_cnt;
    if (threadIdx.x == 0) s_cnt = 0u;
    __syncthreads();
    if (mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(counter, s_cnt);
}

__global__ __launch_bounds__(256) void k_unitig_jump(u64* P, u64 n_nodes, u32* counter) {
    const u64 base = (u64)blockIdx.x * (256u * U_JUMP) + threadIdx.x;
    u64 p[U_JUMP], q[U_JUMP];
#pragma unroll
    for (int i = 0; i < U_JUMP; ++i) { const u64 o = base + (u64)i * 256u; p[i] = o < n_nodes ? P[o] : U_DONE; }
#pragma unroll
    for (int i = 0; i < U_JUMP; ++i) q[i] = (p[i] & U_DONE) ? 0ull : P[(u32)p[i]];
    u32 resolved = 0;
#pragma unroll
    for (int i = 0; i < U_JUMP; ++i) {
        if (p[i] & U_DONE) continue;
        // the ancestor's ancestor, the distances added; a head holds (itself, 0, done), so an ancestor that is a head stays and sets done
        const u64 nw = (q[i] & U_DONE) | ((((p[i] >> 32) + (q[i] >> 32)) & U_DIST) << 32) | (u64)(u32)q[i];
        P[base + (u64)i * 256u] = nw;
        resolved += (u32)(nw >> 63);
    }
    u_block_count(resolved, counter);
}

__global__ __launch_bounds__(256) void k_unitig_cyc_init(const u64* __restrict__ P, const u32* __restrict__ nxt, u64 n_nodes, u64* __restrict__ Q, u32* counter) {
    const u64 o = (u64)blockIdx.x * 256u + threadIdx.x;
    u32 left = 0;
    if (o < n_nodes) {
        left = (P[o] & U_DONE) ? 0u : 1u;
        const u32 nx = nxt[o];                                               // (a node that is left has a next; were the links broken, it points at itself: no index leaves the array)
        if (Q) Q[o] = left ? ((o << 32) | (nx < n_nodes ? nx : (u32)o)) : U_QNONE;      // (Q null: only the count)
    }
    u_block_count(left, counter);
}

__global__ __launch_bounds__(256) void k_unitig_cyc_min(u64* Q, u64 n_nodes, u32* counter) {
    const u64 base = (u64)blockIdx.x * (256u * U_JUMP) + threadIdx.x;
    u64 q[U_JUMP], t[U_JUMP];
#pragma unroll
    for (int i = 0; i < U_JUMP; ++i) { const u64 o = base + (u64)i * 256u; q[i] = o < n_nodes ? Q[o] : U_QNONE; }
#pragma unroll
    for (int i = 0; i < U_JUMP; ++i) t[i] = q[i] == U_QNONE ? 0ull : Q[(u32)q[i]];
    u32 lowered = 0;
#pragma unroll
    for (int i = 0; i < U_JUMP; ++i) {
        if (q[i] == U_QNONE) continue;
        const u64 mn = min(q[i] >> 32, t[i] >> 32);
        Q[base + (u64)i * 256u] = (mn << 32) | (u64)(u32)t[i];
        lowered += mn < (q[i] >> 32) ? 1u : 0u;
    }
    u_block_count(lowered, counter);
}

__global__ __launch_bounds__(256) void k_unitig_cyc_cut(u64* __restrict__ P, const u64* __restrict__ Q, const u32* __restrict__ nxt, u64 n_nodes) {
    const u64 o = (u64)blockIdx.x * 256u + threadIdx.x;
    if (o >= n_nodes) return;
    const u64 q = Q[o];
    if (q == U_QNONE) return;
    const u32 mn = (u32)(q >> 32);
    if (mn & 1u) P[o] = U_DONE | U_NONE;                       // the flip of a kept cycle
    else if (mn == (u32)o) P[o] = U_DONE | o;                  // the cut: the kept cycle starts here
    else { const u32 nf = nxt[o ^ 1ull]; P[o] = nf < n_nodes ? ((1ull << 32) | (nf ^ 1u)) : (U_DONE | o); }      // (nf: always a node, see k_unitig_cyc_init)
}

// val[r] = (1 << 32 | nodes of the unitig) when a side of row r is the first node of the reported reading, else 0
__global__ __launch_bounds__(256) void k_unitig_first(const u64* __restrict__ P, const u32* __restrict__ nxt, u64 n, u64* __restrict__ val, u64* __restrict__ stat) {
    __shared__ u32 s_stat[US_COUNT];
    if (threadIdx.x < US_COUNT) s_stat[threadIdx.x] = 0u;
    __syncthreads();
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r < n) {
        const ulonglong2 pp = reinterpret_cast<const ulonglong2*>(P)[r];
        const uint2 nx = reinterpret_cast<const uint2*>(nxt)[r];
        u64 out = 0;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const u64 p = s ? pp.y : pp.x, pf = s ? pp.x : pp.y;
            const u32 nf = s ? nx.x : nx.y;                                      // next(flip(o)): none <=> o has no prev
            if ((u32)p == U_NONE || ((p >> 32) & U_DIST) != 0ull) continue;      // (dist 0: a head, or the cut of a kept cycle)
            if (nf != U_NONE) {                                                  // a cycle: its last node is prev(o), at position nodes - 1
                const u64 len = ((P[nf ^ 1u] >> 32) & U_DIST) + 1ull;
                out = (1ull << 32) | len;
                atomicAdd(&s_stat[US_CYCLES], 1u); atomicMax(&s_stat[US_MAX], (u32)len);
            } else {                                                             // a chain: tail(o) = flip(head(flip(o))), nodes = dist(flip(o)) + 1
                const u64 len = ((pf >> 32) & U_DIST) + 1ull;
                const u32 tail_row = ((u32)pf ^ 1u) >> 1;
                if ((u32)r < tail_row || (len == 1ull && s == 0)) {
                    out = (1ull << 32) | len;
                    if (len == 1ull) atomicAdd(&s_stat[US_SINGLE], 1u);
                    atomicMax(&s_stat[US_MAX], (u32)len);
                }
            }
        }
        val[r] = out;
    }
    __syncthreads();
    if (threadIdx.x < US_MAX && s_stat[threadIdx.x]) atomicAdd(reinterpret_cast<unsigned long long*>(&stat[threadIdx.x]), (unsigned long long)s_stat[threadIdx.x]);
    if (threadIdx.x == US_MAX && s_stat[US_MAX]) atomicMax(reinterpret_cast<unsigned long long*>(&stat[US_MAX]), (unsigned long long)s_stat[US_MAX]);
}

// scan[r] at a first row = (unitig number << 32 | nodes before it).  offsets[n_unitigs] is written by the thread of row 0.
__global__ __launch_bounds__(256) void k_unitig_number(const u64* __restrict__ P, const u64* __restrict__ scan, const u32* __restrict__ ab, u64 n, int k, u64 n_unitigs,
                                                       u32* __restrict__ unitig, u32* __restrict__ pos_s, u64* __restrict__ offsets,
                                                       u64* __restrict__ ab_sum, unsigned char* __restrict__ kind) {
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const ulonglong2 pp = reinterpret_cast<const ulonglong2*>(P)[r];
    const u32 a0 = (u32)pp.x, a1 = (u32)pp.y;
    // a cycle: the side that is on the kept one.  A chain: the reading whose first row is the smaller (a single node: forward)
    const bool cyc = a0 == U_NONE || a1 == U_NONE;
    const u32 s = cyc ? (a0 == U_NONE ? 1u : 0u) : ((a0 >> 1) <= ((a1 ^ 1u) >> 1) ? 0u : 1u);
    const u64 p = s ? pp.y : pp.x;
    const u32 dist = (u32)((p >> 32) & U_DIST);
    const u64 sc = scan[min((u64)((u32)p >> 1), n - 1)];
    const u32 u = (u32)(sc >> 32);
    unitig[r] = u;
    pos_s[r] = (dist << 1) | s;
    if (u >= n_unitigs) return;                                               // (cannot be: the host checked that the firsts add up; no index leaves an array)
    atomicAdd(reinterpret_cast<unsigned long long*>(&ab_sum[u]), (unsigned long long)ab[r]);
    if (dist == 0u) { offsets[u] = (sc & 0xFFFFFFFFull) + (u64)u * (u64)k; kind[u] = cyc ? 1 : 0; }
    if (r == 0) offsets[n_unitigs] = n + n_unitigs * (u64)k;
}

template <int W>
__global__ __launch_bounds__(256) void k_unitig_stream(RowsIn rows, u64 n, int k, const u32* __restrict__ unitig, const u32* __restrict__ pos_s,
                                                       const u64* __restrict__ offsets, u64 n_unitigs, unsigned char* __restrict__ out) {
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r >= n || unitig[r] >= n_unitigs) return;
    KN<W> x;
#pragma unroll
    for (int q = 0; q < W; ++q) x.w[q] = rows.w[q][r];
    const u32 u = unitig[r], ps = pos_s[r], pos = ps >> 1, s = ps & 1u;
    const u64 off = offsets[u], nodes = offsets[u + 1] - off - (u64)k;
    if (off + (u64)k + pos >= n + n_unitigs * (u64)k) return;                 // (the row's last byte lies inside the stream: the same guard)
    // str(o) for s = 1 is the reverse complement: letter i of it is the complement (code ^ 2) of base i counted from the END of the row
    out[off + (u64)(k - 1) + pos] = u_letter(s ? u_base<W>(x, k - 1) ^ 2u : u_base<W>(x, 0));
    if (pos == 0u)
        for (int i = 0; i < k - 1; ++i) out[off + (u64)i] = u_letter(s ? u_base<W>(x, i) ^ 2u : u_base<W>(x, k - 1 - i));
    if ((u64)pos + 1ull == nodes) out[off + (u64)k + pos] = '\n';
}

// ends[] arrives filled with U_NONE: an end that no row writes (it cannot be) stays a value that is no node and fails every guard after it
__global__ __launch_bounds__(256) void k_unitig_ends(const u32* __restrict__ unitig, const u32* __restrict__ pos_s, const u64* __restrict__ offsets, u64 n, int k,
                                                     u64 n_unitigs, u32* __restrict__ ends) {
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const u32 u = unitig[r], ps = pos_s[r];
    if (u >= n_unitigs) return;                                               // (cannot be: k_unitig_number numbered every row; no index leaves an array)
    const u64 nodes = offsets[u + 1] - offsets[u] - (u64)k;
    const u32 o = 2u * (u32)r + (ps & 1u);
    if ((ps >> 1) == 0u) ends[2u * u + 1u] = o ^ 1u;
    if ((u64)(ps >> 1) + 1ull == nodes) ends[2u * u] = o;
}

template <int W>
__global__ __launch_bounds__(256) void k_unitig_edges(RowsIn rows, u64 n, int k, QTable T, const u32* __restrict__ unitig, const u32* __restrict__ ends,
                                                      u64 n_unitigs, u32* __restrict__ slots, u64* __restrict__ deg, u64* __restrict__ stat) {
    constexpr int R = UEBatch<W>::R, N = 4 * R;
    __shared__ u32 s_stat[UE_COUNT];
    if (threadIdx.x < UE_COUNT) s_stat[threadIdx.x] = 0u;
    __syncthreads();
    const u64 n_or = 2 * n_unitigs;
    const u64 base = (u64)blockIdx.x * (256u * R) + threadIdx.x;
    u64 msk[W];
    g_masks<W>(k, msk);
    const int top = 2 * k - 2, tw = top >> 6, tb = top & 63;
    u32 e[R];
#pragma unroll
    for (int i = 0; i < R; ++i) { const u64 U = base + (u64)i * 256u; e[i] = U < n_or ? ends[U] : U_NONE; }
    KN<W> c[N];
    u32 pend = 0, flipped = 0, broken = 0;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const u64 U = base + (u64)i * 256u;
        const u64 r = e[i] >> 1;
        const bool in = U < n_or && r < n;                                    // (an end that is no node: nothing is probed, the unitig is counted as broken)
        if (U < n_or && !in) ++broken;
        KN<W> x;
#pragma unroll
        for (int q = 0; q < W; ++q) x.w[q] = in ? rows.w[q][r] : 0ull;
        const KN<W> rc = g_revcomp<W>(x, k, msk);
        const bool odd = e[i] & 1u;
        KN<W> fw, bw;                                                         // str(last(U)) and its reverse complement
#pragma unroll
        for (int q = 0; q < W; ++q) { fw.w[q] = odd ? rc.w[q] : x.w[q]; bw.w[q] = odd ? x.w[q] : rc.w[q]; }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const KN<W> f = g_push_low<W>(fw, (u64)b, msk);                   // the successor as last(U) reads it
            const KN<W> v = g_push_top<W>(bw, (u64)(b ^ 2), tw, tb);          // its reverse complement
            const bool sp = u_less<W>(v, f);                                  // (a palindrome: equal, forward)
#pragma unroll
            for (int q = 0; q < W; ++q) c[4 * i + b].w[q] = sp ? v.w[q] : f.w[q];
            if (in) pend |= 1u << (4 * i + b);
            if (sp) flipped |= 1u << (4 * i + b);
        }
    }
    u32 prow[N];
    q_lookup<W, N, true>(T, c, pend, prow);
    u32 pu[N];
#pragma unroll
    for (int j = 0; j < N; ++j) pu[j] = prow[j] < n ? unitig[prow[j]] : U_NONE;
    uint2 pe[N];                                                              // (ends[2v], ends[2v + 1]) of the hit's unitig v
#pragma unroll
    for (int j = 0; j < N; ++j) pe[j] = pu[j] < n_unitigs ? reinterpret_cast<const uint2*>(ends)[pu[j]] : make_uint2(U_NONE, U_NONE);
    u32 edges = 0, self = 0, dead = 0, maxdeg = 0;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const u64 U = base + (u64)i * 256u;
        u32 tg[4], d = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = 4 * i + b;
            tg[b] = U_NONE;
            if (prow[j] == Q_NO_ROW) continue;
            const u32 back = (2u * prow[j] + ((flipped >> j) & 1u)) ^ 1u;      // flip(first(V)) = ends[flip(V)]
            if (pu[j] < n_unitigs && pe[j].y == back) tg[b] = 2u * pu[j];
            else if (pu[j] < n_unitigs && pe[j].x == back) tg[b] = 2u * pu[j] + 1u;
            else { ++broken; continue; }
            ++d;
            self += (u64)(tg[b] >> 1) == (U >> 1) ? 1u : 0u;
        }
        if (U < n_or) {
            reinterpret_cast<uint4*>(slots)[U] = make_uint4(tg[0], tg[1], tg[2], tg[3]);
            deg[U] = (u64)d;
            edges += d; dead += d == 0u ? 1u : 0u; maxdeg = max(maxdeg, d);
        }
    }
    if (edges) atomicAdd(&s_stat[UE_EDGES], edges);
    if (self) atomicAdd(&s_stat[UE_SELF], self);
    if (dead) atomicAdd(&s_stat[UE_DEAD], dead);
    if (broken) atomicAdd(&s_stat[UE_BROKEN], broken);
    if (maxdeg) atomicMax(&s_stat[UE_MAXDEG], maxdeg);
    __syncthreads();
    if (threadIdx.x < UE_MAXDEG && s_stat[threadIdx.x]) atomicAdd(reinterpret_cast<unsigned long long*>(&stat[threadIdx.x]), (unsigned long long)s_stat[threadIdx.x]);
    if (threadIdx.x == UE_MAXDEG && s_stat[UE_MAXDEG]) atomicMax(reinterpret_cast<unsigned long long*>(&stat[UE_MAXDEG]), (unsigned long long)s_stat[UE_MAXDEG]);
}

// offsets[U] .. offsets[U + 1]: where the targets of U go (n_or + 1 offsets, the last one = n_edges)
__global__ __launch_bounds__(256) void k_unitig_edge_fill(const u32* __restrict__ slots, const u64* __restrict__ offsets, u64 n_or, u64 n_edges, u32* __restrict__ targets) {
    const u64 U = (u64)blockIdx.x * 256u + threadIdx.x;
    if (U >= n_or) return;
    const uint4 s = reinterpret_cast<const uint4*>(slots)[U];
    const u32 tg[4] = {s.x, s.y, s.z, s.w};
    u64 at = offsets[U];
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (tg[b] != U_NONE && at < n_edges) targets[at++] = tg[b];           // (at < n_edges: the host checked that the degrees add up; the same guard)
}
