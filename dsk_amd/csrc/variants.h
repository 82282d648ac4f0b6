// variants.h -- HIP kernels that report the bubbles of the compacted de Bruijn graph as variants (gfx950 / MI355X, wave64): dskgpu_variants /
// dskgpu_variants_table / dskgpu_variants_stream (variants.hip; the definition is in include/dskgpu.h).
//
// Notation of bubbles.h: a candidate u is a simple path from P = in(u) ^ 1 to out(u); ends[u] = in(u) << 32 | out(u) and len[u] = L[u] come
// from k_bubble_candidates (bubbles.h; bubble_candidates() of rules.hip launches it), which runs first and is not restated here.  A
// variant is a pair a < b with b a sibling of a; its readings are A = 2 a and B = the X in E(P) that reaches b.
//
//   k_variant_pairs<EMIT>  per candidate a: E(P) (<= 4 targets X), then ends / len of every w = X >> 1 -- r_siblings of rules.h, the gather
//                          of k_bubble_decide, without the abundance sums.  The siblings w > a, each once, ascending by w.  EMIT = false
//                          writes their number, cnt[a]; the host scans it.  EMIT = true writes, from base[a] on, the first half of every
//                          record (A, B, from, to) as one 16-byte store, the two line lengths of the variant stream, and flag[a] = flag[b]
//                          = 1 (flag[] arrives zeroed; every store to it stores a 1)
//   k_variant_tlen         per unitig: tlen[u] = k + L[u] - 1 when flag[u], else 0 -- the host scans it into toff[], the place of every
//                          flagged unitig's letters --; counts the flagged unitigs per block in LDS
//   k_variant_letters<W>   per row, in the manner of k_unitig_stream<W>: a row of a flagged unitig writes the code of its last letter, the
//                          first row its k - 1 leading ones, to letters[toff[u] ..]; rows of other unitigs write nothing.  A letter is
//                          its 2-bit code in a byte (A C T G = 0 1 2 3), so the complement is code ^ 2
//   k_variant_compare      the hot kernel: one wave per variant.  Lane j holds letter j + 64 c of text(A) and of text(B) -- B read
//                          backwards and complemented when it is odd -- and the same two letters counted from the END of both texts; a chunk
//                          gives one 64-bit ballot of the mismatches from the front and one from the back.  lcp = the lowest set bit of the
//                          first non-zero front ballot (none: min(na, nb)), lcs = that of the back ballots, capped at min(na, nb) - lcp;
//                          n_mismatch = the popcounts of the front ballots when na == nb.  The lane writes its two front letters to the two
//                          lines of the variant stream on the way.  Lane 0 writes the second half of the record (lcp, lcs, n_mismatch, kind)
//                          as one 16-byte store; the kinds, the longest text and the variants that failed a check are combined per block in
//                          LDS, one atomic per counter and block.  The grid is a few blocks per CU; a wave takes every n_waves-th variant
//
// The chunk loop of k_variant_compare runs ceil(max(na, nb) / 64) times: na and nb are differences of toff[], checked against
// k + max_nodes - 1 and against the size of letters[] before the loop; its outer loop runs per_wave times, a number from the host; no
// letter decides a trip count.  Every index read from a table is
// checked against the table it is used on.
#pragma once
#include "graph.h"
#include "rules.h"

#define V_SNP 1u
#define V_MULTI 2u
#define V_INDEL 3u
#define V_COMPLEX 4u
#define V_NO_POS 0xFFFFFFFFu              // no mismatch seen yet

enum VStat { VS_SNP = 0, VS_MULTI, VS_INDEL, VS_COMPLEX, VS_UNITIGS, VS_BAD, VS_MAXLEN, VS_COUNT };

__device__ __forceinline__ void v_order(u64& x, u64& y) { const u64 lo = min(x, y), hi = max(x, y); x = lo; y = hi; }

template <bool EMIT>
__global__ __launch_bounds__(256) void k_variant_pairs(const u64* __restrict__ ends, const u32* __restrict__ len, const u64* __restrict__ e_offsets,
                                                       const u32* __restrict__ e_targets, u64 n_unitigs, u64 n_edges, u32 max_diff, int k,
                                                       u64* __restrict__ cnt, const u64* __restrict__ base, u64 n_variants, uint4* __restrict__ rec,
                                                       u64* __restrict__ vlen, unsigned char* __restrict__ flag) {
    const u64 u = (u64)blockIdx.x * 256u + threadIdx.x;
    const u64 mine = u < n_unitigs ? ends[u] : R_NO_ENDS;
    u64 key[4] = {~0ull, ~0ull, ~0ull, ~0ull};                               // X << 32 | L[w] of a sibling w > u; all ones: none
    u32 in = R_NONE, out = R_NONE, Lu = 0;
    if (mine != R_NO_ENDS) {
        in = (u32)(mine >> 32); out = (u32)mine;
        const u64 P = (u64)(in ^ 1u);                                         // (in < 2 n_unitigs, k_bubble_candidates checked it: so is its flip)
        Lu = len[u];
        const u64 p0 = e_offsets[P], p1 = e_offsets[P + 1];
        u32 T[4]; RSibling s[4];
        r_siblings<false>(p0, p1, u, ends, len, nullptr, e_targets, n_unitigs, n_edges, T, s);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (s[i].ends == R_NO_ENDS) continue;
            const bool same_ends = r_same_ends(T[i], s[i].ends, in, out);
            const u32 wl = s[i].len, X = T[i];
            const u32 diff = wl > Lu ? wl - Lu : Lu - wl;
            bool take = same_ends && diff <= max_diff && (u64)(X >> 1) > u;
#pragma unroll
            for (int j = 0; j < i; ++j) take = take && (key[j] == ~0ull || (u32)(key[j] >> 33) != (X >> 1));      // (each sibling once)
            if (take) key[i] = (u64)X << 32 | (u64)wl;
        }
        v_order(key[0], key[1]); v_order(key[2], key[3]); v_order(key[0], key[2]); v_order(key[1], key[3]); v_order(key[1], key[2]);      // ascending by w: the w are distinct
    }
    u32 n = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) n += key[i] != ~0ull ? 1u : 0u;
    if (!EMIT) {
        if (u < n_unitigs) cnt[u] = (u64)n;
        return;
    }
    if (n == 0u) return;
    const u64 at = base[u];
    flag[u] = 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const u64 v = at + (u64)i;
        if (key[i] == ~0ull || v >= n_variants) continue;                     // (v < n_variants: the host read the scan's total; the same guard)
        const u32 X = (u32)(key[i] >> 32), Lw = (u32)key[i];
        rec[2 * v] = make_uint4(2u * (u32)u, X, in ^ 1u, out);
        reinterpret_cast<ulonglong2*>(vlen)[v] = make_ulonglong2((u64)k + Lu, (u64)k + Lw);      // k + L - 1 letters and the '\n'
        flag[X >> 1] = 1;                                                     // (X >> 1 < n_unitigs: checked above)
    }
}

__global__ __launch_bounds__(256) void k_variant_tlen(const unsigned char* __restrict__ flag, const u32* __restrict__ len, u64 n_unitigs, int k, u64* __restrict__ tlen,
                                                      u64* __restrict__ stat) {
    __shared__ u32 s_cnt;
    if (threadIdx.x == 0) s_cnt = 0u;
    __syncthreads();
    const u64 u = (u64)blockIdx.x * 256u + threadIdx.x;
    const bool on = u < n_unitigs && flag[u] != 0;
    if (u <= n_unitigs) tlen[u] = on ? (u64)k + (u64)len[u] - 1ull : 0ull;    // (tlen[n_unitigs] = 0: the scan's last input)
    if (on) atomicAdd(&s_cnt, 1u);
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(reinterpret_cast<unsigned long long*>(&stat[VS_UNITIGS]), (unsigned long long)s_cnt);
}

template <int W>
__global__ __launch_bounds__(256) void k_variant_letters(RowsIn rows, u64 n, int k, const u32* __restrict__ unitig, const u32* __restrict__ pos_s,
                                                         const unsigned char* __restrict__ flag, const u64* __restrict__ toff, u64 n_unitigs, u64 n_letters,
                                                         unsigned char* __restrict__ letters) {
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const u32 u = unitig[r];
    if (u >= n_unitigs || flag[u] == 0) return;
    KN<W> x;
#pragma unroll
    for (int q = 0; q < W; ++q) x.w[q] = rows.w[q][r];
    const u32 ps = pos_s[r], pos = ps >> 1, s = ps & 1u;
    const u64 off = toff[u], end = toff[u + 1];
    if (end > n_letters || off + (u64)(k - 1) + pos >= end) return;           // (the row's letter lies inside its unitig's text, and the text inside letters[])
    // str(o) for s = 1 is the reverse complement: letter i of it is the complement (code ^ 2) of base i counted from the END of the row
    letters[off + (u64)(k - 1) + pos] = (unsigned char)(s ? u_base<W>(x, k - 1) ^ 2u : u_base<W>(x, 0));
    if (pos == 0u)
        for (int i = 0; i < k - 1; ++i) letters[off + (u64)i] = (unsigned char)(s ? u_base<W>(x, i) ^ 2u : u_base<W>(x, k - 1 - i));
}

// A wave takes the variants wave, wave + n_waves, ...: `per_wave` = ceil(n_variants / n_waves) of them, a number the host gives.  With one
// block per four variants the kernel was bound by its own counters: every block ends with two atomics on the same two words, 12 ns each
// one after the other (profiles/variants.md), so the grid is a few blocks per CU and the counters of a block cover all its variants.
__global__ __launch_bounds__(256) void k_variant_compare(uint4* __restrict__ rec, const u64* __restrict__ toff, const unsigned char* __restrict__ letters,
                                                         const u64* __restrict__ voff, u64 n_variants, u32 per_wave, u64 n_unitigs, u64 n_letters, u64 stream_bytes,
                                                         u32 max_letters, unsigned char* __restrict__ stream, u64* __restrict__ stat) {
    __shared__ u32 s_stat[VS_COUNT];
    if (threadIdx.x < VS_COUNT) s_stat[threadIdx.x] = 0u;
    __syncthreads();
    const u64 wave = (u64)blockIdx.x * 4u + (threadIdx.x >> 6), n_waves = (u64)gridDim.x * 4u;
    const u32 lane = threadIdx.x & 63u;
    for (u32 t = 0; t < per_wave; ++t) {
        const u64 v = wave + (u64)t * n_waves;                                // one wave per variant: everything up to the letters is the same in all its lanes
        if (v >= n_variants) break;
        const uint4 h = rec[2 * v];
        const u64 a = (u64)(h.x >> 1), b = (u64)(h.y >> 1);
        const bool b_odd = h.y & 1u;
        const bool in_table = a < n_unitigs && b < n_unitigs;
        const u64 ta = in_table ? toff[a] : 0ull, ta1 = in_table ? toff[a + 1] : 0ull, tb = in_table ? toff[b] : 0ull, tb1 = in_table ? toff[b + 1] : 0ull;
        const u64 o0 = voff[2 * v], o1 = voff[2 * v + 1], o2 = voff[2 * v + 2];
        const u64 na64 = ta1 - ta, nb64 = tb1 - tb;
        const bool ok = in_table && ta < ta1 && tb < tb1 && ta1 <= n_letters && tb1 <= n_letters && na64 <= (u64)max_letters && nb64 <= (u64)max_letters &&
                        o0 < o1 && o1 < o2 && o2 <= stream_bytes && o1 - o0 == na64 + 1ull && o2 - o1 == nb64 + 1ull;
        if (!ok) {
            if (lane == 0u) { rec[2 * v + 1] = make_uint4(0u, 0u, 0u, 0u); atomicAdd(&s_stat[VS_BAD], 1u); }
            continue;
        }
        const u32 na = (u32)na64, nb = (u32)nb64, m = min(na, nb), longest = max(na, nb);
        const unsigned char* A = letters + ta;
        const unsigned char* B = letters + tb;
        u32 lcp = V_NO_POS, lcs = V_NO_POS, nm = 0;
        for (u32 c0 = 0; c0 < longest; c0 += 64u) {                           // (longest <= max_letters: a bound from the tables)
            const u32 j = c0 + lane;
            const u32 fa = j < na ? (u32)A[j] : 4u;
            const u32 fb = j < nb ? (b_odd ? (u32)B[nb - 1u - j] ^ 2u : (u32)B[j]) : 5u;
            const u32 ra = j < m ? (u32)A[na - 1u - j] : 4u;
            const u32 rb = j < m ? (b_odd ? (u32)B[j] ^ 2u : (u32)B[nb - 1u - j]) : 4u;
            const u64 front = __ballot(j < m && fa != fb), back = __ballot(ra != rb);
            if (lcp == V_NO_POS && front) lcp = c0 + (u32)__ffsll((unsigned long long)front) - 1u;
            if (lcs == V_NO_POS && back) lcs = c0 + (u32)__ffsll((unsigned long long)back) - 1u;
            nm += (u32)__popcll(front);
            if (j < na) stream[o0 + j] = u_letter(fa);
            if (j < nb) stream[o1 + j] = u_letter(fb);
        }
        lcp = min(lcp, m);
        lcs = min(min(lcs, m), m - lcp);
        const bool same_len = na == nb;
        const u32 kind = same_len ? (nm == 1u ? V_SNP : nm >= 2u ? V_MULTI : 0u) : (lcp + lcs == m ? V_INDEL : V_COMPLEX);
        if (lane == 0u) {
            stream[o0 + na] = '\n'; stream[o1 + nb] = '\n';
            rec[2 * v + 1] = make_uint4(lcp, lcs, same_len ? nm : 0u, kind);
            if (kind) atomicAdd(&s_stat[VS_SNP + kind - 1u], 1u); else atomicAdd(&s_stat[VS_BAD], 1u);      // (equal texts cannot be: they would be the same rows)
            atomicMax(&s_stat[VS_MAXLEN], longest);
        }
    }
    __syncthreads();
    if (threadIdx.x < VS_MAXLEN && s_stat[threadIdx.x]) atomicAdd(reinterpret_cast<unsigned long long*>(&stat[threadIdx.x]), (unsigned long long)s_stat[threadIdx.x]);
    if (threadIdx.x == VS_MAXLEN && s_stat[VS_MAXLEN]) atomicMax(reinterpret_cast<unsigned long long*>(&stat[VS_MAXLEN]), (unsigned long long)s_stat[VS_MAXLEN]);
}
