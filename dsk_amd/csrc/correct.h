// correct.h -- HIP kernels that correct substitution errors in reads against the last result (gfx950 / MI355X, wave64):
// dskgpu_correct_reads (correct.hip; the rule is in include/dskgpu.h).
//
// state(p) of the window ending at byte p: 0 = not valid, 1 = valid but not trusted, 2 = trusted (a row of abundance >= tmin).  A GAP is a
// maximal run [a, b] of state 1; the two states beside it give its shape and the one byte e that all its windows share.
//
//   k_correct_state<W>     the frame of k_query_reads<W>: the N = 16 / W windows of a thread probed as one batch (q_lookup), one state byte
//                          per position into a buffer of the library's own that is padded to whole words of 32 positions -- so a lane's N
//                          states always leave as ONE 16-, 8- or 4-byte store.  n_valid / n_trusted: per block in LDS, one add per block
//   k_correct_gaps<EMIT>   16 positions per thread (one 16-byte load of states + the byte behind them).  The thread that holds the last
//                          position b of a gap walks back over at most k + 1 state bytes to its first position and classifies it.  EMIT
//                          false: the shaped gaps of every block (scanned by the host side) and the five gap counters; EMIT true: the same
//                          gaps again, ranked inside the block (wave_incl_scan + the waves' totals in LDS) on top of the scanned block
//                          sums -> the candidate list (e, a, m, shape).  The list is in stream order, which the result does not need
//   k_correct_plain<W>     one thread per candidate, 3 x m windows one after the other, an alternative dropped at its first failure.  THE
//                          DEFAULT: on 10 M reads it ran the trials in 14.7 ms against 16.8 ms of the staged pair below -- both issue
//                          the same lookups, and with millions of candidates in flight their rate, not the length of a thread's
//                          chain, is the limit (profiles/read_correction.md)
//   k_correct_first<W>     (with k_correct_rest: DSKGPU_CORRECT_STAGED) per candidate ONE window (the one ending at a) of each of the three
//                          alternatives, CBatch::CAND candidates of a thread as one batch of 3 * CAND independent chains.  A wrong alternative almost always dies here.  A gap of one
//                          window, or one with no alternative left, is decided here; the others leave their surviving alternatives (3 bits)
//   k_correct_rest<W>      one wave per surviving candidate: for each surviving alternative the m - 1 other windows spread over the lanes,
//                          two per lane as one batch (m - 1 <= 127), a ballot for the verdict; lane 0 decides and writes.  The pair is
//                          the second implementation, which the tests compare with the default in a fresh process
//
// The forward value of a window is a funnel shift over the packed words (as k_thread_place derives the orientation), base e is patched in
// it, the reverse complement is graph.h's g_revcomp.  The deciding kernel writes out[e]; every e belongs to one gap, so in place is safe.
//
// Global atomics: as in k_query_build, this is not the count path; every counter is combined per block first.
#pragma once
#include "graph.h"

#define C_PER 16                          // positions per thread of k_correct_gaps: one 16-byte load of states
#define C_BLOCK (256 * C_PER)             // positions per block of it

enum CStat { CS_VALID = 0, CS_TRUSTED, CS_GAPS, CS_INTERIOR, CS_HEAD, CS_TAIL, CS_SKIPPED, CS_CORRECTED, CS_AMBIGUOUS, CS_UNFIXABLE, CS_COUNT };
enum CShape { C_INTERIOR = 0, C_HEAD = 1, C_TAIL = 2, C_SKIPPED = 3 };

struct CGap { u64 e, a; u32 m, shape; };  // candidate byte, first position, windows, CShape
template <int W> struct CBatch { static constexpr int CAND = W == 1 ? 4 : W == 2 ? 2 : 1; };      // candidates per thread of k_correct_first: 12 / 6 / 3 keys

// stat[first + i] += the sum over the block of mine[i], i < NC: LDS first, one add per counter and block that has something.  Every thread
// of the block calls it, once per kernel.
template <int NC>
__device__ __forceinline__ void c_block_counts(const u32 (&mine)[NC], u64* stat, int first) {
    __shared__ u32 s_cnt[NC];
    if (threadIdx.x < NC) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NC; ++i) if (mine[i]) atomicAdd(&s_cnt[i], mine[i]);
    __syncthreads();
    if (threadIdx.x < NC && s_cnt[threadIdx.x]) q_add64(stat + first + threadIdx.x, (u64)s_cnt[threadIdx.x]);
}

// Thread t: the N windows ending at bases 32 * (t / TPW) + (t % TPW) * N + j of the encoded stream, as k_query_reads.  state: nwords * 32
// bytes, 16-byte aligned; the positions from nbytes on get 0.  tmin >= 1
template <int W>
__global__ __launch_bounds__(256) void k_correct_state(const u64* __restrict__ packed, const u32* __restrict__ inval, u64 nwords, u64 nbytes, int k,
                                                       QTable T, u32 tmin, unsigned char* __restrict__ state, u64* __restrict__ stat) {
    constexpr int N = QBatch<W>::N, TPW = 32 / N;
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 wi = t / TPW;
    u32 cnt[2] = {0u, 0u};
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
        u32 res[N];
        q_lookup<W, N>(T, c, vm, res);
        u32 tr = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) if (((vm >> j) & 1u) && res[j] >= tmin) tr |= 1u << j;
        cnt[0] = __popc(vm); cnt[1] = __popc(tr);
        u32 word[N / 4];                                                         // state bytes, position p0 + j in byte j
#pragma unroll
        for (int q = 0; q < N / 4; ++q) {
            word[q] = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) word[q] |= (((vm >> (4 * q + j)) & 1u) + ((tr >> (4 * q + j)) & 1u)) << (8 * j);
        }
        if constexpr (N == 16) *reinterpret_cast<uint4*>(state + p0) = make_uint4(word[0], word[1], word[2], word[3]);
        else if constexpr (N == 8) *reinterpret_cast<uint2*>(state + p0) = make_uint2(word[0], word[1]);
        else *reinterpret_cast<u32*>(state + p0) = word[0];
    }
    c_block_counts<2>(cnt, stat, CS_VALID);
}

// The gap that ends at b (state(b) == 1, `right` = state(b + 1), 0 behind the stream): its first position, its windows and its shape.
// Reads at most k + 1 state bytes below b.
__device__ __forceinline__ CGap c_classify(const unsigned char* __restrict__ S, int k, u64 b, u32 right) {
    u64 a = b;
    while (a > 0 && b - a + 1 <= (u64)k && S[a - 1] == 1) --a;
    CGap g;
    g.a = a; g.m = (u32)(b - a + 1); g.e = a; g.shape = C_SKIPPED;
    if (g.m > (u32)k) return g;
    const u32 left = a > 0 ? S[a - 1] : 0u;
    if (left == 2 && right == 2 && g.m == (u32)k) g.shape = C_INTERIOR;
    else if (left == 0 && right == 2) { g.shape = C_HEAD; g.e = b + 1 - (u64)k; }
    else if (left == 2 && right == 0) g.shape = C_TAIL;
    return g;
}

// EMIT false: bsum[block] = the shaped gaps that end in the block, stat[CS_GAPS ..] += the gaps by shape.  EMIT true: bbase = the exclusive
// scan of bsum; the shaped gaps -> gaps[bbase[block] + rank], n_cand of them in all.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_correct_gaps(const unsigned char* __restrict__ S, u64 nbytes, int k, u64* __restrict__ bsum,
                                                      const u64* __restrict__ bbase, CGap* __restrict__ gaps, u64 n_cand, u64* __restrict__ stat) {
    __shared__ u32 s_wave[4];
    const u64 p0 = (u64)blockIdx.x * C_BLOCK + (u64)threadIdx.x * C_PER;
    u32 s[C_PER + 1];
#pragma unroll
    for (int q = 0; q <= C_PER; ++q) s[q] = 0u;
    if (p0 < nbytes) {                                                           // (S is padded to whole words of 32 positions, zero behind the stream)
        const uint4 v = *reinterpret_cast<const uint4*>(S + p0);
        const u32 w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < C_PER; ++q) s[q] = (w4[q >> 2] >> (8 * (q & 3))) & 0xFFu;
        if (p0 + C_PER < nbytes) s[C_PER] = S[p0 + C_PER];
    }
    u32 ends = 0;
#pragma unroll
    for (int q = 0; q < C_PER; ++q) if (s[q] == 1u && s[q + 1] != 1u) ends |= 1u << q;
    u32 cnt[5] = {0u, 0u, 0u, 0u, 0u};                                           // gaps, interior, head, tail, skipped
    u32 mine = 0;
    CGap found[EMIT ? C_PER / 2 : 1];                                            // (two gap ends are at least two positions apart)
    while (ends) {
        const int q = __builtin_ctz(ends);
        ends &= ends - 1;
        u32 right = 0;
#pragma unroll
        for (int i = 0; i < C_PER; ++i) if (i == q) right = s[i + 1];
        const CGap g = c_classify(S, k, p0 + (u64)q, right);
        ++cnt[0]; ++cnt[1 + g.shape];
        if (g.shape != C_SKIPPED) {
            if constexpr (EMIT) {
#pragma unroll
                for (int i = 0; i < C_PER / 2; ++i) if (i == (int)mine) found[i] = g;
            }
            ++mine;
        }
    }
    const u32 incl = wave_incl_scan(mine);
    if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = incl;
    __syncthreads();
    if constexpr (!EMIT) {
        if (threadIdx.x == 0) bsum[blockIdx.x] = (u64)(s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3]);
        c_block_counts<5>(cnt, stat, CS_GAPS);
    } else {
        u32 excl = incl - mine;
        const u32 wave = threadIdx.x >> 6;
#pragma unroll
        for (u32 w = 0; w < 3; ++w) excl += w < wave ? s_wave[w] : 0u;
        const u64 at = bbase[blockIdx.x] + (u64)excl;
#pragma unroll
        for (int i = 0; i < C_PER / 2; ++i) if (i < (int)mine && at + (u64)i < n_cand) gaps[at + (u64)i] = found[i];
    }
}

// what the trial kernels read: the encoded stream, the index, the bytes in and out (out may be null: a dry run; it may equal in)
struct CTrial { const u64* packed; QTable T; int k; u32 tmin; const unsigned char* in; unsigned char* out; const CGap* gaps; u64 n_cand; };

// the 2-bit code of base e of the encoded stream
__device__ __forceinline__ u32 c_code(const u64* __restrict__ packed, u64 e) { return (u32)(packed[e >> 5] >> (62 - 2 * (int)(e & 31))) & 3u; }

// the canonical value of the window ending at p with code x at base e (p - k < e <= p)
template <int W>
__device__ __forceinline__ KN<W> c_window(const u64* __restrict__ packed, int k, const u64 (&msk)[W], u64 p, u64 e, u32 x) {
    const u64 wi = p >> 5;
    const int tt = (int)(p & 31);
    u64 pw[W + 1];
#pragma unroll
    for (int q = 0; q <= W; ++q) pw[q] = wi >= (u64)q ? packed[wi - q] : 0ull;
    const int d = (int)(p - e), dw = d >> 5, ds = 2 * (d & 31);                  // base e is pair d of the forward value, counted from its low end
    KN<W> f;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        u64 v = tt == 31 ? pw[i] : ((pw[i + 1] << (2 * tt + 2)) | (pw[i] >> (62 - 2 * tt)));
        if (i == dw) v = (v & ~(3ull << ds)) | ((u64)x << ds);
        f.w[i] = v & msk[i];
    }
    return g_min<W>(f, g_revcomp<W>(f, k, msk));
}

// the verdict over the alternatives that work (bit j: code (orig + 1 + j) & 3): one -> the letter is written, in the case of the byte it replaces
__device__ __forceinline__ void c_decide(const CTrial& P, u64 e, u32 orig, u32 works, u32 (&cnt)[3]) {
    const int n = __popc(works);
    if (n == 1) {
        const u32 x = (orig + 1u + (u32)__builtin_ctz(works)) & 3u;
        if (P.out) P.out[e] = (unsigned char)(((0x47544341u >> (8 * x)) & 0xFFu) | (P.in[e] & 0x20u));      // "ACTG"[x]
        ++cnt[0];
    } else if (n > 1) ++cnt[1];
    else ++cnt[2];
}

// A block takes 256 * CAND consecutive candidates, thread t of it the candidates t, t + 256, ...  alive[c] = the alternatives of candidate c
// that k_correct_rest still has to try (0: decided here)
template <int W>
__global__ __launch_bounds__(256) void k_correct_first(CTrial P, unsigned char* __restrict__ alive, u64* __restrict__ stat) {
    constexpr int CAND = CBatch<W>::CAND, N = 3 * CAND;
    const u64 base = (u64)blockIdx.x * (256u * CAND) + threadIdx.x;
    u64 msk[W];
    g_masks<W>(P.k, msk);
    KN<W> c[N];
    u64 e[CAND]; u32 m[CAND], orig[CAND];
    u32 pend = 0;
#pragma unroll
    for (int i = 0; i < CAND; ++i) {
        const u64 ci = base + (u64)i * 256u;
        const bool in = ci < P.n_cand;
        const CGap g = in ? P.gaps[ci] : CGap{0ull, 0ull, 0u, 0u};
        e[i] = g.e; m[i] = g.m;
        orig[i] = in ? c_code(P.packed, g.e) : 0u;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (in) c[3 * i + j] = c_window<W>(P.packed, P.k, msk, g.a, g.e, (orig[i] + 1u + (u32)j) & 3u);
            else {
#pragma unroll
                for (int x = 0; x < W; ++x) c[3 * i + j].w[x] = 0ull;
            }
        }
        if (in) pend |= 7u << (3 * i);
    }
    u32 res[N];
    q_lookup<W, N>(P.T, c, pend, res);
    u32 cnt[3] = {0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < CAND; ++i) {
        const u64 ci = base + (u64)i * 256u;
        if (ci >= P.n_cand) continue;
        u32 surv = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) if (res[3 * i + j] >= P.tmin) surv |= 1u << j;
        if (m[i] == 1u || surv == 0u) { c_decide(P, e[i], orig[i], surv, cnt); surv = 0u; }
        alive[ci] = (unsigned char)surv;
    }
    c_block_counts<3>(cnt, stat, CS_CORRECTED);
}

// Wave w of the grid: the candidates w, w + waves, ...  Lane l tries the windows ending at a + 1 + l and a + 65 + l.
template <int W>
__global__ __launch_bounds__(256) void k_correct_rest(CTrial P, const unsigned char* __restrict__ alive, u64* __restrict__ stat) {
    const u32 lane = threadIdx.x & 63u;
    const u64 waves = (u64)gridDim.x * 4u;
    u64 msk[W];
    g_masks<W>(P.k, msk);
    u32 cnt[3] = {0u, 0u, 0u};
    for (u64 ci = (u64)blockIdx.x * 4u + (threadIdx.x >> 6); ci < P.n_cand; ci += waves) {
        const u32 surv = alive[ci];
        if (surv == 0u) continue;
        const CGap g = P.gaps[ci];
        const u32 orig = c_code(P.packed, g.e);
        const u32 i0 = 1u + lane, i1 = 65u + lane;
        const u32 pend = (i0 < g.m ? 1u : 0u) | (i1 < g.m ? 2u : 0u);
        u32 works = 0;
        for (u32 j = 0; j < 3; ++j) {
            if (!((surv >> j) & 1u)) continue;
            const u32 x = (orig + 1u + j) & 3u;
            KN<W> c[2];
            c[0] = c_window<W>(P.packed, P.k, msk, g.a + (u64)((pend & 1u) ? i0 : 0u), g.e, x);      // (a lane with nothing to try: the window at a, not probed)
            c[1] = c_window<W>(P.packed, P.k, msk, g.a + (u64)((pend & 2u) ? i1 : 0u), g.e, x);
            u32 res[2];
            q_lookup<W, 2>(P.T, c, pend, res);
            const bool fails = ((pend & 1u) && res[0] < P.tmin) || ((pend & 2u) && res[1] < P.tmin);
            if (__ballot(fails) == 0ull) works |= 1u << j;
        }
        if (lane == 0u) c_decide(P, g.e, orig, works, cnt);
    }
    c_block_counts<3>(cnt, stat, CS_CORRECTED);
}

template <int W>
__global__ __launch_bounds__(256) void k_correct_plain(CTrial P, u64* __restrict__ stat) {
    const u64 ci = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 cnt[3] = {0u, 0u, 0u};
    if (ci < P.n_cand) {
        u64 msk[W];
        g_masks<W>(P.k, msk);
        const CGap g = P.gaps[ci];
        const u32 orig = c_code(P.packed, g.e);
        u32 works = 0;
        for (u32 j = 0; j < 3; ++j) {
            bool ok = true;
            for (u32 i = 0; ok && i < g.m; ++i) {
                KN<W> c[1];
                c[0] = c_window<W>(P.packed, P.k, msk, g.a + (u64)i, g.e, (orig + 1u + j) & 3u);
                u32 res[1];
                q_lookup<W, 1>(P.T, c, 1u, res);
                ok = res[0] >= P.tmin;
            }
            if (ok) works |= 1u << j;
        }
        c_decide(P, g.e, orig, works, cnt);
    }
    c_block_counts<3>(cnt, stat, CS_CORRECTED);
}
