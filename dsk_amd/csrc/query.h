// query.h -- HIP kernels of the lookups in the last result (gfx950 / MI355X, wave64): dskgpu_query_* (query.hip).
//
// The index is ONE open-addressing hash table in HBM over the result rows, whatever their order (global, partition order, unsorted,
// the rows of several passes, a rank's rows):
//
//   slot    : 64 bits = (fingerprint << 32) | row number; all ones = empty (row number 2^32 - 1 is never a row: Q_MAX_ROWS)
//   hash    : h = kmix(k-mer) for one-word keys, the mixed top word of kmixN for two- and four-word keys (kmer_device.h: a 64-bit
//             hash of the WHOLE key); home slot = h & (cap - 1), fingerprint = h >> 32 -- the multiply's high half, the slot bits are
//             its low half folded with the high one
//   probing : linear; cap = power of two >= 2 * rows, so the load is 0.25 .. 0.5
//
// A lookup is two dependent memory levels: the slot, then -- only when the fingerprint matches -- the key words and the abundance of
// that row, which are addressed by the same row number and so travel together.  A binary search over the sorted rows is log2(rows)
// dependent levels.  The kernels are bound by the latency of those random accesses, so every thread works on a BATCH of keys and
// issues the slot loads of the whole batch before it looks at any of them, then the row loads of all candidates; keys that met a
// foreign slot go round again, one slot further, again as a batch.
//
//   k_query_build     one thread per row: hash, claim the first empty slot from the home slot on with a 64-bit compare-and-swap
//   k_query_reads<W>  the canonical k-mer of the window ending at every byte of a 2-bit encoded stream (gen_kmers*) -> abundance or 0
//   k_query_kmers<W>  the same probe for k-mer values in a caller's array
#pragma once
#include "layouts.h"

#define Q_EMPTY 0xFFFFFFFFFFFFFFFFull
#define Q_MAX_ROWS 0xFFFFFFFEull          // row numbers 0 .. 2^32 - 3; 2^32 - 1 belongs to the empty marker
#define Q_MIN_CAP 1024ull

// Keys a thread holds at once: 16 one-word, 8 two-word, 4 four-word (16 words of keys, as a thread of the count path's tiles).  A key in
// flight costs about ten VGPRs (hash, slot, two addresses, row key, abundance, result), so the one-word kernels take ~160 and run 3 waves
// per SIMD: 48 chains per lane slot -- halving the batch (Q_KEYS = 8, an experiment switch) gives 5 waves of 8, fewer chains.
#ifndef Q_KEYS
#define Q_KEYS 16
#endif
template <int W> struct QBatch { static constexpr int N = Q_KEYS / W < 4 ? 4 : Q_KEYS / W; };

struct QTable { const u64* slots; u64 mask; RowsIn rows; const u32* ab; };

// the no-return 64-bit add of the kernels built on this header (thread.h, correct.h): relaxed, agent scope
__device__ __forceinline__ void q_add64(u64* at, u64 v) {
    (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(at), (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int W> __device__ __forceinline__ u64 q_hash(const KN<W>& c) {
    if constexpr (W == 1) return kmix(c.w[0]);
    else return kmix(c.w[W - 1] ^ kfold_low(c));
}

// Rows are distinct k-mers, so an insert never has to compare keys: it takes the first empty slot.  Which row lands in which slot of a
// run depends on the order the threads arrive in; what a lookup returns does not.  (Global atomics: this runs once per result and is
// not on the count path.)
template <int W>
__global__ __launch_bounds__(256) void k_query_build(RowsIn rows, u64 n, u64* __restrict__ slots, u64 mask) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        KN<W> c;
#pragma unroll
        for (int x = 0; x < W; ++x) c.w[x] = rows.w[x][r];
        const u64 h = q_hash<W>(c);
        const u64 val = (h & 0xFFFFFFFF00000000ull) | r;
        u64 s = h & mask;
        for (u64 tries = 0; tries <= mask; ++tries) {       // (bounded: a table that is full would otherwise spin; the host sizes it at <= half full)
            u64 expect = Q_EMPTY;
            if (__hip_atomic_compare_exchange_strong(&slots[s], &expect, val, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
            s = (s + 1) & mask;
        }
    }
}

#define Q_NO_ROW 0xFFFFFFFFu               // q_lookup<W, N, true>: the key is no row

// out[j] = abundance of c[j] for the keys whose bit is set in `pend`, 0 for the others and for keys that are no row.  ROW: the row
// NUMBER instead (unitigs.h), Q_NO_ROW for the others and for keys that are no row; the abundance column is not read then.
template <int W, int N, bool ROW = false>
__device__ __forceinline__ void q_lookup(const QTable& T, const KN<W> (&c)[N], u32 pend, u32 (&out)[N]) {
    u64 h[N];
#pragma unroll
    for (int j = 0; j < N; ++j) { h[j] = q_hash<W>(c[j]); out[j] = ROW ? Q_NO_ROW : 0u; }
    for (u64 d = 0; pend; ++d) {
        u64 v[N];
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = ((pend >> j) & 1u) ? T.slots[(h[j] + d) & T.mask] : Q_EMPTY;      // level 1: the slots of the batch
        u32 cand = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            if (v[j] == Q_EMPTY) pend &= ~(1u << j);                                            // the run ends: not a row
            else if ((u32)(v[j] >> 32) == (u32)(h[j] >> 32)) cand |= 1u << j;
        }
        KN<W> rk[N]; u32 ra[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {                                                           // level 2: key words + abundance of the candidates
            const u32 r = (u32)v[j];
            if ((cand >> j) & 1u) {
#pragma unroll
                for (int x = 0; x < W; ++x) rk[j].w[x] = T.rows.w[x][r];
                if constexpr (ROW) ra[j] = r; else ra[j] = T.ab[r];
            } else {
#pragma unroll
                for (int x = 0; x < W; ++x) rk[j].w[x] = 0ull;
                ra[j] = 0u;
            }
        }
#pragma unroll
        for (int j = 0; j < N; ++j) {
            bool eq;
            if constexpr (W == 1) eq = kmix(rk[j].w[0]) == h[j];                                // (kmix is a bijection: the key itself need not stay in registers)
            else eq = key_eq(rk[j], c[j]);
            if (((cand >> j) & 1u) && eq) { out[j] = ra[j]; pend &= ~(1u << j); }
        }
        if (d > T.mask) break;                                                                  // (a full table: cannot happen at load <= 0.5)
    }
}

// Thread t: the N = 16 / W windows ending at bases 32 * (t / TPW) + (t % TPW) * N + j of the encoded stream; out[p] for every p < nbytes.
// ALIGNED: `out` is 16-byte aligned and a lane's N results leave as 16-byte stores (64 B per lane for one-word keys).
template <int W, bool ALIGNED>
__global__ __launch_bounds__(256) void k_query_reads(const u64* __restrict__ packed, const u32* __restrict__ inval, u64 nwords, u64 nbytes,
                                                     int k, QTable T, u32* __restrict__ out) {
    constexpr int N = QBatch<W>::N, TPW = 32 / N;
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 wi = t / TPW;
    if (wi >= nwords) return;
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
    u32 res[N];
    q_lookup<W, N>(T, c, vm, res);
    const u64 p0 = wi * 32 + (u64)t0;
    if (ALIGNED && p0 + N <= nbytes) {
        uint4* o = reinterpret_cast<uint4*>(out + p0);                   // (p0 is a multiple of N >= 4)
#pragma unroll
        for (int q = 0; q < N / 4; ++q) o[q] = make_uint4(res[4 * q], res[4 * q + 1], res[4 * q + 2], res[4 * q + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) if (p0 + j < nbytes) out[p0 + j] = res[j];
    }
}
// keys[i * ow + x] = word x of value i (ow = ceil(k / 32) words at the ABI; the device key's words above them are zero).  A block takes
// 256 * N consecutive values, thread t of it the values t, t + 256, ...: neighbouring lanes read and write neighbouring addresses.
template <int W>
__global__ __launch_bounds__(256) void k_query_kmers(const u64* __restrict__ keys, u64 n, int ow, QTable T, u32* __restrict__ out) {
    constexpr int N = QBatch<W>::N;
    const u64 base = (u64)blockIdx.x * (256u * N) + threadIdx.x;
    KN<W> c[N];
    u32 pend = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const u64 i = base + (u64)j * 256u;
        const bool in = i < n;
#pragma unroll
        for (int x = 0; x < W; ++x) c[j].w[x] = (in && x < ow) ? keys[i * (u64)ow + x] : 0ull;
        if (in) pend |= 1u << j;
    }
    u32 res[N];
    q_lookup<W, N>(T, c, pend, res);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const u64 i = base + (u64)j * 256u;
        if (i < n) out[i] = res[j];
    }
}
