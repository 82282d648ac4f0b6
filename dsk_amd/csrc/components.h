// components.h -- HIP kernels of the connected components of the compacted de Bruijn graph (gfx950 / MI355X, wave64): dskgpu_components* /
// dskgpu_graph_small_components / dskgpu_drop_components (components.hip; the definition is in include/dskgpu.h).
//
// Unitig u has L[u] = offsets[u + 1] - offsets[u] - k rows and the abundance sum S[u]; its oriented readings are U = 2 u + t with the
// targets E(U) = e_targets[e_offsets[U] .. e_offsets[U + 1]) (unitigs.h).  u ~ v when some entry leads from a reading of u to a reading of v;
// every entry is taken in both directions, so nothing here relies on the table being symmetric.
//
//   k_cc_init          parent[u] = u
//   k_cc_hook          the labelling, ONE launch: a lock-free union-find over parent[].  One thread per unitig walks its at most 8 targets; for
//                      each it finds both roots with path halving and hooks the LARGER root under the smaller with a compare-and-swap,
//                      going on from the value the swap returned when it lost.  parent[x] <= x always and a value only ever falls, so the
//                      trees have no cycle, every walk ends, and the root of a finished component is its smallest unitig: the label, whatever
//                      the scheduling.  Every access to parent[] in this launch is a relaxed agent-scope atomic -- the eight L2s of the chip are
//                      not coherent for plain loads inside a launch, and a find that spins on a stale line never ends.  The steps of one
//                      thread are counted against 4 * n_unitigs + 64, which no walk can reach; a thread that does sets CM_BROKEN and stops
//   k_cc_flatten       a launch of its own, so plain loads: label[u] = the root above u
//   k_cc_number        rank = the exclusive scan of (label[u] == u): comp[u] = rank[label[u]], first[rank[u]] = u for the roots
//   k_cc_table<false>  the per-component sums, one add per unitig and column: the yardstick
//   k_cc_table<true>   the same sums combined on chip first.  On real data one component holds nearly every unitig, and a million adds to one
//                      word run at the rate of one address.  Per wave: the component of the first lane that still has one, a ballot of
//                      the lanes that share it, their four sums by a butterfly of cross-lane adds.  The first round's sums of every wave meet
//                      in LDS, where wave 0 adds up those of the block's leading component: one lane issues its four no-return adds, the other
//                      components among the waves' leaders get theirs.  A second round per wave, then whatever lanes are left add for themselves
//   k_cc_stats         per component: CM_SINGLE += (unitigs == 1), CM_MAXU / CM_MAXR = the most unitigs / rows; per block in LDS first
//   k_cc_small         per component: small[c] by the rule; CR_SMALL / CR_UNITIGS / CR_ROWS of the small ones into the round's record
//   k_cc_rows<FLAGS>   per row, through unitig[r] and comp[]: the component (u32) or the small flag of it and / or its complement (u8); four
//                      / sixteen rows per thread, leaving as one 16-byte store where the output is 16-byte aligned
//
// No loop on the device but the union-find's depends on the data; every index read from a table is checked against the table it is used on.
#pragma once
#include "layouts.h"

#define C_NONE 0xFFFFFFFFu                 // no component, no unitig
#define CC_BLOCK 1024                       // threads of a k_cc_table block: 16 waves meet in LDS
#define CC_WAVES (CC_BLOCK / 64)

enum CompStat { CM_BROKEN = 0, CM_SINGLE, CM_MAXU, CM_MAXR, CM_COUNT };
enum CRec { CR_SMALL = 0, CR_UNITIGS, CR_ROWS, CR_SPARE, CR_COUNT };
enum CCol { CC_UNITIGS = 0, CC_ROWS, CC_AB, CC_EDGES, CC_COUNT };      // the columns of the table: cols[col * n_c + c]

#define C_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__global__ __launch_bounds__(256) void k_cc_init(u32* __restrict__ parent, u64 n_unitigs) {
    const u64 u = (u64)blockIdx.x * 256u + threadIdx.x;
    if (u < n_unitigs) parent[u] = (u32)u;
}

// the root above x; halves the path on the way.  steps: the thread's budget, 0 = spent
__device__ __forceinline__ u32 cc_find(u32* parent, u32 x, u64& steps) {
    for (;;) {
        const u32 p = __hip_atomic_load(&parent[x], C_RLX);
        if (p == x || steps == 0) return x;
        --steps;
        const u32 g = __hip_atomic_load(&parent[p], C_RLX);
        if (g == p) return p;
        u32 expect = p;
        (void)__hip_atomic_compare_exchange_strong(&parent[x], &expect, g, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (lost: somebody put x lower still)
        x = g;
    }
}

__device__ __forceinline__ void cc_unite(u32* parent, u32 a, u32 b, u64& steps) {
    for (;;) {
        a = cc_find(parent, a, steps);
        b = cc_find(parent, b, steps);
        if (a == b || steps == 0) return;
        if (a < b) { const u32 t = a; a = b; b = t; }                          // a: the larger root, goes under b
        u32 expect = a;
        if (__hip_atomic_compare_exchange_strong(&parent[a], &expect, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        --steps;
        a = expect;                                                            // a was hooked meanwhile: on from where it hangs now
    }
}

__global__ __launch_bounds__(256) void k_cc_hook(const u64* __restrict__ e_offsets, const u32* __restrict__ e_targets, u64 n_unitigs, u64 n_edges,
                                                 u32* parent, u64* __restrict__ stat) {
    const u64 u = (u64)blockIdx.x * 256u + threadIdx.x;
    if (u >= n_unitigs) return;
    const u64 e0 = e_offsets[2 * u], e2 = e_offsets[2 * u + 2];
    const u32 d = (u32)min(e2 - e0, 8ull);                                     // (two readings of at most 4 targets each)
    u32 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = ((u32)i < d && e0 + i < n_edges) ? e_targets[e0 + i] >> 1 : C_NONE;
    u64 steps = 4 * n_unitigs + 64;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (v[i] == C_NONE || (u64)v[i] >= n_unitigs || (u64)v[i] == u) continue;      // self edges join nothing
        cc_unite(parent, (u32)u, v[i], steps);
    }
    if (steps == 0) atomicAdd(reinterpret_cast<unsigned long long*>(&stat[CM_BROKEN]), 1ull);
}

__global__ __launch_bounds__(256) void k_cc_flatten(const u32* __restrict__ parent, u64 n_unitigs, u32* __restrict__ label, u64* __restrict__ stat) {
    const u64 u = (u64)blockIdx.x * 256u + threadIdx.x;
    if (u >= n_unitigs) return;
    u32 x = (u32)u;
    bool broken = false;
    for (;;) {
        const u32 p = parent[x];
        if (p == x) break;
        if (p > x) { broken = true; break; }                                   // (cannot be: a parent is never above its child; and so the walk ends)
        x = p;
    }
    label[u] = x;
    if (broken) atomicAdd(reinterpret_cast<unsigned long long*>(&stat[CM_BROKEN]), 1ull);
}

// the root flag as the scan's input
struct CRootFlag {
    const u32* label;
    __host__ __device__ u32 operator()(u32 u) const { return label[u] == u ? 1u : 0u; }
};

__global__ __launch_bounds__(256) void k_cc_number(const u32* __restrict__ label, const u32* __restrict__ rank, u64 n_unitigs, u64 n_c,
                                                   u32* __restrict__ comp, u32* __restrict__ first) {
    const u64 u = (u64)blockIdx.x * 256u + threadIdx.x;
    if (u >= n_unitigs) return;
    const u32 l = label[u];
    const u32 c = (u64)l < n_unitigs ? rank[l] : C_NONE;
    comp[u] = c;
    if ((u64)l == u && (u64)c < n_c) first[c] = (u32)u;
}

__device__ __forceinline__ void cc_add(u64* p, u64 v) { (void)__hip_atomic_fetch_add(p, v, C_RLX); }      // (result unused: the no-return form)

__device__ __forceinline__ void cc_add_all(u64* __restrict__ cols, u64 n_c, u32 c, u64 cnt, u64 rows, u64 ab, u64 edges) {
    cc_add(cols + CC_UNITIGS * n_c + c, cnt); cc_add(cols + CC_ROWS * n_c + c, rows); cc_add(cols + CC_AB * n_c + c, ab); cc_add(cols + CC_EDGES * n_c + c, edges);
}

__device__ __forceinline__ u64 cc_shfl_xor64(u64 x, int m) {
    const u32 lo = (u32)__shfl_xor((int)(u32)x, m, 64), hi = (u32)__shfl_xor((int)(u32)(x >> 32), m, 64);
    return ((u64)hi << 32) | lo;
}

// the sums over the wave of what the lanes with `mine` hold; every lane gets them.  All 64 lanes call it
__device__ __forceinline__ void cc_wave_sums(bool mine, u64& rows, u64& ab, u32& edges) {
    rows = mine ? rows : 0ull; ab = mine ? ab : 0ull; edges = mine ? edges : 0u;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        rows += cc_shfl_xor64(rows, m); ab += cc_shfl_xor64(ab, m); edges += (u32)__shfl_xor((int)edges, m, 64);
    }
}

template <bool COMBINE>
__global__ __launch_bounds__(CC_BLOCK) void k_cc_table(const u32* __restrict__ comp, const u64* __restrict__ offsets, const u64* __restrict__ ab_sum,
                                                      const u64* __restrict__ e_offsets, u64 n_unitigs, int k, u64 n_c, u64* __restrict__ cols) {
    const u64 u = (u64)blockIdx.x * CC_BLOCK + threadIdx.x;
    u32 c = C_NONE; u64 L = 0, S = 0; u32 E = 0;
    if (u < n_unitigs) {
        c = comp[u];
        L = offsets[u + 1] - offsets[u] - (u64)k; S = ab_sum[u]; E = (u32)min(e_offsets[2 * u + 2] - e_offsets[2 * u], 8ull);
    }
    bool have = (u64)c < n_c;                                                  // (always, for a unitig: k_cc_number numbered it; no index leaves the table)
    if (!COMBINE) {
        if (have) cc_add_all(cols, n_c, c, 1ull, L, S, (u64)E);
        return;
    }
    __shared__ u32 s_key[CC_WAVES], s_cnt[CC_WAVES], s_edges[CC_WAVES];
    __shared__ u64 s_rows[CC_WAVES], s_ab[CC_WAVES];
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // round 1: the component of the wave's first lane; its sums go to LDS
    {
        const u64 left = __ballot(have);
        const int leader = left ? __ffsll((unsigned long long)left) - 1 : 0;
        const u32 key = left ? (u32)__shfl((int)c, leader, 64) : C_NONE;
        const bool mine = have && c == key;
        const u32 cnt = (u32)__popcll(__ballot(mine));
        u64 r = L, a = S; u32 e = E;
        cc_wave_sums(mine, r, a, e);
        if (lane == 0) { s_key[wave] = key; s_cnt[wave] = cnt; s_rows[wave] = r; s_ab[wave] = a; s_edges[wave] = e; }
        have = have && !mine;
    }
    __syncthreads();
    if (wave == 0) {                                                           // the waves' leaders: those of the block's leading component as one
        const bool in = lane < CC_WAVES;
        const u32 key = in ? s_key[lane] : C_NONE, lead = s_key[0];
        const bool mine = key != C_NONE && key == lead;
        u64 r = in ? s_rows[lane] : 0ull, a = in ? s_ab[lane] : 0ull; u32 e = in ? s_edges[lane] : 0u, n = in ? s_cnt[lane] : 0u;
        const u64 r1 = r, a1 = a; const u32 e1 = e, n1 = n;
        cc_wave_sums(mine, r, a, e);
        u64 nn = mine ? (u64)n : 0ull, unused = 0; u32 unused32 = 0;
        cc_wave_sums(true, nn, unused, unused32);
        if (lane == 0 && lead != C_NONE) cc_add_all(cols, n_c, lead, nn, r, a, (u64)e);
        if (key != C_NONE && !mine) cc_add_all(cols, n_c, key, (u64)n1, r1, a1, (u64)e1);
    }
    // round 2 per wave, then every lane that is left for itself
    {
        const u64 left = __ballot(have);
        if (left) {
            const int leader = __ffsll((unsigned long long)left) - 1;
            const u32 key = (u32)__shfl((int)c, leader, 64);
            const bool mine = have && c == key;
            const u32 cnt = (u32)__popcll(__ballot(mine));
            u64 r = L, a = S; u32 e = E;
            cc_wave_sums(mine, r, a, e);
            if ((int)lane == leader) cc_add_all(cols, n_c, key, (u64)cnt, r, a, (u64)e);
            have = have && !mine;
        }
    }
    if (have) cc_add_all(cols, n_c, c, 1ull, L, S, (u64)E);
}

__global__ __launch_bounds__(256) void k_cc_stats(const u64* __restrict__ cols, u64 n_c, u64* __restrict__ stat) {
    __shared__ unsigned long long s_single, s_maxu, s_maxr;
    if (threadIdx.x == 0) { s_single = 0; s_maxu = 0; s_maxr = 0; }
    __syncthreads();
    const u64 c = (u64)blockIdx.x * 256u + threadIdx.x;
    if (c < n_c) {
        const u64 nu = cols[CC_UNITIGS * n_c + c], nr = cols[CC_ROWS * n_c + c];
        if (nu == 1) atomicAdd(&s_single, 1ull);
        atomicMax(&s_maxu, (unsigned long long)nu); atomicMax(&s_maxr, (unsigned long long)nr);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_single) atomicAdd(reinterpret_cast<unsigned long long*>(&stat[CM_SINGLE]), s_single);
        atomicMax(reinterpret_cast<unsigned long long*>(&stat[CM_MAXU]), s_maxu); atomicMax(reinterpret_cast<unsigned long long*>(&stat[CM_MAXR]), s_maxr);
    }
}

// small[c] <=> rows[c] < min_rows and (max_abundance == 0 or ab_sum[c] <= max_abundance * rows[c]); rows[c] < 2^31 keeps the product in 64 bits
__global__ __launch_bounds__(256) void k_cc_small(const u64* __restrict__ cols, u64 n_c, u32 min_rows, u32 max_abundance, unsigned char* __restrict__ small,
                                                  u64* __restrict__ rec) {
    __shared__ unsigned long long s_rec[CR_COUNT];
    if (threadIdx.x < CR_COUNT) s_rec[threadIdx.x] = 0;
    __syncthreads();
    const u64 c = (u64)blockIdx.x * 256u + threadIdx.x;
    if (c < n_c) {
        const u64 nu = cols[CC_UNITIGS * n_c + c], nr = cols[CC_ROWS * n_c + c], ab = cols[CC_AB * n_c + c];
        const bool sm = nr < (u64)min_rows && (max_abundance == 0u || ab <= (u64)max_abundance * nr);
        small[c] = sm ? 1 : 0;
        if (sm) { atomicAdd(&s_rec[CR_SMALL], 1ull); atomicAdd(&s_rec[CR_UNITIGS], (unsigned long long)nu); atomicAdd(&s_rec[CR_ROWS], (unsigned long long)nr); }
    }
    __syncthreads();
    if (threadIdx.x < CR_COUNT && s_rec[threadIdx.x]) atomicAdd(reinterpret_cast<unsigned long long*>(&rec[threadIdx.x]), s_rec[threadIdx.x]);
}

// per row.  FLAGS false: row_comp[r] = comp[unitig[r]], 4 rows per thread.  FLAGS true: row_drop[r] = small[comp[unitig[r]]] and / or keep[r] = its
// complement, 16 rows per thread (either may be null).  A thread's results leave as one 16-byte store when the output is 16-byte aligned
// and the rows are all there, else one by one
template <bool FLAGS>
__global__ __launch_bounds__(256) void k_cc_rows(const u32* __restrict__ unitig, const u32* __restrict__ comp, const unsigned char* __restrict__ small, u64 n, u64 n_unitigs,
                                                 u64 n_c, u32* __restrict__ row_comp, unsigned char* __restrict__ row_drop, unsigned char* __restrict__ keep) {
    constexpr int PER = FLAGS ? 16 : 4;
    const u64 r0 = ((u64)blockIdx.x * 256u + threadIdx.x) * PER;
    if (r0 >= n) return;
    const bool whole = r0 + PER <= n;
    u32 un[PER], cc[PER];
    if (whole) {                                                               // (unitig: an array of the library's own, 16-byte aligned; r0 a multiple of 4)
#pragma unroll
        for (int q = 0; q < PER / 4; ++q) {
            const uint4 x = reinterpret_cast<const uint4*>(unitig + r0)[q];
            un[4 * q] = x.x; un[4 * q + 1] = x.y; un[4 * q + 2] = x.z; un[4 * q + 3] = x.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < PER; ++i) un[i] = r0 + i < n ? unitig[r0 + i] : C_NONE;
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) cc[i] = (u64)un[i] < n_unitigs ? comp[un[i]] : C_NONE;
    if (!FLAGS) {
        if (whole && (reinterpret_cast<uintptr_t>(row_comp) & 15u) == 0) {
            *reinterpret_cast<uint4*>(row_comp + r0) = make_uint4(cc[0], cc[1], cc[2], cc[3]);
        } else {
#pragma unroll
            for (int i = 0; i < PER; ++i) if (r0 + i < n) row_comp[r0 + i] = cc[i];
        }
        return;
    }
    u32 f[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) f[i] = (u64)cc[i] < n_c ? (u32)small[cc[i]] & 1u : 0u;
    u32 w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < PER; ++i) w[i >> 2] |= f[i] << (8 * (i & 3));
    if (row_drop) {
        if (whole && (reinterpret_cast<uintptr_t>(row_drop) & 15u) == 0) {
            *reinterpret_cast<uint4*>(row_drop + r0) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int i = 0; i < PER; ++i) if (r0 + i < n) row_drop[r0 + i] = (unsigned char)f[i];
        }
    }
    if (keep) {
        if (whole && (reinterpret_cast<uintptr_t>(keep) & 15u) == 0) {
            *reinterpret_cast<uint4*>(keep + r0) = make_uint4(w[0] ^ 0x01010101u, w[1] ^ 0x01010101u, w[2] ^ 0x01010101u, w[3] ^ 0x01010101u);
        } else {
#pragma unroll
            for (int i = 0; i < PER; ++i) if (r0 + i < n) keep[r0 + i] = (unsigned char)(f[i] ^ 1u);
        }
    }
}
