// loadrows.h -- HIP kernels of dskgpu_load_rows (loadrows.hip; gfx950 / MI355X, wave64): (k-mer, abundance) pairs become a result.
//
//   k_load_check<W>     one pass over the caller's row-major input: every value below 4^k, canonical (g_revcomp / g_min of graph.h),
//                       abundance >= 1 -- the lowest offending index by one atomicMin of the lanes that found something --, the exact 64-bit
//                       sum of the abundances (per wave, per block, one add per block), "some row is not above its predecessor" (one flag
//                       per block), and the transposition into the per-word arrays the row order takes
//   k_load_heads<W>     the ordered rows: 1 where a row differs from its predecessor (the scan of these flags numbers the distinct values)
//   k_load_combine<W,M> SUM / MAX / MIN of the abundances of equal rows into one 64-bit accumulator per distinct value.  A thread takes
//                       LR_RPT consecutive rows and merges its own equal ones in registers; a run that lies inside the thread's rows is
//                       stored, a run that crosses into a neighbour's rows goes out as ONE no-return agent-scope atomic per (thread, value);
//                       a wave whose 64 x LR_RPT rows all hold one value combines across the lanes first and sends one atomic.  No loop is
//                       as long as a run: 10^6 equal rows are 10^6 / 256 atomics on one address
//   k_load_finish       the distinct values: saturate, bin min(v, histo_max) (LDS per block, one add per non-empty bin and block), apply the
//                       abundance filter -> keep flags + the three counters
//   k_load_compact<W>   the kept values to their places (the scan of the keep flags)
//   k_load_first<W> / k_load_repeat<W>   DSKGPU_LOAD_UNIQUE met a repeat (error path): the lowest input index whose value also stands at a
//                       lower index, by bisection of every input value in the ordered rows
#pragma once
#include "graph.h"

#define LR_BLOCK 256
#define LR_RPT 4                          // consecutive ordered rows of a thread in k_load_combine
#define LR_HIST_LDS 12288u                // histogram bins a block keeps in LDS (48 KB); bins above go to the global histogram one by one
enum { LR_BAD = 0, LR_KMERS, LR_DESC, LR_BELOW, LR_ABOVE, LR_SAT, LR_REPEAT, LR_COUNT = 8 };      // the record of a load (u64 each)
enum { LR_M_SUM = 0, LR_M_MAX = 1, LR_M_MIN = 2 };

__device__ __forceinline__ u64 lr_shfl_xor64(u64 x, int m) {
    const u32 lo = (u32)__shfl_xor((int)(u32)x, m, 64), hi = (u32)__shfl_xor((int)(u32)(x >> 32), m, 64);
    return ((u64)hi << 32) | lo;
}
template <int M> __device__ __forceinline__ u64 lr_op(u64 a, u64 b) { return M == LR_M_SUM ? a + b : M == LR_M_MAX ? (a > b ? a : b) : (a < b ? a : b); }
template <int M> __device__ __forceinline__ void lr_atomic(u64* p, u64 v) {      // (results unused: the no-return forms)
    if constexpr (M == LR_M_SUM) (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if constexpr (M == LR_M_MAX) (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <int W> __device__ __forceinline__ KN<W> lr_input(const u64* __restrict__ in, u64 i, int ow) {      // value i of the row-major input (ow words; the rest zero)
    KN<W> x;
#pragma unroll
    for (int j = 0; j < W; ++j) x.w[j] = j < ow ? in[i * (u64)ow + j] : 0ull;
    return x;
}
template <int W> __device__ __forceinline__ KN<W> lr_row(const RowsIn& r, u64 i) {
    KN<W> x;
#pragma unroll
    for (int j = 0; j < W; ++j) x.w[j] = r.w[j][i];
    return x;
}
template <int W> __device__ __forceinline__ bool lr_eq(const KN<W>& a, const KN<W>& b) {
    bool e = true;
#pragma unroll
    for (int j = 0; j < W; ++j) e = e && a.w[j] == b.w[j];
    return e;
}
template <int W> __device__ __forceinline__ bool lr_less(const KN<W>& a, const KN<W>& b) {      // a < b, most significant word first
    bool lt = false, decided = false;
#pragma unroll
    for (int j = W - 1; j >= 0; --j) { if (!decided && a.w[j] != b.w[j]) { lt = a.w[j] < b.w[j]; decided = true; } }
    return lt;
}

__global__ void k_load_set(u32* __restrict__ p, u32 v) { if (threadIdx.x == 0) *p = v; }      // a scan's length from a kernel argument (as k_set_rs_scalars)

template <int W>
__global__ __launch_bounds__(LR_BLOCK) void k_load_check(const u64* __restrict__ in, const u32* __restrict__ ab, u64 n, int ow, int k, RowsOut out,
                                                         u32* __restrict__ out_ab, u64* __restrict__ rec) {
    __shared__ u64 s_sum[LR_BLOCK / 64];
    u64 msk[W];
    g_masks<W>(k, msk);
    u64 sum = 0; bool desc = false;
    for (u64 i = (u64)blockIdx.x * LR_BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * LR_BLOCK) {
        const KN<W> x = lr_input<W>(in, i, ow);
        const u32 a = ab[i];
        if (i > 0) { const KN<W> p = lr_input<W>(in, i - 1, ow); desc = desc || !lr_less<W>(p, x); }
        bool bad = a == 0u;
#pragma unroll
        for (int j = 0; j < W; ++j) bad = bad || (x.w[j] & ~msk[j]) != 0ull;
        bad = bad || !lr_eq<W>(g_min<W>(x, g_revcomp<W>(x, k, msk)), x);
        if (bad) (void)atomicMin(rec + LR_BAD, i);
#pragma unroll
        for (int j = 0; j < W; ++j) out.w[j][i] = x.w[j];
        out_ab[i] = a;
        sum += a;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sum += lr_shfl_xor64(sum, m);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum;
    const int any_desc = __syncthreads_or(desc ? 1 : 0);
    if (threadIdx.x == 0) {
        u64 t = 0;
        for (int w = 0; w < LR_BLOCK / 64; ++w) t += s_sum[w];
        if (t) lr_atomic<LR_M_SUM>(rec + LR_KMERS, t);
        if (any_desc) rec[LR_DESC] = 1ull;
    }
}

template <int W>
__global__ __launch_bounds__(LR_BLOCK) void k_load_heads(RowsIn rows, u64 n, u32* __restrict__ head) {
    const u64 i = (u64)blockIdx.x * LR_BLOCK + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0 || !lr_eq<W>(lr_row<W>(rows, i), lr_row<W>(rows, i - 1))) ? 1u : 0u;
}

// pos = the exclusive scan of the head flags (n + 1 entries): row i is a head when pos[i + 1] != pos[i], and its value is distinct value pos[i + 1] - 1
template <int W, int M>
__global__ __launch_bounds__(LR_BLOCK) void k_load_combine(RowsIn rows, const u32* __restrict__ ab, u64 n, const u32* __restrict__ pos, RowsOut dk,
                                                           u64* __restrict__ acc) {
    const u64 i0 = ((u64)blockIdx.x * LR_BLOCK + threadIdx.x) * LR_RPT;
    u32 p[LR_RPT + 2];
#pragma unroll
    for (int j = 0; j < LR_RPT + 2; ++j) { const u64 i = i0 + j; p[j] = pos[i < n ? i : n]; }
    const bool full = i0 + LR_RPT <= n;
    u32 cur_d = 0; u64 cur_v = 0; bool open = false, cur_head = false, single = true;
#pragma unroll
    for (int j = 0; j < LR_RPT; ++j) {
        const u64 i = i0 + j;
        if (i < n) {
            const bool head = p[j + 1] != p[j];
            const u32 d = p[j + 1] - 1u;
            const u64 a = ab[i];
            if (head) {
#pragma unroll
                for (int x = 0; x < W; ++x) dk.w[x][d] = rows.w[x][i];
            }
            if (open && d == cur_d) cur_v = lr_op<M>(cur_v, a);
            else {
                if (open) {      // the run before this one ends inside my rows: stored when it began there too
                    if (cur_head) acc[cur_d] = cur_v; else lr_atomic<M>(acc + cur_d, cur_v);
                    single = false;
                }
                cur_d = d; cur_v = a; cur_head = head; open = true;
            }
        }
    }
    // my last run: complete when it began in my rows and the row behind them is a head (or there is none)
    const bool closed = i0 + LR_RPT >= n || p[LR_RPT + 1] != p[LR_RPT];
    // a wave whose rows all hold one value: one atomic for the wave
    const bool uniform = __all(full && single) && (u32)__shfl((int)cur_d, 0, 64) == (u32)__shfl((int)cur_d, 63, 64);
    if (uniform) {
        u64 v = cur_v;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v = lr_op<M>(v, lr_shfl_xor64(v, m));
        if ((threadIdx.x & 63) == 0) lr_atomic<M>(acc + cur_d, v);
    } else if (open) {
        if (cur_head && closed) acc[cur_d] = cur_v; else lr_atomic<M>(acc + cur_d, cur_v);
    }
}

// v[d] = the combined abundance of distinct value d: acc (64 bits) when rows were combined, else the abundances themselves
template <bool ACC>
__device__ __forceinline__ u32 lr_value(const u64* __restrict__ acc, const u32* __restrict__ ab, u64 d, bool* sat) {
    if constexpr (ACC) { const u64 v = acc[d]; *sat = v > 0xFFFFFFFFull; return *sat ? 0xFFFFFFFFu : (u32)v; }
    else { *sat = false; return ab[d]; }
}

template <bool ACC>
__global__ __launch_bounds__(LR_BLOCK) void k_load_finish(const u64* __restrict__ acc, const u32* __restrict__ ab, u64 nd, u32 amin, u32 amax, u32 histo_max,
                                                          u32 nl, u64* __restrict__ ghist, u32* __restrict__ keep, u64* __restrict__ rec) {
    extern __shared__ u32 lh[];             // nl bins, then below / above / saturated
    for (u32 b = threadIdx.x; b < nl + 3; b += LR_BLOCK) lh[b] = 0u;
    __syncthreads();
    for (u64 d = (u64)blockIdx.x * LR_BLOCK + threadIdx.x; d < nd; d += (u64)gridDim.x * LR_BLOCK) {
        bool sat;
        const u32 c = lr_value<ACC>(acc, ab, d, &sat);
        const u32 b = c < histo_max ? c : histo_max;
        if (b < nl) atomicAdd(&lh[b], 1u); else (void)atomicAdd(ghist + b, 1ull);
        const bool below = c < amin, above = c > amax;
        if (below) atomicAdd(&lh[nl], 1u);
        if (above) atomicAdd(&lh[nl + 1], 1u);
        if (sat) atomicAdd(&lh[nl + 2], 1u);
        keep[d] = (below || above) ? 0u : 1u;
    }
    __syncthreads();
    for (u32 b = threadIdx.x; b < nl; b += LR_BLOCK) if (lh[b]) (void)atomicAdd(ghist + b, (u64)lh[b]);
    if (threadIdx.x < 3 && lh[nl + threadIdx.x]) (void)atomicAdd(rec + LR_BELOW + threadIdx.x, (u64)lh[nl + threadIdx.x]);
}

// kpos = the exclusive scan of the keep flags (nd + 1 entries)
template <int W, bool ACC>
__global__ __launch_bounds__(LR_BLOCK) void k_load_compact(RowsIn dk, const u64* __restrict__ acc, const u32* __restrict__ ab, u64 nd, const u32* __restrict__ kpos,
                                                           RowsOut out, u32* __restrict__ out_ab) {
    const u64 d = (u64)blockIdx.x * LR_BLOCK + threadIdx.x;
    if (d >= nd) return;
    const u32 at = kpos[d];
    if (kpos[d + 1] == at) return;
    bool sat;
    const u32 c = lr_value<ACC>(acc, ab, d, &sat);
#pragma unroll
    for (int x = 0; x < W; ++x) out.w[x][at] = dk.w[x][d];
    out_ab[at] = c;
}

// the first ordered row that is not below x (x is a row: it is found)
template <int W> __device__ __forceinline__ u64 lr_lower_bound(const RowsIn& rows, u64 n, const KN<W>& x) {
    u64 lo = 0, hi = n;
    while (lo < hi) { const u64 mid = lo + ((hi - lo) >> 1); if (lr_less<W>(lr_row<W>(rows, mid), x)) lo = mid + 1; else hi = mid; }
    return lo;
}
template <int W>
__global__ __launch_bounds__(LR_BLOCK) void k_load_first(const u64* __restrict__ in, u64 n, int ow, RowsIn rows, u32* __restrict__ first) {
    const u64 i = (u64)blockIdx.x * LR_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u64 at = lr_lower_bound<W>(rows, n, lr_input<W>(in, i, ow));
    if (at < n) (void)atomicMin(first + at, (u32)i);
}
template <int W>
__global__ __launch_bounds__(LR_BLOCK) void k_load_repeat(const u64* __restrict__ in, u64 n, int ow, RowsIn rows, const u32* __restrict__ first, u64* __restrict__ rec) {
    const u64 i = (u64)blockIdx.x * LR_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u64 at = lr_lower_bound<W>(rows, n, lr_input<W>(in, i, ow));
    if (at < n && first[at] != (u32)i) (void)atomicMin(rec + LR_REPEAT, i);
}
