// colors.h -- HIP kernels of the sample colours (gfx950 / MI355X, wave64): dskgpu_colors_begin / _colors_add / _colors_rows /
// _colors_unitigs / _colors_pairs / _colors_marks (colors.hip; the definitions are in include/dskgpu.h).
//
// The MATRIX is u32 C[n_rows][n_colors], row-major, in result order: C[r][c] = the valid windows of colour c whose canonical k-mer is row r.
//
//   k_color_reads<W>   the frame of k_query_reads<W>: the N = 16 / W windows of a thread probed as one batch for their ROW NUMBERS
//                      (q_lookup<W, N, true>).  The bank ends travel as a kernel argument (COL_MAX u64); a thread's N positions are
//                      consecutive, so it finds the bank of its first position once and walks on from there.  A position behind the last
//                      end has no bank: its window is taken out of the batch before the probe.  After the probe a lane merges the RUNS of
//                      equal (row, colour) among its N results into one no-return add of the run length (a homopolymer otherwise sends N
//                      adds of one lane to one address; COL_NO_MERGE, an experiment switch, leaves one add per hit: profiles/colors.md).
//                      n_valid / n_placed: combined per block first (col_block_counts), one add each
//   k_color_mask<VEC>  one thread per row: its mask (bit c: C[r][c] >= min_count) and, when asked, the copy of its cells.  VEC: n_colors
//                      is a multiple of 4 and the copy's target is 16-byte aligned: 16-byte loads and stores
//   k_color_fill64     all[u] = the n_colors low bits
//   k_color_unitigs    one thread per row: its non-zero cells onto sum[unitig[r]], its mask into any / all.  Plain 64-bit agent-scope
//                      atomics, as k_unitig_number
//
//
// Comparing the samples: dskgpu_colors_pairs / _colors_marks (dskgpu_colors_load is a device copy).  With C' the THRESHOLDED CELL of the header
// (C[r][c] when >= min_count, else 0; every cell of an unselected row 0), the three pair matrices are sums over the rows of
//   shared[i][j] += C'[i] > 0 && C'[j] > 0      cross[i][j] += C'[j] > 0 ? C'[i] : 0      min_sum[i][j] += min(C'[i], C'[j])
// Accumulators: the cell sums (cross, min_sum) are u64 from the first add on -- a cell may be 2^32 - 1; the row counts (shared, the stats) are
// u32 in a thread and in a block's counters, which is exact because a launch has at most CP_GRID blocks that share the rows out evenly: a
// thread sees fewer than 2^32 rows for any n_rows below 2^51.  Everything wider than a thread is u64.
//
//   k_color_pairs_reg<NC, FULL>   few colours (n_colors <= CP_REG_MAX; bound by reading the matrix): one thread per row, CP_GRID blocks at
//                      the most walk the rows, 16-byte loads when NC is a multiple of 4.  All pairs of the upper triangle in registers
//                      (NC (NC + 1) / 2 counts, as many minima, NC * NC cross sums).  At the end: a butterfly per wave, lane 0 of every wave
//                      adds into the block's LDS copy, then ONE 64-bit agent-scope add per non-zero entry and block, the lower triangle of
//                      shared / min_sum read from the upper one.  The global adds do not grow with n_rows
//   k_color_pairs_tile<FULL>      many colours (bound by arithmetic): a block stages CP_TILE_ROWS rows of thresholded cells in LDS (row stride
//                      = n_colors rounded up to 4, the pad cells 0).  A thread owns a 4 x 4 register block of ORDERED pairs (i-colours x
//                      j-colours): two 16-byte LDS reads feed 16 pairs.  With nb = ceil(n_colors / 4) there are nb * nb such blocks; the 256
//                      threads form 256 / (nb * nb) groups that take the tile's rows in turn.  The accumulators stay in registers across
//                      all the tiles a block walks; at the end they meet in LDS (64-bit LDS adds, one matrix at a time in the tile's
//                      memory), then one global add per non-zero entry and block.  The whole square is computed, not the triangle: with
//                      4 x 4 blocks the 136 blocks of the triangle at 64 colours carry 44 accumulators more per thread and still fill three
//                      of a block's four waves (profiles/color_pairs.md).  A row whose thresholded cells are all 0 is stepped over
//                      (CP_NO_SKIP as a kernel argument leaves that out: the measurement)
//   FULL = false       only `shared` is wanted: no cell sums at all
//   k_color_marks      one thread per row: its mask, the rule, one byte; the kept rows counted per block first
//
// Global atomics: integer adds, ORs and ANDs only; they commute, so nothing that is reported depends on their order.
#pragma once
#include "query.h"

#define COL_MAX 64                        // colours of a matrix, and banks of one call, at the most: a mask is one u64
#define COL_NONE 0xFFFFFFFFu              // the colour of a position behind the last end

enum ColStat { COL_ST_VALID = 0, COL_ST_PLACED, COL_ST_COUNT };

// end[b], b < n: the non-decreasing ends of the call's banks; colour of bank b = first + b
struct ColBanks { u64 end[COL_MAX]; u32 n, first; };

__device__ __forceinline__ void col_add32(u32* at, u32 v) {
    (void)__hip_atomic_fetch_add(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// stat[i] += the sum over the block of mine[i], i < COL_ST_COUNT: LDS first, one add per counter and block that has something (as
// rs_block_counts of readsum.h, which only readsum.hip may include: its kernels are no templates).  Every thread of the block calls it, once
__device__ __forceinline__ void col_block_counts(const u32 (&mine)[COL_ST_COUNT], u64* stat) {
    __shared__ u32 s_cnt[COL_ST_COUNT];
    if (threadIdx.x < COL_ST_COUNT) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < COL_ST_COUNT; ++i) if (mine[i]) atomicAdd(&s_cnt[i], mine[i]);
    __syncthreads();
    if (threadIdx.x < COL_ST_COUNT && s_cnt[threadIdx.x]) q_add64(stat + threadIdx.x, (u64)s_cnt[threadIdx.x]);
}

// Thread t: the N windows ending at bases 32 * (t / TPW) + (t % TPW) * N + j of the encoded stream, as k_query_reads.  t_base: the first
// thread of this launch (a stream of more blocks than one launch takes).  C: n_rows * n_colors cells.  stat[COL_ST_VALID] += the valid
// windows that have a bank, stat[COL_ST_PLACED] += those of them that are rows
template <int W>
__global__ __launch_bounds__(256) void k_color_reads(const u64* __restrict__ packed, const u32* __restrict__ inval, u64 nwords, u64 nbytes, u64 t_base, int k,
                                                     QTable T, ColBanks B, u64 n_rows, u32 n_colors, u32* __restrict__ C, u64* __restrict__ stat) {
    constexpr int N = QBatch<W>::N, TPW = 32 / N;
    const u64 t = t_base + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 wi = t / TPW;
    u32 cnt[COL_ST_COUNT] = {0u, 0u};
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
        // the bank of p0: the least b with p0 < end[b]; the later positions walk on from it (an empty bank is stepped over)
        u32 b = 0;
        while (b < B.n && p0 >= B.end[b]) ++b;
        u64 cur_end = b < B.n ? B.end[b] : 0ull;
        u32 col[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const u64 p = p0 + (u64)j;
            while (b < B.n && p >= cur_end) { ++b; cur_end = b < B.n ? B.end[b] : 0ull; }
            col[j] = b < B.n ? B.first + b : COL_NONE;
            if (col[j] >= n_colors) vm &= ~(1u << j);                                // (no bank; the host side keeps first + n <= n_colors)
        }
        cnt[COL_ST_VALID] = (u32)__popc(vm);
        u32 row[N];
        q_lookup<W, N, true>(T, c, vm, row);
        u32 run = 0, run_row = 0, run_col = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const bool hit = ((vm >> j) & 1u) && (u64)row[j] < n_rows;               // (Q_NO_ROW is above every row number)
            cnt[COL_ST_PLACED] += hit ? 1u : 0u;
#ifdef COL_NO_MERGE
            if (hit) col_add32(C + (u64)row[j] * n_colors + col[j], 1u);
#else
            if (hit && run && row[j] == run_row && col[j] == run_col) { ++run; continue; }
            if (run) col_add32(C + (u64)run_row * n_colors + run_col, run);
            run = hit ? 1u : 0u; run_row = row[j]; run_col = col[j];
#endif
        }
        if (run) col_add32(C + (u64)run_row * n_colors + run_col, run);
    }
    col_block_counts(cnt, stat);
}

// mask[r] (may be null) bit c: C[r][c] >= min_count; counts (may be null) = the copy of C
template <bool VEC>
__global__ __launch_bounds__(256) void k_color_mask(const u32* __restrict__ C, u64 n_rows, u32 n_colors, u32 min_count, u32* __restrict__ counts, u64* __restrict__ mask) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const u64 at = r * n_colors;
    u64 m = 0;
    if constexpr (VEC) {
        for (u32 c = 0; c < n_colors; c += 4) {                                      // (n_colors is a multiple of 4: 16-byte aligned both sides)
            const uint4 v = *reinterpret_cast<const uint4*>(C + at + c);
            if (counts) *reinterpret_cast<uint4*>(counts + at + c) = v;
            m |= (u64)((v.x >= min_count ? 1u : 0u) | (v.y >= min_count ? 2u : 0u) | (v.z >= min_count ? 4u : 0u) | (v.w >= min_count ? 8u : 0u)) << c;
        }
    } else {
        for (u32 c = 0; c < n_colors; ++c) {
            const u32 v = C[at + c];
            if (counts) counts[at + c] = v;
            m |= (u64)(v >= min_count ? 1u : 0u) << c;
        }
    }
    if (mask) mask[r] = m;
}

__global__ __launch_bounds__(256) void k_color_fill64(u64* __restrict__ out, u64 n, u64 value) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = value;
}

// sum[u][c] += C[r][c], any[u] |= mask(r), all[u] &= mask(r) for u = unitig[r]; any of the three may be null.  sum and any start as
// zeros, all as the n_colors low bits
__global__ __launch_bounds__(256) void k_color_unitigs(const u32* __restrict__ C, const u32* __restrict__ unitig, u64 n_rows, u64 n_unitigs, u32 n_colors, u32 min_count,
                                                       u64* __restrict__ sum, u64* __restrict__ all, u64* __restrict__ any) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const u64 u = unitig[r];
    if (u >= n_unitigs) return;                                                      // (a row always has a unitig)
    const u64 at = r * n_colors;
    u64 m = 0;
    for (u32 c = 0; c < n_colors; ++c) {
        const u32 v = C[at + c];
        if (v && sum) q_add64(sum + u * n_colors + c, (u64)v);
        m |= (u64)(v >= min_count ? 1u : 0u) << c;
    }
    if (any && m) (void)__hip_atomic_fetch_or(reinterpret_cast<unsigned long long*>(any + u), (unsigned long long)m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (all) (void)__hip_atomic_fetch_and(reinterpret_cast<unsigned long long*>(all + u), (unsigned long long)m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- comparing the samples: the pair matrices and the row marks
#define CP_BLOCK 256                      // threads of a pair kernel's block
#define CP_GRID 2048                      // blocks of a pair kernel at the most: they walk the rows, so the global adds do not grow with n_rows
#define CP_TILE_ROWS 64                   // rows of a tile of k_color_pairs_tile
#define CP_REG_MAX 8                      // the widest matrix k_color_pairs_reg is built for
#define CP_REG_SWITCH 8                   // n_colors up to which dskgpu_colors_pairs takes k_color_pairs_reg: it measured faster than the tiled kernel at every width it is built for (profiles/color_pairs.md; DSKGPU_PAIRS_REG_MAX)

enum ColPairStat { CP_ST_SELECTED = 0, CP_ST_PRESENT, CP_ST_COUNT };
static_assert((int)CP_ST_COUNT == (int)COL_ST_COUNT,"col_block_counts serves both");

// u64[n_colors][n_colors] each, zeroed before the launch; any may be null.  stat: CP_ST_COUNT counters, zeroed
struct ColPairOut { u64 *shared, *cross, *min_sum, *stat; };

__device__ __forceinline__ u64 cp_shfl_xor64(u64 x, int m) {
    const u32 lo = (u32)__shfl_xor((int)(u32)x, m, 64), hi = (u32)__shfl_xor((int)(u32)(x >> 32), m, 64);
    return ((u64)hi << 32) | lo;
}

// *at (LDS) += the sum of x over the wave.  All 64 lanes call it
__device__ __forceinline__ void cp_wave_add(u64* at, u64 x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += cp_shfl_xor64(x, m);
    if ((threadIdx.x & 63u) == 0 && x) (void)atomicAdd(reinterpret_cast<unsigned long long*>(at), (unsigned long long)x);
}

template <int NC, bool FULL>
__global__ __launch_bounds__(CP_BLOCK) void k_color_pairs_reg(const u32* __restrict__ C, u64 n_rows, u32 min_count, const unsigned char* __restrict__ select, ColPairOut out) {
    constexpr int P = NC * (NC + 1) / 2, NN = NC * NC;
    __shared__ u64 s_acc[3 * NN];                                                    // shared | cross | min_sum; of shared and min_sum the upper triangle
    u32 sh[P];
    u64 mn[P], cr[NN];
#pragma unroll
    for (int p = 0; p < P; ++p) { sh[p] = 0u; mn[p] = 0ull; }
#pragma unroll
    for (int e = 0; e < NN; ++e) cr[e] = 0ull;
    u32 cnt[CP_ST_COUNT] = {0u, 0u};
    for (u64 r = (u64)blockIdx.x * CP_BLOCK + threadIdx.x; r < n_rows; r += (u64)gridDim.x * CP_BLOCK) {
        if (select && !select[r]) continue;
        ++cnt[CP_ST_SELECTED];
        u32 v[NC];
        if constexpr (NC % 4 == 0) {
#pragma unroll
            for (int c = 0; c < NC; c += 4) {
                const uint4 q = *reinterpret_cast<const uint4*>(C + r * NC + c);
                v[c] = q.x; v[c + 1] = q.y; v[c + 2] = q.z; v[c + 3] = q.w;
            }
        } else {
#pragma unroll
            for (int c = 0; c < NC; ++c) v[c] = C[r * NC + c];
        }
        u32 any = 0;
#pragma unroll
        for (int c = 0; c < NC; ++c) { v[c] = v[c] >= min_count ? v[c] : 0u; any |= v[c]; }
        cnt[CP_ST_PRESENT] += any ? 1u : 0u;
        int p = 0;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
#pragma unroll
            for (int j = i; j < NC; ++j, ++p) {
                sh[p] += (v[i] && v[j]) ? 1u : 0u;
                if constexpr (FULL) {
                    if (i == j) cr[i * NC + i] += (u64)v[i];
                    else {
                        mn[p] += (u64)(v[i] < v[j] ? v[i] : v[j]);
                        cr[i * NC + j] += (u64)(v[j] ? v[i] : 0u);
                        cr[j * NC + i] += (u64)(v[i] ? v[j] : 0u);
                    }
                }
            }
        }
    }
    for (u32 t = threadIdx.x; t < 3 * NN; t += CP_BLOCK) s_acc[t] = 0ull;
    __syncthreads();
    {
        int p = 0;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
#pragma unroll
            for (int j = i; j < NC; ++j, ++p) {
                cp_wave_add(&s_acc[i * NC + j], (u64)sh[p]);
                if constexpr (FULL) {
                    if (i == j) { cp_wave_add(&s_acc[NN + i * NC + i], cr[i * NC + i]); }
                    else {
                        cp_wave_add(&s_acc[2 * NN + i * NC + j], mn[p]);
                        cp_wave_add(&s_acc[NN + i * NC + j], cr[i * NC + j]);
                        cp_wave_add(&s_acc[NN + j * NC + i], cr[j * NC + i]);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (u32 t = threadIdx.x; t < 3 * NN; t += CP_BLOCK) {
        const u32 kind = t / NN, e = t % NN, i = e / NC, j = e % NC, lo = i < j ? i : j, hi = i < j ? j : i;
        u64* to = kind == 0 ? out.shared : kind == 1 ? out.cross : out.min_sum;
        if (!to || (!FULL && kind)) continue;
        // min_sum[i][i] == cross[i][i]
        const u64 x = kind == 1 ? s_acc[NN + e] : kind == 2 && i == j ? s_acc[NN + e] : s_acc[kind * NN + lo * NC + hi];
        if (x) q_add64(to + e, x);
    }
    col_block_counts(cnt, out.stat);
}

template <bool FULL>
__global__ __launch_bounds__(CP_BLOCK) void k_color_pairs_tile(const u32* __restrict__ C, u64 n_rows, u32 n_colors, u32 min_count, const unsigned char* __restrict__ select, u32 no_skip,
                                                               ColPairOut out) {
    __shared__ __attribute__((aligned(16))) u64 s_mem[COL_MAX * COL_MAX];           // the tile (u32[CP_TILE_ROWS][ncs]: the first half at the most), then one matrix of sums
    __shared__ u32 s_any[CP_TILE_ROWS];
    static_assert(CP_TILE_ROWS * COL_MAX * 4 <= COL_MAX * COL_MAX * 8, "the tile fits");
    u32* s_tile = reinterpret_cast<u32*>(s_mem);
    const u32 nb = (n_colors + 3) / 4, ncs = nb * 4, T = nb * nb, G = CP_BLOCK / T;  // (nb <= 16: G >= 1)
    const u32 g = threadIdx.x / T, task = threadIdx.x % T, ci = 4 * (task / nb), cj = 4 * (task % nb);
    const bool active = g < G;
    u32 sh[16];
    u64 cr[16], mn[16];
#pragma unroll
    for (int p = 0; p < 16; ++p) { sh[p] = 0u; cr[p] = 0ull; mn[p] = 0ull; }
    u32 cnt[CP_ST_COUNT] = {0u, 0u};
    const u64 n_tiles = (n_rows + CP_TILE_ROWS - 1) / CP_TILE_ROWS;
    for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const u64 r0 = tile * CP_TILE_ROWS;
        const u32 rows = (u32)(n_rows - r0 < CP_TILE_ROWS ? n_rows - r0 : CP_TILE_ROWS);
        __syncthreads();                                                             // the last tile has been read
        if (threadIdx.x < CP_TILE_ROWS) s_any[threadIdx.x] = 0u;
        __syncthreads();
        for (u32 e = threadIdx.x; e < CP_TILE_ROWS * ncs; e += CP_BLOCK) {
            const u32 row = e / ncs, col = e - row * ncs;
            u32 v = 0u;
            if (row < rows && col < n_colors && (!select || select[r0 + row])) {
                v = C[(r0 + row) * n_colors + col];
                v = v >= min_count ? v : 0u;
            }
            s_tile[e] = v;
            if (v) (void)atomicOr(&s_any[row], 1u);
        }
        __syncthreads();
        if (threadIdx.x < rows) {
            cnt[CP_ST_SELECTED] += (!select || select[r0 + threadIdx.x]) ? 1u : 0u;
            cnt[CP_ST_PRESENT] += s_any[threadIdx.x];
        }
        if (active) {
            for (u32 row = g; row < rows; row += G) {
                if (!no_skip && !s_any[row]) continue;
                const uint4 a4 = *reinterpret_cast<const uint4*>(s_tile + row * ncs + ci), b4 = *reinterpret_cast<const uint4*>(s_tile + row * ncs + cj);
                const u32 a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                for (int x = 0; x < 4; ++x) {
#pragma unroll
                    for (int y = 0; y < 4; ++y) {
                        sh[x * 4 + y] += (a[x] && b[y]) ? 1u : 0u;
                        if constexpr (FULL) {
                            cr[x * 4 + y] += (u64)(b[y] ? a[x] : 0u);
                            mn[x * 4 + y] += (u64)(a[x] < b[y] ? a[x] : b[y]);
                        }
                    }
                }
            }
        }
    }
    // one matrix at a time: the block's sums in LDS, then one global add per non-zero entry (the pad colours hold zeros and are not read)
#pragma unroll
    for (int kind = 0; kind < 3; ++kind) {
        u64* to = kind == 0 ? out.shared : kind == 1 ? out.cross : out.min_sum;
        if (!to || (!FULL && kind)) continue;                                        // (uniform over the block)
        __syncthreads();
        for (u32 t = threadIdx.x; t < ncs * ncs; t += CP_BLOCK) s_mem[t] = 0ull;
        __syncthreads();
        if (active) {
#pragma unroll
            for (int x = 0; x < 4; ++x) {
#pragma unroll
                for (int y = 0; y < 4; ++y) {
                    const u64 v = kind == 0 ? (u64)sh[x * 4 + y] : kind == 1 ? cr[x * 4 + y] : mn[x * 4 + y];
                    if (v) (void)atomicAdd(reinterpret_cast<unsigned long long*>(&s_mem[(ci + x) * ncs + cj + y]), (unsigned long long)v);
                }
            }
        }
        __syncthreads();
        for (u32 t = threadIdx.x; t < n_colors * n_colors; t += CP_BLOCK) {
            const u64 v = s_mem[(t / n_colors) * ncs + t % n_colors];
            if (v) q_add64(to + t, v);
        }
    }
    col_block_counts(cnt, out.stat);
}

// the rule of dskgpu_colors_marks (include/dskgpu.h); invert: 0 or 1
struct ColRule { u64 need_all, need_none; u32 min_count, min_present, max_present, invert; };

// keep[r] = the rule on mask(min_count)[r], XOR invert; stat[0] += the rows kept.  Every thread of the block reaches col_block_counts
__global__ __launch_bounds__(256) void k_color_marks(const u32* __restrict__ C, u64 n_rows, u32 n_colors, ColRule R, unsigned char* __restrict__ keep, u64* __restrict__ stat) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 cnt[COL_ST_COUNT] = {0u, 0u};
    if (r < n_rows) {
        const u64 at = r * n_colors;
        u64 m = 0;
        for (u32 c = 0; c < n_colors; ++c) m |= (u64)(C[at + c] >= R.min_count ? 1u : 0u) << c;
        const u32 present = (u32)__popcll(m);
        const bool keep0 = (m & R.need_all) == R.need_all && (m & R.need_none) == 0 && present >= R.min_present && (R.max_present == 0 || present <= R.max_present);
        const u32 k = (keep0 ? 1u : 0u) ^ R.invert;
        keep[r] = (unsigned char)k;
        cnt[0] = k;
    }
    col_block_counts(cnt, stat);
}
