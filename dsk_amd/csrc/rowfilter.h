// rowfilter.h -- HIP kernels of the row filter that takes flagged rows out of a result (gfx950 / MI355X, wave64): dskgpu_filter_rows and
// the rounds of the graph rules (rowfilter.hip; the definition is in include/dskgpu.h).
//
//   k_tip_rows         per row: bit 1 of its unitig's byte (R_TAKEN of rules.h: the tip, popped or removed bit of whichever rule wrote the
//                      bytes) -> row_tip[r] and / or keep[r] = !bit
//   k_rows_compact<W>  per row with keep[r] != 0: all W words and the abundance to position scan[r] (the exclusive scan of the keep flags)
//   k_filter_offsets   the scan read at the old partition offsets = the new ones; an old offset of n_rows reads as the kept total
//
// No loop on the device depends on the data; every index read from a table is checked against the table it is used on.
#pragma once
#include "layouts.h"

// either output may be null
__global__ __launch_bounds__(256) void k_tip_rows(const u32* __restrict__ unitig, const unsigned char* __restrict__ bits, u64 n, u64 n_unitigs,
                                                  unsigned char* __restrict__ row_tip, unsigned char* __restrict__ keep) {
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const u32 u = unitig[r];
    const u32 tip = (u64)u < n_unitigs ? ((u32)bits[u] >> 1) & 1u : 0u;      // (cannot be: k_unitig_number numbered every row; no index leaves an array)
    if (row_tip) row_tip[r] = (unsigned char)tip;
    if (keep) keep[r] = (unsigned char)(tip ^ 1u);
}

// the keep flag as the scan's input: non-zero = 1
struct TKeepFlag { __host__ __device__ u64 operator()(unsigned char c) const { return c ? 1ull : 0ull; } };

template <int W>
__global__ __launch_bounds__(256) void k_rows_compact(RowsIn rows, const u32* __restrict__ ab, const unsigned char* __restrict__ keep, const u64* __restrict__ scan,
                                                      u64 n, u64 n_kept, RowsOut out, u32* __restrict__ out_ab) {
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r >= n || keep[r] == 0) return;
    u64 x[W];
#pragma unroll
    for (int q = 0; q < W; ++q) x[q] = rows.w[q][r];
    const u32 a = ab[r];
    const u64 d = scan[r];
    if (d >= n_kept) return;                                                  // (cannot be: n_kept is the scan's total; the same guard)
#pragma unroll
    for (int q = 0; q < W; ++q) out.w[q][d] = x[q];
    out_ab[d] = a;
}

// new_off[i] = kept rows before old row old_off[i]; old_off[i] >= n: all the kept rows
__global__ __launch_bounds__(256) void k_filter_offsets(const u64* __restrict__ old_off, u64 n_off, const u64* __restrict__ scan, const unsigned char* __restrict__ keep,
                                                        u64 n, u64* __restrict__ new_off) {
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_off) return;
    const u64 o = old_off[i];
    new_off[i] = o < n ? scan[o] : scan[n - 1] + (keep[n - 1] ? 1ull : 0ull);      // (launched with n > 0 only)
}
