// layouts.h -- what the kernel headers (kernels.h, superkmer.h, rowsort.h, rowsort2.h, partsort.h) and the host (engine.h)
// share: the chunk descriptors of the key scatters, the super-k-mer sender's parameters, the layouts of the solid rows, the
// LDS-only barrier and tile scan of the LDS-staged scatters, and the index gather that the row sort and the bank merge both
// launch.  No other kernel here: each host translation unit defines its own (dskgpu.hip the count path, sender.hip the record sender, rowsort.hip the row
// sort), and a non-template kernel that both included would be defined twice.
#pragma once
#include "kmer_device.h"

// Workgroup barrier that orders LDS traffic only.  HIP's __syncthreads() also
// drains every outstanding global load (s_waitcnt vmcnt(0)), which would kill
// the register prefetch of the next tile / sub-partition; this one waits for
// LDS (lgkmcnt) and leaves HBM reads in flight across the barrier
// (cdna_hip_programming.md "Pipelining across barriers").  Global data is never
// exchanged between threads inside these kernels, so no vmcnt wait is needed.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Exclusive scan of cnt[0..P) fused with the cursor bookkeeping of the tile:
//   off[b]   = start of bin b inside the staged tile
//   delta[b] = cur[b] - off[b]   (HBM index of staged element i of bin b is delta[b] + i)
//   cur[b]  += cnt[b];  cnt[b] = 0
// sg.lim (block-owned slices): bin b may only be written below lim[b], the end of the block's slice of that bin; a bin whose keys
// of this tile would not fit is redirected, for this tile, to the dump zone [dump, dump + tile) behind the last slice (never read) -- the
// check costs a few instructions per BIN and tile instead of per key, and nothing is ever written outside the block's own
// slices or the dump zone.  The cursor of such a bin is parked at end + 1, so the overflow shows at the end of the launch.
struct SliceGuard { const u32* lim; u32 dump; u32 uslice, first; };      // lim[b] (LDS): end of the block's slice of bin b; or uniform slices of uslice keys from `first` (no array); neither = no guard
template <int NT>
__device__ __forceinline__ void tile_scan(u32* cnt, u32* off, u32* delta, u32* cur, int P, u32* wsum, u32* tot, SliceGuard sg = SliceGuard{nullptr, 0u, 0u, 0u}) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ipt = (P + NT - 1) / NT;
    const int base = tid * ipt;
    u32 v[4]; u32 s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int idx = base + j;
        v[j] = (j < ipt && idx < P) ? cnt[idx] : 0u;
        s += v[j];
    }
    const u32 inc = wave_incl_scan(s);
    if (lane == 63) wsum[wave] = inc;
    lds_barrier();
    if (wave == 0) {
        const u32 x = lane < NT / 64 ? wsum[lane] : 0u;
        const u32 y = wave_incl_scan(x);
        if (lane < NT / 64) wsum[lane] = y - x;
        if (lane == NT / 64 - 1) { *tot = y; off[P] = y; }        // off[P]: the dummy bin (invalid windows) is staged behind the keys
    }
    lds_barrier();
    u32 run = wsum[wave] + inc - s;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int idx = base + j;
        if (j < ipt && idx < P) {
            const u32 c = cur[idx];
            // (a cursor that left its slice stays at end + 1: it marks the overflow for the end of the launch and cannot wrap 2^32
            //  however many keys the bin still receives; below the end, c + v <= 0xFFFF0000 + a tile)
            const u32 end = sg.lim ? sg.lim[idx] : sg.uslice ? sg.first + (u32)(idx + 1) * sg.uslice : 0xFFFFFFFFu;
            const bool fits = (sg.lim || sg.uslice) ? c + v[j] <= end : true;
            off[idx] = run; delta[idx] = fits ? c - run : sg.dump; cur[idx] = fits ? c + v[j] : end + 1u; cnt[idx] = 0;
            run += v[j];
        }
    }
}

struct ChunkDesc {
    u64 begin, end;          // source range: packed words (reads) or keys
    u32 flat_base;           // matrix entry of bin 0
    u32 stride;              // matrix stride between bins (= chunks in the segment)
};

#define SK_MAX_OWNERS 64
#define SK_BUCKETS 4096                   // minimizer buckets of the repartition table
struct SkParams {
    u64 ngroups;          // 2 * packed words
    u64 ntiles;
    u32 tiles_per_chunk, nchunks;
    u32 k, m, G, R;
    u32 sample_step;      // k_sk_hist: look at every sample_step-th tile only (1 = exact count)
    u32 slice;            // k_sk_scatter<true>: records per (owner, chunk) slice
    // k_sk_scatter<true> writes the chunks [c0, c0 + gridDim) of a layout GROUP of clen chunks that starts at chunk c0g and at record
    // rbase of the send buffer: owner o of the group starts at rbase + o * clen * slice, its chunk c at + (c - c0g) * slice (all 64-bit).
    // One group = all chunks (c0 = c0g = 0, clen = nchunks, rbase = 0): the layout of a whole step; S groups: a step sent in S
    // slices, each complete -- and on its way -- before the next is written (dskgpu_mg_scatter_slice).
    u32 c0, c0g, clen;
    u64 rbase;                    // (64-bit: a rank's shard of a 90 Gbp job holds more than 2^32 records' worth of slices)
    const unsigned char* table;   // SK_BUCKETS owners (device memory)
    u32 has_split;                // the table holds SK_SPLIT entries (set with the table: the kernels skip the split bookkeeping otherwise)
    // k_sk_scatter<true> for the passes of a multi-pass count on ONE GPU ("virtual owners": owner = pass; sender.hip: rec_l0_*): only
    // the records of owners [olo, ohi) are written (a sweep materialises as many passes as HBM holds), every owner has its own slice
    // length oslice[o] (a pass that holds a k-mer with 10^8 occurrences gets longer slices, the others do not pay for it) and its
    // region starts at record obase[o] of the buffer (64-bit: a sweep holds more than 2^32 records).  oslice == nullptr: the
    // uniform layout above, all owners.
    u32 olo, ohi;
    const u32* oslice; const unsigned long long* obase;
};

struct RowsOut { u64* w[4]; };                    // struct-of-arrays rows: word i of row r at w[i][r]
struct RowsIn { const u64* w[4]; };
struct Rows2 { u64* hi; u64* lo; u32* ab; };            // two-word rows as three arrays (rowsort2.h)
struct Rows2C { const u64* hi; const u64* lo; const u32* ab; };
// the solid rows of a single pass where the count kernel left them (regions of cap rows, or exact ranges from fstart; soff = the
// scan of the per-sub-partition solid counts): the row sort's first step reads them there (one- / two-word keys, still mixed)
struct RsSparse { const u64* keys; const u32* ab; const u32* soff; const u32* fstart; u32 cap, F, qpc; };
struct Rs2Sparse { const K2* keys; const u32* ab; const u32* soff; const u32* fstart; u32 cap, F, qpc; };
// four-word keys (k > 64): read there by the partition-order pass only (partsort.h: k_part_sort4) -- the global sort of four-word rows takes dense rows
struct Rs4Sparse { const KN<4>* keys; const u32* ab; const u32* soff; const u32* fstart; u32 cap, F, qpc; };

template <class T>
__global__ void k_gather(T* __restrict__ dst, const T* __restrict__ src, const u32* __restrict__ idx, u64 n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}
