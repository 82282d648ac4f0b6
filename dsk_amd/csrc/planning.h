// planning.h -- the host arithmetic that sizes the count path from a few integers: how many final sub-partitions a pass gets and how they
// split over the two scatter levels (make_plan), how a level-1 source is cut into chunks (chunks1 / chunk_desc1, which build_descs1 of
// dskgpu.hip writes into the context) and which share of it the busiest block of the level-1 scatter walks (busiest_share1).
// Host only, no kernel is launched, no context: pure functions, so that tests/host/test_planning.cpp can sweep them over every CU count.
// (The row sort's chunkers: planning_rowsort.h.)
#pragma once
#include <algorithm>

#include <vector>

#include "kernels.h"      // SC_NT, ascatter_lds, DigitSpec, ChunkDesc

// ---- level 1: chunks of a source of n_units_total units (packed words or keys) in tiles of `tile` units: at most max_chunks chunks of
// *tpc whole tiles each -> the number of chunks (every chunk but the last holds *tpc tiles, none is empty)
inline u64 chunks1(u64 n_units_total, u64 tile, u64 max_chunks, u64* tpc) {
    const u64 ntiles = std::max<u64>(1, (n_units_total + tile - 1) / tile);
    u64 nch = std::min<u64>(ntiles, max_chunks);
    *tpc = (ntiles + nch - 1) / nch;
    nch = (ntiles + *tpc - 1) / *tpc;
    return nch;
}
inline ChunkDesc chunk_desc1(u64 c, u64 nch, u64 tpc, u64 tile, u64 n_units_total) {
    ChunkDesc d;
    d.begin = c * tpc * tile;
    d.end = std::min<u64>(n_units_total, (c + 1) * tpc * tile);
    if (d.begin > d.end) d.begin = d.end;
    d.flat_base = (u32)c;
    d.stride = (u32)nch;
    return d;
}

// the share of the input that the busiest block of the level-1 scatter walks: block b of `grid` takes chunks b, b + grid, .. of the nch
// descriptors d.  Not ceil(nch / grid) / nch: the last chunk may hold one tile where the others hold tpc, and with few chunks (8 per
// CU: a device or partition with a dozen CUs) a block that walks only full chunks then has up to 1 / nch more than that share -- more
// than the 1 % of room the level-1 slices are given, so level 1 overflowed and the count fell back to the exact (histogram) path.
// E.g. 295 tiles at 3 CUs: 23 chunks of 13 tiles, block 0 walks 8 full ones = 104 / 295 = 0.3525 of the input against 8 / 23 = 0.3478.
inline double busiest_share1(const ChunkDesc* d, u64 nch, u64 grid) {
    std::vector<u64> units(grid, 0); u64 all = 0;
    for (u64 c = 0; c < nch; ++c) { const u64 u = d[c].end - d[c].begin; units[c % grid] += u; all += u; }
    return all ? (double)*std::max_element(units.begin(), units.end()) / (double)all : (double)((nch + grid - 1) / grid) / (double)nch;
}

// ---- the count plan
struct Plan {
    int levels;
    u32 P1, P2, F;
    DigitSpec d1, d2;
};

#define TARGET_KEYS 2900      // mean keys per final sub-partition (the count kernel prefetches 3072 per sub-partition; table: 4096 slots, 3584 usable)
#define TARGET_KEYS2 2560     // two-word keys: 3072-slot top-word table (k_count2v3), 2688 usable; 4096-slot index table (k_count_mw)
#ifndef TARGET_KEYS4
#define TARGET_KEYS4 640      // four-word keys: 1024 staged per sub-partition
#endif
#define MAX_LEVEL_BINS 2048
#define ONE_LEVEL_BINS 1024
inline u64 target_keys(int W) { return W == 1 ? TARGET_KEYS : W == 2 ? TARGET_KEYS2 : TARGET_KEYS4; }
// most level-2 bins whose per-bin carry the aligned level-2 scatter holds in one CU's LDS
inline u64 plan_p2max(int W) { u64 p2max = MAX_LEVEL_BINS; while (p2max > 64 && ascatter_lds(W, (u32)p2max) > 160 * 1024) --p2max; return p2max; }

// Final sub-partitions F = P1 * P2 sized to the input (any integer, not a power
// of two: digits use the multiply-shift reduction of key_digit()).
inline bool make_plan(u64 n_upper, int extra_bits, int W, u32 num_cu, Plan* pl) {
    const u64 target = target_keys(W);
    u64 F = ((n_upper + target - 1) / target) << extra_bits;
    if (F < 2) F = 2;
    if (F <= ONE_LEVEL_BINS) { pl->levels = 1; pl->P1 = (u32)F; pl->P2 = 1; }
    else {
        // Level 1 costs more per key the more bins it has (3.05 ps + 1.7 fs per bin and key, NOTEBOOK.md section 6: every tile leaves a
        // partial line per bin), level 2 costs the same for any number of bins its kernel holds (the per-bin carry must fit LDS:
        // p2max).  So: the FEWEST level-1 bins that keep level 2 inside that kernel -- but at least one segment per CU, and a
        // multiple of the CU count: level 2 gives every block whole segments (level-1 bins), one block per CU, and a count that is
        // not a multiple leaves some blocks one segment more than the rest (770 segments on 256 CUs cost 20 %).
        const u64 p2max = plan_p2max(W);
        u64 p1 = 1; while (p1 * p1 < F) ++p1;                                  // balanced split: small inputs
        const bool large = F >= (u64)num_cu * 64;
        if (large) {
            p1 = std::max<u64>((F + p2max - 2) / (p2max - 1), std::max<u64>(num_cu, 2));      // (p2max - 1: room for the odd-P2 adjustment below; 2: a single CU and four-word keys, whose p2max is above ONE_LEVEL_BINS, would get "two levels" with one level-1 bin)
            p1 = (p1 + num_cu - 1) / num_cu * num_cu;
            if (p1 > MAX_LEVEL_BINS - 8) p1 = MAX_LEVEL_BINS - 8;
        }
        u64 p2 = (F + p1 - 1) / p1;
        // An ODD number of level-2 bins: the regions of sub-partition q start q * 545 groups of 64 B into the buffer, and the
        // blocks walk their segments in step, so with an even P2 (768 * 545 * 64 B = a multiple of 8 KB between segments) all
        // write fronts sit on the same few HBM channels -- measured 6.0 ms at P2 = 768 against 4.7-5.0 ms at P2 = 769.
        if (p2 % 2 == 0 && p2 + 1 <= p2max) ++p2;
        if (p1 > MAX_LEVEL_BINS || p2 > MAX_LEVEL_BINS) return false;
        pl->levels = 2; pl->P1 = (u32)p1; pl->P2 = (u32)p2;
    }
    pl->F = pl->P1 * pl->P2;
    pl->d1 = DigitSpec{1u, pl->P1, 0u, 1u, 1u, 0u};
    pl->d2 = DigitSpec{2u, pl->P1, pl->P2, 1u, 1u, 0u};
    return true;
}
