// test_planning.cpp -- unit test (test infrastructure) of the host planners in dsk_amd/csrc/planning.h and planning_rowsort.h, compiled for the HOST with the
// constants of the device headers (no kernel is launched, no device call): make_plan, the level-1 chunking behind build_descs1, and the
// chunks of the row sort's first step, swept over every CU count from 1 to 320 (the library has only ever run at 256), the three key widths,
// extra_bits 0..3 and a logarithmic grid of sizes from 1 to 2^33 with the neighbours of every threshold the code names.  What is checked is what
// the comments in planning.h and the callers promise, not what the functions happen to return.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>
#include "../../dsk_amd/csrc/kernels.h"
#include "../../dsk_amd/csrc/rowsort.h"
#include "../../dsk_amd/csrc/rowsort2.h"
#include "../../dsk_amd/csrc/planning.h"
#include "../../dsk_amd/csrc/planning_rowsort.h"

static long failures = 0, checks = 0;
#define CHECK(c, ...) do { ++checks; if (!(c)) { if (failures < 40) { printf("FAIL %s:%d %s  [", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("]\n"); } ++failures; } } while (0)

// sizes: ~6 per octave from 1 to 2^33
static std::vector<u64> log_grid() {
    std::set<u64> s;
    for (int e = 0; e <= 33; ++e) for (u64 f : {8ull, 9ull, 10ull, 11ull, 13ull, 15ull}) { const u64 v = (f << e) / 8; if (v >= 1 && v <= (1ull << 33)) s.insert(v); }
    return std::vector<u64>(s.begin(), s.end());
}
static void around(std::set<u64>& s, u64 v) { for (long long d = -2; d <= 2; ++d) { const long long x = (long long)v + d; if (x >= 1 && (u64)x <= (1ull << 33)) s.insert((u64)x); } }

static void test_make_plan() {
    const std::vector<u64> grid = log_grid();
    long two_level = 0, large_seen = 0, capped = 0, refused = 0;
    for (int W : {1, 2, 4}) {
        const u64 target = target_keys(W), p2max = plan_p2max(W);
        CHECK(p2max >= 64 && p2max <= MAX_LEVEL_BINS && ascatter_lds(W, (u32)p2max) <= 160 * 1024, "W %d p2max %llu", W, (unsigned long long)p2max);
        for (int eb = 0; eb <= 3; ++eb)
            for (u32 cu = 1; cu <= 320; ++cu) {
                // the thresholds the code names, as numbers of sub-partitions F: one level / two levels, the `large` branch, P1 leaving
                // one and two multiples of the CU count, the cap of P1, the largest F two levels hold
                std::set<u64> ns(grid.begin(), grid.end());
                for (u64 Fth : {(u64)2, (u64)ONE_LEVEL_BINS, (u64)cu * 64, (u64)cu * (p2max - 1), (u64)2 * cu * (p2max - 1), p2max, p2max - 1,
                                (u64)(MAX_LEVEL_BINS - 8) * (p2max - 1), (u64)(MAX_LEVEL_BINS - 8) * MAX_LEVEL_BINS}) {
                    const u64 units = Fth >> eb;      // F = ceil(n / target) << eb
                    for (u64 u : {units, units + 1}) { around(ns, u * target); }
                }
                for (u64 n : ns) {
                    Plan pl{};
                    const bool ok = make_plan(n, eb, W, cu, &pl);
                    u64 F = ((n + target - 1) / target) << eb; if (F < 2) F = 2;
                    if (!ok) { ++refused; CHECK(F > (u64)(MAX_LEVEL_BINS - 8) * MAX_LEVEL_BINS, "refused F %llu W %d eb %d cu %u", (unsigned long long)F, W, eb, cu); continue; }
                    CHECK(pl.P1 >= 1 && pl.P2 >= 1 && pl.P1 <= MAX_LEVEL_BINS && pl.P2 <= MAX_LEVEL_BINS, "P1 %u P2 %u", pl.P1, pl.P2);
                    CHECK((u64)pl.P1 * pl.P2 >= F && pl.F == pl.P1 * pl.P2, "n %llu W %d eb %d cu %u: F %llu P1 %u P2 %u", (unsigned long long)n, W, eb, cu, (unsigned long long)F, pl.P1, pl.P2);
                    CHECK((pl.levels == 1) == (F <= ONE_LEVEL_BINS) && (pl.levels == 1 || pl.levels == 2), "levels %d F %llu", pl.levels, (unsigned long long)F);
                    CHECK(pl.d1.mode == 1 && pl.d1.pa == pl.P1 && pl.d2.mode == 2 && pl.d2.pa == pl.P1 && pl.d2.pb == pl.P2, "digits");
                    if (pl.levels == 1) { CHECK(pl.P2 == 1 && pl.P1 == F, "one level: P1 %u P2 %u F %llu", pl.P1, pl.P2, (unsigned long long)F); continue; }
                    ++two_level;
                    CHECK(pl.P1 >= 2, "two levels with P1 %u: n %llu W %d eb %d cu %u", pl.P1, (unsigned long long)n, W, eb, cu);
                    CHECK(pl.P2 % 2 == 1 || (u64)pl.P2 + 1 > p2max, "even P2 %u (p2max %llu) n %llu W %d eb %d cu %u", pl.P2, (unsigned long long)p2max, (unsigned long long)n, W, eb, cu);
                    if (F >= (u64)cu * 64) {      // the `large` branch
                        ++large_seen;
                        const bool cap = pl.P1 == MAX_LEVEL_BINS - 8;
                        capped += cap;
                        CHECK(cap || pl.P1 % cu == 0, "P1 %u no multiple of %u CUs", pl.P1, cu);
                        CHECK(cap || pl.P1 >= cu, "P1 %u < %u CUs", pl.P1, cu);
                        CHECK(cap || pl.P2 <= p2max, "P2 %u > p2max %llu: n %llu W %d eb %d cu %u", pl.P2, (unsigned long long)p2max, (unsigned long long)n, W, eb, cu);
                        // the fewest such level-1 bins: one multiple of the CU count less (where that still leaves two bins) would not keep level 2 inside p2max - 1 bins
                        if (!cap && pl.P1 > cu && pl.P1 - cu >= 2) CHECK((u64)(pl.P1 - cu) * (p2max - 1) < F, "P1 %u is not the fewest: F %llu cu %u", pl.P1, (unsigned long long)F, cu);
                    }
                }
            }
    }
    CHECK(two_level > 0 && large_seen > 0 && capped > 0 && refused > 0, "the sweep never saw: two levels %ld, large %ld, capped %ld, refused %ld", two_level, large_seen, capped, refused);
}

// chunks1 / chunk_desc1: the chunks cover [0, n) exactly once and in order, none is empty, every one but the last holds whole tiles
static void test_chunks1() {
    const std::vector<u64> grid = log_grid();
    const u64 tiles[] = {1, (u64)Tile<1>::WORDS, (u64)Tile<2>::WORDS, (u64)Tile<4>::WORDS, (u64)Tile<1>::KEYS, (u64)Tile<2>::KEYS, (u64)Tile<4>::KEYS};
    for (u64 tile : tiles)
        for (u32 cu = 1; cu <= 320; ++cu)
            for (u64 per : {1ull, 8ull, 16ull}) {
                const u64 maxc = (u64)cu * per;
                std::set<u64> ns(grid.begin(), grid.end());
                for (u64 t : {tile, tile * maxc, tile * maxc * 2, tile * (maxc + 1)}) around(ns, t);
                for (u64 n : ns) {
                    u64 tpc = 0; const u64 nch = chunks1(n, tile, maxc, &tpc);
                    CHECK(nch >= 1 && nch <= maxc && tpc >= 1, "n %llu tile %llu maxc %llu: nch %llu tpc %llu", (unsigned long long)n, (unsigned long long)tile, (unsigned long long)maxc, (unsigned long long)nch, (unsigned long long)tpc);
                    CHECK(nch * tpc * tile >= n && (nch - 1) * tpc * tile < n, "n %llu tile %llu maxc %llu: nch %llu tpc %llu", (unsigned long long)n, (unsigned long long)tile, (unsigned long long)maxc, (unsigned long long)nch, (unsigned long long)tpc);
                    // the descriptors: first, last, and a few in between (all of them when there are few)
                    u64 expect = 0; bool all = nch <= 64;
                    std::set<u64> cs;
                    if (all) for (u64 c = 0; c < nch; ++c) cs.insert(c);
                    else for (u64 i = 0; i <= 8; ++i) { const u64 c = (nch - 1) * i / 8; cs.insert(c); cs.insert(c ? c - 1 : 0); }
                    for (u64 c : cs) {
                        const ChunkDesc d = chunk_desc1(c, nch, tpc, tile, n);
                        CHECK(d.begin == c * tpc * tile && d.begin < d.end && d.end <= n && d.flat_base == (u32)c && d.stride == (u32)nch, "chunk %llu of %llu: [%llu, %llu) n %llu", (unsigned long long)c, (unsigned long long)nch, (unsigned long long)d.begin, (unsigned long long)d.end, (unsigned long long)n);
                        if (c + 1 < nch) CHECK(d.end - d.begin == tpc * tile, "inner chunk %llu is no %llu whole tiles", (unsigned long long)c, (unsigned long long)tpc);
                        else CHECK(d.end == n, "last chunk ends at %llu, n %llu", (unsigned long long)d.end, (unsigned long long)n);
                        if (all) { CHECK(d.begin == expect, "gap before chunk %llu", (unsigned long long)c); expect = d.end; }
                    }
                }
            }
}

// step_a_chunks: nch chunks of `chunk` rows cover [0, n) (chunk c = [c * chunk, min(n, (c + 1) * chunk))), none empty; no more than the
// CU-multiple of 64 K-row chunks; the chunk x bin matrix stays below the row sort's 32-bit guard for every n here
static void test_step_a() {
    const std::vector<u64> grid = log_grid();
    for (u64 tile : {(u64)0, (u64)RS_TILE, (u64)RS2_TILE})
        for (u64 cu = 1; cu <= 320; ++cu) {
            std::set<u64> ns(grid.begin(), grid.end());
            for (u64 t : {(u64)65536, 65536 * cu, 2 * 65536 * cu, (u64)RS_TILE, (u64)RS2_TILE, RS_TILE * cu, RS2_TILE * cu}) around(ns, t);
            for (u64 n : ns) {
                u64 chunk = 0; const u64 nch = step_a_chunks(n, cu, tile, &chunk);
                const u64 rounds = ((n + 65535) / 65536 + cu - 1) / cu;
                CHECK(nch >= 1 && chunk >= 1 && nch * chunk >= n && (nch - 1) * chunk < n, "n %llu cu %llu tile %llu: nch %llu chunk %llu", (unsigned long long)n, (unsigned long long)cu, (unsigned long long)tile, (unsigned long long)nch, (unsigned long long)chunk);
                CHECK(nch <= rounds * cu, "n %llu cu %llu: %llu chunks, more than %llu rounds of blocks", (unsigned long long)n, (unsigned long long)cu, (unsigned long long)nch, (unsigned long long)rounds);
                CHECK(chunk <= 65536, "n %llu cu %llu tile %llu: chunk of %llu rows", (unsigned long long)n, (unsigned long long)cu, (unsigned long long)tile, (unsigned long long)chunk);
                if (tile && n >= tile) CHECK(2 * chunk > tile, "n %llu cu %llu tile %llu: chunk of %llu rows", (unsigned long long)n, (unsigned long long)cu, (unsigned long long)tile, (unsigned long long)chunk);
                CHECK((u64)RS_ABINS * nch < 0xFFFFFFF0ull, "matrix of %llu chunks", (unsigned long long)nch);
            }
        }
}

// step_a_chunks_sparse: groups of qpc <= RS_SP_MAXQ consecutive sub-partitions cover the F of them, none empty; one more chunk for the tail
static void test_step_a_sparse() {
    const u64 Fs[] = {2, 3, 63, 64, 1023, 1024, 1025, 1297, 2047, 2048, 2049, 36 * 37, 256 * 64, 256 * 769, 304 * 769, 1024 * 1024 + 1, (u64)(MAX_LEVEL_BINS - 8) * MAX_LEVEL_BINS};
    for (u64 F : Fs)
        for (u64 cu = 1; cu <= 320; ++cu)
            for (u64 fill : {0ull, 1ull, 7ull, 100ull, 1000ull, 2900ull, 4360ull}) {      // rows per sub-partition, up to a full region
                const u64 n_sparse = std::min<u64>(F * fill, 0xFFFF0000ull);
                for (u32 n_tail : {0u, 1u, 4096u}) {
                    u32 qpc = 0; u64 nch_sp = 0, chunk = ~0ull;
                    const u64 nch = step_a_chunks_sparse(F, n_sparse, n_tail, cu, &qpc, &nch_sp, &chunk);
                    CHECK(qpc >= 1 && qpc <= RS_SP_MAXQ, "F %llu rows %llu cu %llu: qpc %u", (unsigned long long)F, (unsigned long long)n_sparse, (unsigned long long)cu, qpc);
                    CHECK(nch_sp >= 1 && nch_sp * qpc >= F && (nch_sp - 1) * qpc < F, "F %llu rows %llu cu %llu: qpc %u nch_sp %llu", (unsigned long long)F, (unsigned long long)n_sparse, (unsigned long long)cu, qpc, (unsigned long long)nch_sp);
                    CHECK(nch == nch_sp + (n_tail ? 1 : 0) && chunk == n_tail, "tail chunk: nch %llu nch_sp %llu chunk %llu", (unsigned long long)nch, (unsigned long long)nch_sp, (unsigned long long)chunk);
                    CHECK((u64)RS_ABINS * nch < 0xFFFFFFF0ull, "F %llu rows %llu cu %llu: matrix of %llu chunks", (unsigned long long)F, (unsigned long long)n_sparse, (unsigned long long)cu, (unsigned long long)nch);
                }
            }
}

// busiest_share1: the share the level-1 slices are sized from is the share of the block that walks the most units -- no block walks more,
// one walks exactly that -- for every grid the scatter may take (1 .. nch blocks).  And the figure it replaced, ceil(nch / grid) / nch,
// is too small by more than the 1 % of room the slices have where the last chunk is short and the chunks are few: the witness below
// (295 tiles, 3 CUs) is the k = 31 stream of tests/test_gpu_cu_counts.py, whose level 1 overflowed into the exact path before.
static void test_busiest_share() {
    const std::vector<u64> grid = log_grid();
    const u64 tile = (u64)Tile<1>::WORDS;
    long understated = 0;
    for (u32 cu = 1; cu <= 320; cu += (cu < 40 ? 1 : 7))
        for (u64 n : grid) {
            if (n > (1ull << 30)) continue;
            u64 tpc = 0; const u64 nch = chunks1(n, tile, (u64)cu * 8, &tpc);
            std::vector<ChunkDesc> d(nch);
            for (u64 c = 0; c < nch; ++c) d[c] = chunk_desc1(c, nch, tpc, tile, n);
            for (u64 g : {(u64)1, (u64)cu, std::min<u64>(nch, (u64)cu * 2), nch}) {
                if (g < 1 || g > nch) continue;
                const double share = busiest_share1(d.data(), nch, g);
                u64 most = 0;
                for (u64 b = 0; b < g; ++b) { u64 u = 0; for (u64 c = b; c < nch; c += g) u += d[c].end - d[c].begin; most = std::max(most, u); }
                CHECK(share == (double)most / (double)n && share > 0 && share <= 1.0, "n %llu cu %u grid %llu: share %f, busiest block %llu units", (unsigned long long)n, cu, (unsigned long long)g, share, (unsigned long long)most);
                const double old_share = (double)((nch + g - 1) / g) / (double)nch;
                if (share > old_share * 1.01) ++understated;
            }
        }
    CHECK(understated > 0, "no input of the sweep where chunks / grid understates the busiest block by more than 1 %%");
    const u64 n = 295 * (u64)Tile<1>::WORDS - 5;
    u64 tpc = 0; const u64 nch = chunks1(n, tile, 3 * 8, &tpc);
    std::vector<ChunkDesc> d(nch);
    for (u64 c = 0; c < nch; ++c) d[c] = chunk_desc1(c, nch, tpc, tile, n);
    CHECK(nch == 23 && tpc == 13, "witness: nch %llu tpc %llu", (unsigned long long)nch, (unsigned long long)tpc);
    CHECK(busiest_share1(d.data(), nch, 3) > 8.0 / 23.0 * 1.01, "witness: share %f", busiest_share1(d.data(), nch, 3));
}

int main() {
    test_make_plan();
    test_chunks1();
    test_busiest_share();
    test_step_a();
    test_step_a_sparse();
    printf("%ld checks, %ld failures\n", checks, failures);
    if (failures) return 1;
    printf("ALL OK\n");
    return 0;
}
