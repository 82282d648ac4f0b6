// planning_rowsort.h -- the host arithmetic that cuts the rows into the chunks of the row sort's first step (step_a_chunks,
// step_a_chunks_sparse).  Host only, no kernel, no context: pure functions of a few integers, swept by tests/host/test_planning.cpp
// over every CU count.  (The count path's planners: planning.h.)
#pragma once
#include <algorithm>

#include "rowsort.h"      // RS_SP_MAXQ

// step A's chunks: about 64 K rows each, a multiple of the CU count of them (whole rounds of blocks), at least one tile each (tile 0:
// no such floor) -> the number of chunks, *chunk = rows per chunk
inline u64 step_a_chunks(u64 n, u64 ncu, u64 tile, u64* chunk) {
    u64 nch = (n + 65535) / 65536;
    nch = (nch + ncu - 1) / ncu * ncu;
    if (tile) nch = std::max<u64>(1, std::min<u64>(nch, (n + tile - 1) / tile));
    *chunk = (n + nch - 1) / nch;
    return (n + *chunk - 1) / *chunk;
}

// the same over a sparse source (the rows still lie in the count kernel's F sub-partitions): chunks = groups of *qpc consecutive sub-partitions
// (about 64 K rows, at most RS_SP_MAXQ sub-partitions), *nch_sp of them, + one chunk of *chunk rows for the dense tail (the rows of the
// k-mers counted apart) -> the number of chunks
inline u64 step_a_chunks_sparse(u64 F, u64 n_sparse, u32 n_tail, u64 ncu, u32* qpc, u64* nch_sp, u64* chunk) {
    u64 want = std::max<u64>(1, (n_sparse + 65535) / 65536);
    want = (want + ncu - 1) / ncu * ncu;
    *qpc = (u32)std::min<u64>(std::max<u64>(1, (F + want - 1) / want), RS_SP_MAXQ);
    *nch_sp = (F + *qpc - 1) / *qpc;
    *chunk = n_tail;
    return *nch_sp + (n_tail ? 1 : 0);
}
