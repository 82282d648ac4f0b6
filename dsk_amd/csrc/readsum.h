// readsum.h -- HIP kernels of the per-read abundance summaries and of the read selection (gfx950 / MI355X, wave64): dskgpu_read_summaries /
// _read_summaries_table / _read_marks / dskgpu_select_reads (readsum.hip; the definitions are in include/dskgpu.h).
//
// A RECORD is what lies between two '\n' of the stream; its VALUES are the abundances a(p) of its valid windows.
//
//   k_rs_values<W>          the frame of k_query_reads<W>: the N = 16 / W windows of a thread probed as one batch (q_lookup).  a(p) into a buffer
//                           of the library's own that is padded to whole words of 32 positions, so a lane's N values always leave as 16-byte
//                           stores; the frame's valid mask vm, one bit per position, is gathered over the 32 / N lanes of a word by xor
//                           shuffles and leaves as ONE u32 per word.  Zero alone cannot tell "invalid" from "no row": the bit does
//   k_rs_records<EMIT, AL>  16 bytes per thread (AL: one 16-byte load).  EMIT false: the '\n' of every block (scanned by the host side).
//                           EMIT true: the same '\n' again, ranked inside the block (wave_incl_scan + the waves' totals in LDS) on top of the
//                           scanned block sums -> ends[i] = the position of the i-th '\n'; a last record without one ends at nbytes
//   k_rs_spans              one thread per record: start and len into its summary, the longest record, a record above the u32 limit, and the
//                           records longer than RS_WAVE_CAP onto the list of the block path (one add per wave that has some; the ORDER of
//                           the list depends on scheduling, what is computed from it does not: every record owns its summary)
//   k_rs_short              one wave per record of len <= RS_WAVE_CAP, the values in RS_SLOTS registers per lane.  n_valid / n_solid: ballots;
//                           sum / max: xor-shuffle reductions; the median: a bitwise radix select from the top set bit of the wave's maximum
//                           down, one ballot + popcount per register slot and bit.  Every lane stays in every wave-wide operation
//   k_rs_long               one block per listed record, looping over it in strides of 256 (any len up to the u32 limit): the reductions through
//                           LDS, the median by up to four passes of 8-bit digit histograms in LDS over the values in HBM, top digit first
//   k_rs_marks              one thread per record: the RULE, products compared in u64
//   k_rs_outlen             one thread per record: len + 1 of a kept record, 0 of another (scanned by the host side), the kept records longer
//                           than RS_WAVE_CAP onto the list of the block copy
//   k_rs_copy_short / _long the kept records to their places: one wave per short record, one block per listed long one, byte by byte -- any
//                           alignment of either side -- and the '\n' behind
//
// Both summary paths give the same 32 bytes for the same record (the tests move records across RS_WAVE_CAP).  Global atomics: counters only,
// combined per block (or wave) first; nothing that is reported depends on their order.
#pragma once
#include "query.h"

#ifndef RS_WAVE_CAP
#define RS_WAVE_CAP 256                   // the longest record of the wave path (profiles/read_summaries.md); a multiple of 64
#endif
#define RS_SLOTS (RS_WAVE_CAP / 64)       // values a lane of k_rs_short holds
#define RS_PER 16                         // bytes per thread of k_rs_records: one 16-byte load
#define RS_BLOCK (256 * RS_PER)           // bytes per block of it
static_assert(RS_WAVE_CAP % 64 == 0 && RS_WAVE_CAP >= 64 && RS_WAVE_CAP <= 1024, "RS_WAVE_CAP");

enum RsStat { RS_ST_EMPTY = 0, RS_ST_VALID, RS_ST_SOLID, RS_ST_MAXLEN, RS_ST_TOOLONG, RS_ST_NLONG, RS_ST_KEPT, RS_ST_KBYTES, RS_ST_KVALID, RS_ST_COUNT };

struct RsSummary { u64 start, sum; u32 len, n_valid, n_solid, median; };      // the SUMMARY of include/dskgpu.h: 32 bytes
static_assert(sizeof(RsSummary) == 32, "RsSummary");

struct RsRule { u32 min_valid, median_min, median_max, solid_num, solid_den, invert; };

__device__ __forceinline__ u64 rs_shfl_xor64(u64 x, int m) {
    const u32 lo = (u32)__shfl_xor((int)(u32)x, m, 64), hi = (u32)__shfl_xor((int)(u32)(x >> 32), m, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 rs_shfl64(u64 x, int src) {
    const u32 lo = (u32)__shfl((int)(u32)x, src, 64), hi = (u32)__shfl((int)(u32)(x >> 32), src, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 rs_wave_sum64(u64 x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += rs_shfl_xor64(x, m);
    return x;
}
__device__ __forceinline__ u32 rs_wave_max32(u32 x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const u32 y = (u32)__shfl_xor((int)x, m, 64); x = y > x ? y : x; }
    return x;
}
__device__ __forceinline__ void rs_max64(u64* at, u64 v) {
    (void)__hip_atomic_fetch_max(reinterpret_cast<unsigned long long*>(at), (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// stat[first + i] += the sum over the block of mine[i], i < NC (64-bit: a block of a grid-stride kernel may see more than 2^32): LDS first,
// one add per counter and block that has something.  Every thread of the block calls it, once per kernel.
template <int NC>
__device__ __forceinline__ void rs_block_counts(const u64 (&mine)[NC], u64* stat, int first) {
    __shared__ unsigned long long s_cnt[NC];
    if (threadIdx.x < NC) s_cnt[threadIdx.x] = 0ull;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NC; ++i) if (mine[i]) atomicAdd(&s_cnt[i], (unsigned long long)mine[i]);
    __syncthreads();
    if (threadIdx.x < NC && s_cnt[threadIdx.x]) q_add64(stat + first + threadIdx.x, (u64)s_cnt[threadIdx.x]);
}

// Thread t: the N windows ending at bases 32 * (t / TPW) + (t % TPW) * N + j of the encoded stream, as k_query_reads.  vals: nwords * 32
// values, 16-byte aligned, 0 where no valid window ends (the positions from nbytes on included); vbits[w] bit j: position 32 w + j is valid.
// The TPW lanes of a word are neighbours inside one wave (TPW divides 64, a block starts at a multiple of TPW)
template <int W>
__global__ __launch_bounds__(256) void k_rs_values(const u64* __restrict__ packed, const u32* __restrict__ inval, u64 nwords, u64 nbytes, int k,
                                                   QTable T, u32* __restrict__ vals, u32* __restrict__ vbits) {
    constexpr int N = QBatch<W>::N, TPW = 32 / N;
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 wi = t / TPW;
    const int t0 = (int)(t % TPW) * N;
    u32 vm = 0;
    if (wi < nwords) {
        KN<W> c[N];
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
        uint4* o = reinterpret_cast<uint4*>(vals + p0);                          // (p0 is a multiple of N >= 4; vals is padded to whole words)
#pragma unroll
        for (int q = 0; q < N / 4; ++q) o[q] = make_uint4(res[4 * q], res[4 * q + 1], res[4 * q + 2], res[4 * q + 3]);
    }
    u32 word = vm << t0;                                                         // no lane leaves before the shuffles
#pragma unroll
    for (int m = 1; m < TPW; m <<= 1) word |= (u32)__shfl_xor((int)word, m, 64);
    if (t0 == 0 && wi < nwords) vbits[wi] = word;
}

// EMIT false: bsum[block] = the '\n' of the block.  EMIT true: bbase = the exclusive scan of bsum; ends[i] = the position of the i-th '\n',
// i < n_nl; n_ends > n_nl (the last byte is no '\n'): ends[n_nl] = nbytes.
template <bool EMIT, bool ALIGNED>
__global__ __launch_bounds__(256) void k_rs_records(const unsigned char* __restrict__ s, u64 nbytes, u64* __restrict__ bsum, const u64* __restrict__ bbase,
                                                    u64* __restrict__ ends, u64 n_nl, u64 n_ends) {
    __shared__ u32 s_wave[4];
    const u64 p0 = (u64)blockIdx.x * RS_BLOCK + (u64)threadIdx.x * RS_PER;
    u32 nl = 0;                                                                  // bit q: byte p0 + q is a '\n'
    if (ALIGNED && p0 + RS_PER <= nbytes) {
        const uint4 v = *reinterpret_cast<const uint4*>(s + p0);
        const u32 w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < RS_PER; ++q) if (((w4[q >> 2] >> (8 * (q & 3))) & 0xFFu) == 0x0Au) nl |= 1u << q;
    } else {
#pragma unroll
        for (int q = 0; q < RS_PER; ++q) if (p0 + q < nbytes && s[p0 + q] == 0x0A) nl |= 1u << q;
    }
    const u32 mine = (u32)__popc(nl);
    const u32 incl = wave_incl_scan(mine);
    if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = incl;
    __syncthreads();
    if constexpr (!EMIT) {
        if (threadIdx.x == 0) bsum[blockIdx.x] = (u64)(s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3]);
    } else {
        u32 excl = incl - mine;
        const u32 wave = threadIdx.x >> 6;
#pragma unroll
        for (u32 w = 0; w < 3; ++w) excl += w < wave ? s_wave[w] : 0u;
        u64 at = bbase[blockIdx.x] + (u64)excl;
        while (nl) {
            const int q = __builtin_ctz(nl);
            nl &= nl - 1;
            if (at < n_nl) ends[at] = p0 + (u64)q;
            ++at;
        }
        if (n_ends > n_nl && p0 < nbytes && nbytes <= p0 + RS_PER) ends[n_nl] = nbytes;      // (the thread of the last byte)
    }
}

__device__ __forceinline__ u64 rs_start(const u64* __restrict__ ends, u64 r) { return r ? ends[r - 1] + 1 : 0ull; }

// tab[r].start / .len of every record; stat[RS_ST_MAXLEN], [RS_ST_TOOLONG]; list[0 .. stat[RS_ST_NLONG]) = the records longer than RS_WAVE_CAP
__global__ __launch_bounds__(256) void k_rs_spans(const u64* __restrict__ ends, u64 n_rec, RsSummary* __restrict__ tab, u64* __restrict__ list, u64* __restrict__ stat) {
    __shared__ unsigned long long s_max;
    if (threadIdx.x == 0) s_max = 0ull;
    __syncthreads();
    const u64 stride = (u64)gridDim.x * blockDim.x;
    const u64 rounds = (n_rec + stride - 1) / stride;                            // (every lane makes every round: the ballot below is wave-wide)
    u64 longest = 0;
    for (u64 i = 0; i < rounds; ++i) {
        const u64 r = i * stride + (u64)blockIdx.x * blockDim.x + threadIdx.x;
        bool is_long = false;
        if (r < n_rec) {
            const u64 start = rs_start(ends, r), len = ends[r] - start;
            tab[r].start = start;
            tab[r].len = (u32)len;
            longest = len > longest ? len : longest;
            is_long = len > (u64)RS_WAVE_CAP;
        }
        const u64 b = __ballot(is_long);
        if (b) {
            const u32 lane = threadIdx.x & 63u;
            u64 base = 0;
            if (lane == (u32)__builtin_ctzll(b))
                base = __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(stat + RS_ST_NLONG), (unsigned long long)__popcll(b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            base = rs_shfl64(base, __builtin_ctzll(b));
            if (is_long) list[base + (u64)__popcll(b & ((1ull << lane) - 1ull))] = r;
        }
    }
    if (longest) atomicMax(&s_max, (unsigned long long)longest);
    __syncthreads();
    if (threadIdx.x == 0 && s_max) {
        rs_max64(stat + RS_ST_MAXLEN, (u64)s_max);
        if (s_max > 0xFFFFFFFFull) rs_max64(stat + RS_ST_TOOLONG, 1ull);
    }
}

__device__ __forceinline__ bool rs_valid(const u32* __restrict__ vbits, u64 p) { return (vbits[p >> 5] >> (u32)(p & 31)) & 1u; }

// Wave w of the grid: the records w, w + waves, ...; those longer than RS_WAVE_CAP are the block path's.  Lane l holds the positions
// start + l + 64 s, s < RS_SLOTS.  tmin >= 1.  stat[RS_ST_EMPTY ..]: records without a valid window, valid positions, solid positions
__global__ __launch_bounds__(256) void k_rs_short(const u32* __restrict__ vals, const u32* __restrict__ vbits, u64 n_rec, u32 tmin, RsSummary* __restrict__ tab,
                                                  u64* __restrict__ stat) {
    const u32 lane = threadIdx.x & 63u;
    const u64 waves = (u64)gridDim.x * 4u;
    u64 cnt[3] = {0ull, 0ull, 0ull};
    for (u64 r = (u64)blockIdx.x * 4u + (threadIdx.x >> 6); r < n_rec; r += waves) {      // (r is the wave's: the loop and the skip are wave-uniform)
        const u64 start = tab[r].start;
        const u32 len = tab[r].len;
        if (len > (u32)RS_WAVE_CAP) continue;
        u32 a[RS_SLOTS]; bool v[RS_SLOTS];
#pragma unroll
        for (int s = 0; s < RS_SLOTS; ++s) {
            const u32 i = lane + 64u * (u32)s;
            v[s] = i < len && rs_valid(vbits, start + i);
            a[s] = v[s] ? vals[start + i] : 0u;
        }
        u32 n_valid = 0, n_solid = 0, mx = 0;
        u64 sum = 0;
#pragma unroll
        for (int s = 0; s < RS_SLOTS; ++s) {
            n_valid += (u32)__popcll(__ballot(v[s]));
            n_solid += (u32)__popcll(__ballot(v[s] && a[s] >= tmin));
            sum += (u64)a[s];
            mx = a[s] > mx ? a[s] : mx;
        }
        sum = rs_wave_sum64(sum);
        mx = (u32)__builtin_amdgcn_readfirstlane((int)rs_wave_max32(mx));
        // the element of index kth of the valid values in ascending order: bit by bit from the top, v[] = the values still in the race
        u32 kth = n_valid >> 1, median = 0;
        for (int b = mx ? 31 - __builtin_clz(mx) : -1; b >= 0; --b) {
            u32 zeros = 0;
#pragma unroll
            for (int s = 0; s < RS_SLOTS; ++s) zeros += (u32)__popcll(__ballot(v[s] && !((a[s] >> b) & 1u)));
            const bool one = kth >= zeros;
            if (one) { kth -= zeros; median |= 1u << b; }
#pragma unroll
            for (int s = 0; s < RS_SLOTS; ++s) v[s] = v[s] && (((a[s] >> b) & 1u) == (one ? 1u : 0u));
        }
        if (lane == 0) {
            tab[r].sum = sum; tab[r].n_valid = n_valid; tab[r].n_solid = n_solid; tab[r].median = median;
            cnt[0] += n_valid == 0 ? 1ull : 0ull; cnt[1] += n_valid; cnt[2] += n_solid;
        }
    }
    rs_block_counts<3>(cnt, stat, RS_ST_EMPTY);
}

// Block b of the grid: the listed records b, b + blocks, ...  Thread t takes the positions start + t + 256 i
__global__ __launch_bounds__(256) void k_rs_long(const u32* __restrict__ vals, const u32* __restrict__ vbits, const u64* __restrict__ list, u64 n_long, u32 tmin,
                                                 RsSummary* __restrict__ tab, u64* __restrict__ stat) {
    __shared__ u32 s_hist[256];
    __shared__ unsigned long long s_sum;
    __shared__ u32 s_nv, s_ns, s_max, s_digit, s_kth;
    u64 cnt[3] = {0ull, 0ull, 0ull};
    for (u64 li = blockIdx.x; li < n_long; li += gridDim.x) {                    // (block-uniform)
        const u64 r = list[li];
        const u64 start = tab[r].start;
        const u32 len = tab[r].len;
        if (threadIdx.x == 0) { s_sum = 0ull; s_nv = 0u; s_ns = 0u; s_max = 0u; }
        __syncthreads();
        u32 nv = 0, ns = 0, mx = 0;
        u64 sum = 0;
        for (u64 i = threadIdx.x; i < (u64)len; i += 256u) {
            if (!rs_valid(vbits, start + i)) continue;
            const u32 a = vals[start + i];
            ++nv; ns += a >= tmin ? 1u : 0u; sum += (u64)a; mx = a > mx ? a : mx;
        }
        if (nv) { atomicAdd(&s_nv, nv); atomicAdd(&s_sum, (unsigned long long)sum); atomicMax(&s_max, mx); }
        if (ns) atomicAdd(&s_ns, ns);
        __syncthreads();
        const u32 n_valid = s_nv, top = s_max;
        // the element of index n_valid / 2: the 8-bit digit of it from the top digit of the maximum down, `prefix` = the digits above
        u32 prefix = 0;
        if (threadIdx.x == 0) s_kth = n_valid >> 1;
        for (int shift = top ? ((31 - __builtin_clz(top)) & ~7) : -8; shift >= 0; shift -= 8) {
            s_hist[threadIdx.x] = 0u;
            __syncthreads();
            for (u64 i = threadIdx.x; i < (u64)len; i += 256u) {
                if (!rs_valid(vbits, start + i)) continue;
                const u32 a = vals[start + i];
                if (shift == 24 || (a >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&s_hist[(a >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                u32 kth = s_kth, d = 0;
                while (d < 255u && kth >= s_hist[d]) { kth -= s_hist[d]; ++d; }
                s_kth = kth; s_digit = d;
            }
            __syncthreads();
            prefix |= s_digit << shift;
        }
        if (threadIdx.x == 0) {
            tab[r].sum = (u64)s_sum; tab[r].n_valid = n_valid; tab[r].n_solid = s_ns; tab[r].median = prefix;
            cnt[0] += n_valid == 0 ? 1ull : 0ull; cnt[1] += n_valid; cnt[2] += s_ns;
        }
        __syncthreads();                                                         // (the next record's reset comes after this one's reads)
    }
    rs_block_counts<3>(cnt, stat, RS_ST_EMPTY);
}

__device__ __forceinline__ bool rs_kept(const RsSummary& S, const RsRule& R) {
    bool keep = S.n_valid >= R.min_valid && S.median >= R.median_min && (R.median_max == 0u || S.median <= R.median_max) &&
                (R.solid_den == 0u || (u64)S.n_solid * (u64)R.solid_den >= (u64)R.solid_num * (u64)S.n_valid);
    return keep != (R.invert != 0u);
}

// keep[r] (may be null) = 1 or 0; stat[RS_ST_KEPT ..]: the kept records, their len + 1, their valid positions
__global__ __launch_bounds__(256) void k_rs_marks(const RsSummary* __restrict__ tab, u64 n_rec, RsRule R, unsigned char* __restrict__ keep, u64* __restrict__ stat) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    u64 cnt[3] = {0ull, 0ull, 0ull};
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += stride) {
        const RsSummary S = tab[r];
        const bool kp = rs_kept(S, R);
        if (keep) keep[r] = kp ? 1 : 0;
        if (kp) { cnt[0] += 1ull; cnt[1] += (u64)S.len + 1ull; cnt[2] += (u64)S.n_valid; }
    }
    rs_block_counts<3>(cnt, stat, RS_ST_KEPT);
}

// olen[r] = len + 1 of a kept record, else 0; olen[n_rec] = 0 (the scan's last input); stat[RS_ST_KEPT] += the kept records;
// list[0 .. stat[RS_ST_NLONG]) = the kept records longer than RS_WAVE_CAP
__global__ __launch_bounds__(256) void k_rs_outlen(const u64* __restrict__ ends, u64 n_rec, const unsigned char* __restrict__ keep, u64* __restrict__ olen,
                                                   u64* __restrict__ list, u64* __restrict__ stat) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    u64 cnt[1] = {0ull};
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r <= n_rec; r += stride) {
        u64 o = 0;
        if (r < n_rec && keep[r]) {
            const u64 len = ends[r] - rs_start(ends, r);
            o = len + 1;
            cnt[0] += 1ull;
            if (len > (u64)RS_WAVE_CAP)
                list[__hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(stat + RS_ST_NLONG), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)] = r;
        }
        olen[r] = o;
    }
    rs_block_counts<1>(cnt, stat, RS_ST_KEPT);
}

// Wave w of the grid: the records w, w + waves, ...: a kept one of len <= RS_WAVE_CAP goes to out[obase[r] ..], a '\n' behind it
__global__ __launch_bounds__(256) void k_rs_copy_short(const unsigned char* __restrict__ s, const u64* __restrict__ ends, u64 n_rec, const unsigned char* __restrict__ keep,
                                                       const u64* __restrict__ obase, unsigned char* __restrict__ out) {
    const u32 lane = threadIdx.x & 63u;
    const u64 waves = (u64)gridDim.x * 4u;
    for (u64 r = (u64)blockIdx.x * 4u + (threadIdx.x >> 6); r < n_rec; r += waves) {
        if (!keep[r]) continue;
        const u64 start = rs_start(ends, r), len = ends[r] - start;
        if (len > (u64)RS_WAVE_CAP) continue;
        const u64 at = obase[r];
#pragma unroll
        for (int q = 0; q < RS_SLOTS; ++q) {
            const u64 i = lane + 64u * (u32)q;
            if (i < len) out[at + i] = s[start + i];
        }
        if (lane == 0) out[at + len] = 0x0A;
    }
}

// Block b of the grid: the listed records b, b + blocks, ..., in strides of 256 bytes
__global__ __launch_bounds__(256) void k_rs_copy_long(const unsigned char* __restrict__ s, const u64* __restrict__ ends, const u64* __restrict__ list, u64 n_long,
                                                      const u64* __restrict__ obase, unsigned char* __restrict__ out) {
    for (u64 li = blockIdx.x; li < n_long; li += gridDim.x) {
        const u64 r = list[li];
        const u64 start = rs_start(ends, r), len = ends[r] - start, at = obase[r];
        for (u64 i = threadIdx.x; i < len; i += 256u) out[at + i] = s[start + i];
        if (threadIdx.x == 0) out[at + len] = 0x0A;
    }
}
