// superkmer_recv.h -- the receiving side of the super-k-mer records (superkmer.h): records -> k-mer counts per chunk, -> a dense array of
// mixed keys, -> a positional sample as a key array with pads.  Include after kernels.h (KeyT, empty_key, sk_key).  k_sk_count is no
// template: one translation unit only (dskgpu.hip).
#pragma once
#include "superkmer.h"

// ---------------------------------------------------------------- receiver: k-mers per chunk of records
#define SKX_NT 256
__global__ __launch_bounds__(SKX_NT) void k_sk_count(const u64* __restrict__ rec, u64 nrec, u32 R, u32 rpc, u32* __restrict__ sums) {
    __shared__ u32 ws[SKX_NT / 64];
    const u64 rbeg = (u64)blockIdx.x * rpc;
    const u64 rend = rbeg + rpc < nrec ? rbeg + rpc : nrec;
    u32 s = 0;
    for (u64 r = rbeg + threadIdx.x; r < rend; r += SKX_NT) s += (u32)(rec[r * R + R - 1] & 0xFFu);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) { u32 t = 0; for (int i = 0; i < SKX_NT / 64; ++i) t += ws[i]; sums[blockIdx.x] = t; }
}

// ---------------------------------------------------------------- receiver: records -> dense mixed keys
// One block per chunk of records.  A tile of SKX_NT records is staged in LDS together with a slot map
// (output slot -> record, k-mer index), then every thread builds ONE k-mer per trip straight from the
// staged bases (a funnel shift + rev_pairs; no rolling, no idle lanes) and stores it coalesced.
template <int W>
__global__ __launch_bounds__(SKX_NT) void k_sk_expand(const u64* __restrict__ rec, u64 nrec, u32 R, int k, u32 rpc,
                                                      const u64* __restrict__ chunk_base, typename KeyT<W>::T* __restrict__ out) {
    __shared__ u64 srec[SKX_NT * 3];
    __shared__ unsigned short smap[SKX_NT * SK_MAXN];
    __shared__ u32 wsum[SKX_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 rbeg = (u64)blockIdx.x * rpc;
    const u64 rend = rbeg + rpc < nrec ? rbeg + rpc : nrec;
    u64 obase = chunk_base[blockIdx.x];
    for (u64 r0 = rbeg; r0 < rend; r0 += SKX_NT) {
        const u64 r = r0 + tid;
        u32 n = 0;
        if (r < rend) {
            const u64* p = rec + r * R;
            const u64 a = p[0], b = p[1], c = (R == 3) ? p[2] : 0ull;
            srec[tid * 3] = a; srec[tid * 3 + 1] = b; srec[tid * 3 + 2] = c;
            n = (u32)((R == 3 ? c : b) & 0xFFu);
        }
        u32 inc = n;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const u32 v = __shfl_up(inc, d); if (lane >= d) inc += v; }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        u32 off = inc - n, total = 0;
#pragma unroll
        for (int x = 0; x < SKX_NT / 64; ++x) { const u32 v = wsum[x]; if (x < wave) off += v; total += v; }
        for (u32 j = 0; j < n; ++j) smap[off + j] = (unsigned short)((tid << 5) | j);
        __syncthreads();
        for (u32 i = tid; i < total; i += SKX_NT) {
            const u32 e = smap[i];
            const u64* rr = srec + (e >> 5) * 3;
            if (W == 1) reinterpret_cast<u64*>(out)[obase + i] = sk_key1(rr, (int)(e & 31u), k);
            else reinterpret_cast<K2*>(out)[obase + i] = sk_key2(rr, (int)(e & 31u), k);
        }
        obase += total;
        __syncthreads();
    }
}

// ---------------------------------------------------------------- receiver: a positional SAMPLE of the records as a key array
// Sample chunk c = the records [cbeg[c], cbeg[c] + nr) (nr candidates, as a level-1 tile takes them); every candidate gets 16 key
// slots in out[(c * nr + i) * SK_MAXN ..], filled with its k-mers' mixed keys and, behind them (and for candidates past the end of the
// records), the all-ones sentinel -- a key array with pads, which the histogram / heavy-k-mer kernels of the key-array source read
// as it is (tile_keys_array masks the pads).  The level-1 slices of the receive side are sized from it, per bin.
template <int W>
__global__ __launch_bounds__(SKX_NT) void k_sk_sample_keys(const u64* __restrict__ rec, u64 nrec, u32 R, int k, const u64* __restrict__ cbeg, u32 nr,
                                                           typename KeyT<W>::T* __restrict__ out) {
    typedef typename KeyT<W>::T Key;
    const u64 r0 = cbeg[blockIdx.x];
    Key* o = out + (u64)blockIdx.x * nr * SK_MAXN;
    for (u32 i = threadIdx.x; i < nr; i += SKX_NT) {
        const u64 r = r0 + i;
        u64 w[3] = {0ull, 0ull, 0ull};
        u32 n = 0;
        if (r < nrec) {
            const u64* p = rec + r * R;
            w[0] = p[0]; w[1] = p[1]; if (R == 3) w[2] = p[2];
            n = (u32)(w[R - 1] & 0xFFu);
            if (n > SK_MAXN) n = SK_MAXN;
        }
        for (u32 j = 0; j < SK_MAXN; ++j) {
            Key key = empty_key<W>();
            if (j < n) sk_key(w, (int)j, k, key);
            o[(u64)i * SK_MAXN + j] = key;
        }
    }
}
