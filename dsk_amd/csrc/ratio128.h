// ratio128.h -- a * b > c * d on unsigned 64-bit operands, exactly: the comparison of the erroneous-connection rule (connections.h), whose
// products S[w] * L[u] and (min_ratio * S[u]) * L[w] reach 2^87.  Two 64 x 64 -> 128 products, compared high half first.  On the device the
// high half is __umul64hi; as plain C++ on the host (tests/test_connections_compare.py compiles it alone) it is four 32 x 32 products.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RATIO128_FN __host__ __device__ inline
#else
#define RATIO128_FN inline
#endif

RATIO128_FN uint64_t ratio128_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    const uint64_t a0 = a & 0xFFFFFFFFull, a1 = a >> 32, b0 = b & 0xFFFFFFFFull, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (p01 & 0xFFFFFFFFull) + (p10 & 0xFFFFFFFFull);      // (< 3 * 2^32: no carry is lost)
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
#endif
}

// a * b > c * d, every operand any 64-bit value
RATIO128_FN bool ratio128_greater(uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
    const uint64_t lh = ratio128_mulhi(a, b), ll = a * b, rh = ratio128_mulhi(c, d), rl = c * d;
    return lh > rh || (lh == rh && ll > rl);
}
