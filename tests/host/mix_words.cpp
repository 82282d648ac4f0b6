// mix_words.cpp -- test infrastructure: the key mixers of dsk_amd/csrc/kmer_device.h compiled for the HOST (the functions are
// __host__ __device__; no kernel, no device call), as a filter.  Every input line holds a key as hex words, `W w0 .. w(W-1)` (W = 1,
// 2 or 4 words, least significant first); the output line is the mixed top word, the 64 bits every digit, table slot and lookup
// fingerprint of that key are taken from.  tests/test_crafted_keys_restatement.py pins the Python restatement of the mixers
// (tests/crafted_keys.py) to the header with it.
#include <cstdio>
#include "../../dsk_amd/csrc/kmer_device.h"

template <int W> static u64 top_of(const u64* w) { KN<W> x; for (int i = 0; i < W; ++i) x.w[i] = w[i]; kmixN(x); return x.w[W - 1]; }

int main() {
    int W;
    while (scanf("%d", &W) == 1) {
        u64 w[4] = {0, 0, 0, 0};
        if (W != 1 && W != 2 && W != 4) { fprintf(stderr, "mix_words: W = %d\n", W); return 2; }
        for (int i = 0; i < W; ++i) if (scanf("%llx", &w[i]) != 1) { fprintf(stderr, "mix_words: short line\n"); return 2; }
        const u64 h = W == 1 ? kmix(w[0]) : W == 2 ? top_of<2>(w) : top_of<4>(w);
        printf("%016llx\n", h);
    }
    return 0;
}
