"""The 128-bit comparison of the erroneous-connection rule (dsk_amd/csrc/ratio128.h) as plain C++ on the host: a small stand-alone program,
compiled here with one g++ command, checks ratio128_greater and ratio128_mulhi against unsigned __int128 on the edge values, on equal
products, on products that differ in one half only and on seeded random operands, in the documented ranges (S[w] < 2^63, L[u] < 2^16,
min_ratio * S[u] < 2^56, L[w] < 2^31) and over all 64 bits.  No small input of the device tests reaches abundances whose products need
the high halves; this test does."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include "ratio128.h"

typedef unsigned __int128 u128;
static unsigned long long n_checked = 0, n_wrong = 0, n_true = 0, n_high = 0;

static void check(uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
    const u128 l = (u128)a * b, r = (u128)c * d;
    const bool want = l > r, got = ratio128_greater(a, b, c, d);
    const bool hi_ok = ratio128_mulhi(a, b) == (uint64_t)(l >> 64) && ratio128_mulhi(c, d) == (uint64_t)(r >> 64);
    ++n_checked; n_true += want; n_high += (l >> 64) != 0 || (r >> 64) != 0;
    if (want != got || !hi_ok) {
        if (n_wrong++ < 8) std::printf("wrong: %llu * %llu > %llu * %llu: want %d got %d, high halves %s\n", (unsigned long long)a, (unsigned long long)b,
                                       (unsigned long long)c, (unsigned long long)d, (int)want, (int)got, hi_ok ? "ok" : "differ");
    }
}

static uint64_t state = 0x9E3779B97F4A7C15ull;                               // splitmix64, seeded: the same operands on every run
static uint64_t next() {
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main() {
    const uint64_t one = 1;
    const uint64_t edge[] = {0, 1, 2, 255, 65535, (one << 31) - 1, (one << 32) - 1, one << 32, (one << 32) + 1, (one << 48) - 1, (one << 56) - 1,
                             (one << 63) - 1, one << 63, ~(uint64_t)0};
    const int n_edge = (int)(sizeof(edge) / sizeof(edge[0]));
    for (int i = 0; i < n_edge; ++i) for (int j = 0; j < n_edge; ++j) for (int p = 0; p < n_edge; ++p) for (int q = 0; q < n_edge; ++q)
        check(edge[i], edge[j], edge[p], edge[q]);
    // equal products, and products that differ in the high half only or in the low half only
    for (int i = 0; i < n_edge; ++i) for (int j = 0; j < n_edge; ++j) {
        check(edge[i], edge[j], edge[j], edge[i]);
        if (edge[i] < (one << 63) && edge[j] < (one << 63)) check(2 * edge[i], edge[j], edge[i], 2 * edge[j]);
    }
    check(one << 33, one << 32, one << 32, one << 32); check(one << 32, one << 32, one << 33, one << 32);      // 2^65 against 2^64: the low halves are 0
    check(one << 32, one << 32, 0, 5); check(0, 5, one << 32, one << 32);
    check((one << 32) + 1, one << 32, one << 32, one << 32); check(one << 32, one << 32, (one << 32) + 1, one << 32);      // the high halves are 1
    check((one << 63) - 1, 65535, ((one << 56) - 1), (one << 31) - 1); check(((one << 56) - 1), (one << 31) - 1, (one << 63) - 1, 65535);
    for (int i = 0; i < 4000; ++i) {                                           // the documented ranges: S[w] * L[u] > (min_ratio * S[u]) * L[w]
        const uint64_t Sw = next() >> (1 + next() % 63), Lu = 1 + next() % 65535, rSu = next() >> (8 + next() % 56), Lw = 1 + (next() >> 33) % ((one << 31) - 1);
        check(Sw, Lu, rSu, Lw);
    }
    for (int i = 0; i < 4000; ++i) check(next(), next(), next(), next());      // all 64 bits
    for (int i = 0; i < 4000; ++i) {                                           // next to each other: equal, one more, one less
        const uint64_t a = next() >> (next() % 40), b = next() >> (next() % 40);
        check(a, b, b, a); check(a, b, b, a + 1); check(a, b + 1, b, a); check(a, b, b + 1, a + 1);
        if (a) { check(a, b, b, a - 1); check(a - 1, b, b, a); }
    }
    std::printf("checked %llu comparisons, %llu true, %llu with a product of 2^64 or more, %llu wrong\n", n_checked, n_true, n_high, n_wrong);
    return n_wrong ? 1 : 0;
}
"""


def test_the_comparison_agrees_with_int128(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("this test needs g++")
    src, exe = tmp_path / "ratio128_check.cpp", tmp_path / "ratio128_check"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "dsk_amd", "csrc"), "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    last = out.stdout.strip().split("\n")[-1].split()
    assert last[0] == "checked" and int(last[1]) > 60000 and last[-2] == "0"
    assert 0 < int(last[3]) < int(last[1]) and int(last[5]) > 10000          # both answers occur, and the high halves are exercised
