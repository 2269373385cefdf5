// Host-side check of the read filter's predicate (kmer_internal.hpp:
// filter_match, filter_mul96) against unsigned __int128 brute force:
// hits >= min_hits AND hits * frac_den >= frac_num * windows.  Edge values 0,
// 1, 2^32 - 1, 2^32, 2^32 + 1, 2^63, 2^64 - 1 (and neighbours) in every
// position (hits, windows, min_hits), the fractions 0/1, 1/1, 1/2, 2/3 and
// (2^32 - 1)/(2^32 - 1), plus random values.  Built and run by
// tests/test_filter_pred.py.
#include "kmer_internal.hpp"
#include <cstdio>
#include <random>
#include <vector>
using namespace kmerhip;

typedef unsigned __int128 u128;

int main() {
    const std::vector<uint64_t> edge = {0,
                                        1,
                                        2,
                                        3,
                                        (1ull << 32) - 1,
                                        1ull << 32,
                                        (1ull << 32) + 1,
                                        (1ull << 63) - 1,
                                        1ull << 63,
                                        (1ull << 63) + 1,
                                        ~0ull - 1,
                                        ~0ull};
    const uint32_t fr[][2] = {{0, 1}, {1, 1}, {1, 2}, {2, 3}, {0xFFFFFFFFu, 0xFFFFFFFFu}, {0xFFFFFFFEu, 0xFFFFFFFFu},
                              {1, 0xFFFFFFFFu}, {0, 0xFFFFFFFFu}};
    long bad = 0, n = 0, yes = 0, no = 0, wide = 0;
    auto check = [&](uint64_t hits, uint64_t windows, uint64_t min_hits, uint32_t num, uint32_t den) {
        const u128 l = (u128)hits * den, r = (u128)num * windows;
        const bool want = hits >= min_hits && l >= r;
        const bool got = filter_match(hits, windows, min_hits, num, den);
        uint64_t hi, lo;
        filter_mul96(hits, den, &hi, &lo);
        const bool mul_ok = hi == (uint64_t)(l >> 64) && lo == (uint64_t)l;
        ++n;
        yes += want;
        no += !want;
        wide += (l >> 64) != 0 || (r >> 64) != 0;
        if ((got != want || !mul_ok) && bad++ < 8)
            printf("hits %llu windows %llu min_hits %llu frac %u/%u: %d (want %d), product %s\n",
                   (unsigned long long)hits, (unsigned long long)windows, (unsigned long long)min_hits, num, den,
                   (int)got, (int)want, mul_ok ? "ok" : "wrong");
    };
    for (auto &f : fr)
        for (uint64_t h : edge)
            for (uint64_t w : edge)
                for (uint64_t m : edge) check(h, w, m, f[0], f[1]);
    std::mt19937_64 g(7);
    for (int i = 0; i < 200000; ++i) {
        const uint64_t w = g() >> (g() & 63), h = (i & 1) ? g() >> (g() & 63) : w - (w ? g() % w : 0);
        uint32_t den = (uint32_t)(g() >> (32 + (g() & 31)));
        den = den ? den : 1;
        const uint32_t num = (uint32_t)(g() % ((uint64_t)den + 1));
        check(h, w, g() >> (g() & 63), num, den);
        check(h, w, 0, num, den);
    }
    // with min_hits = 0 and frac_num = 0 every read matches, also one without windows
    for (uint64_t h : edge)
        for (uint64_t w : edge)
            if (!filter_match(h, w, 0, 0, 1) || !filter_match(h, w, 0, 0, 0xFFFFFFFFu)) ++bad;
    if (!yes || !no || !wide) {
        printf("the cases do not cover matches (%ld), misses (%ld) and products past 64 bits (%ld)\n", yes, no, wide);
        return 1;
    }
    printf("filter predicate: %ld of %ld bad\n", bad, n);
    return bad != 0;
}
