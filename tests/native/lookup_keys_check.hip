// Host-side check of the lookup's key arithmetic (kmer_internal.hpp:
// tab_bytes_h, tab_str_le), for every k in 1..32: from the k bytes of a key x,
// h followed by tab_code and the planar decode the host result uses gives back
// x or rc x; x and rc x give the same h; two different classes give different
// h; for k <= 21 the low 23 bits of h are 0; tab_str_le is the string order
// of x and rc x.  Random k-mers plus all-A, all-T, AT-repeats (palindromes at
// even k) and, at odd k, every middle base in a fixed frame; a key with a byte
// other than A/C/G/T is refused.  Built and run by tests/test_lookup_keys.py.
#include "kmer_internal.hpp"
#include <algorithm>
#include <cstdio>
#include <map>
#include <random>
#include <string>
#include <vector>
using namespace kmerhip;

static std::string rc_of(const std::string &x) {
    std::string r(x.rbegin(), x.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    return r;
}

// the planar decode of build_table_result
static std::string decode(uint64_t code, uint32_t k) {
    const uint64_t kmask = k >= 32 ? 0xFFFFFFFFull : ((1ull << k) - 1);
    const uint64_t lo = code & kmask, hi = (code >> k) & kmask;
    std::string key(k, 'A');
    for (uint32_t j = 0; j < k; ++j) key[j] = "ACGT"[(uint32_t)(((hi >> j) & 1u) << 1 | ((lo >> j) & 1u))];
    return key;
}

int main() {
    std::mt19937_64 g(7);
    long bad = 0, n = 0;
    for (uint32_t k = 1; k <= 32; ++k) {
        std::vector<std::string> keys;
        keys.push_back(std::string(k, 'A'));
        keys.push_back(std::string(k, 'T'));
        keys.push_back(std::string(k, 'C'));
        std::string at(k, 'A'), ta(k, 'T');
        for (uint32_t j = 1; j < k; j += 2) at[j] = 'T', ta[j] = 'A';
        keys.push_back(at);
        keys.push_back(ta);
        if (k & 1)
            for (char m : {'A', 'C', 'G', 'T'}) {
                std::string x(k, 'G');
                x[k / 2] = m;
                keys.push_back(x);
                x = at;
                x[k / 2] = m;
                keys.push_back(x);
            }
        for (int it = 0; it < 3000; ++it) {
            std::string x(k, 'A');
            const uint64_t r = g(), r2 = g();
            for (uint32_t j = 0; j < k; ++j) x[j] = "ACGT"[((j < 16 ? r >> (2 * j) : r2 >> (2 * (j - 16))) & 3)];
            keys.push_back(x);
        }
        std::map<uint64_t, std::string> seen;   // h -> the class's smaller string
        for (const std::string &x : keys) {
            ++n;
            const std::string r = rc_of(x);
            uint64_t cf, cr, h, cf2, cr2, h2;
            bool ok = tab_bytes_h((const uint8_t *)x.data(), k, &cf, &cr, &h);
            ok = ok && tab_bytes_h((const uint8_t *)r.data(), k, &cf2, &cr2, &h2);
            ok = ok && h == h2 && cf == cr2 && cr == cf2 && decode(cf, k) == x && decode(cr, k) == r;
            const std::string back = decode(tab_code(h, k, k <= TAB_NARROW_K, TAB_INV), k);
            ok = ok && (back == x || back == r);
            if (k <= TAB_NARROW_K) ok = ok && (h & ((1ull << TAB_NSH) - 1)) == 0;
            ok = ok && tab_str_le(cf, cr, k) == (x <= r) && tab_str_le(cr, cf, k) == (r <= x);
            const std::string cls = std::min(x, r);
            const auto it = seen.find(h);
            if (it == seen.end()) seen.emplace(h, cls);
            else ok = ok && it->second == cls;         // (equal h: the same class)
            if (!ok && bad++ < 5) printf("k %u key %s\n", k, x.c_str());
        }
        // the same class never under two h: as many h as classes
        std::vector<std::string> classes;
        for (auto &kv : seen) classes.push_back(kv.second);
        std::sort(classes.begin(), classes.end());
        ++n;
        if (std::adjacent_find(classes.begin(), classes.end()) != classes.end() && bad++ < 5) printf("k %u: a class with two h\n", k);
        // a byte that is none of A/C/G/T is refused, wherever it stands
        for (char c : {'N', 'a', '\r', 'B'})
            for (uint32_t pos : {0u, k / 2, k - 1}) {
                std::string x = keys.back();
                x[pos] = c;
                uint64_t cf, cr, h;
                ++n;
                if (tab_bytes_h((const uint8_t *)x.data(), k, &cf, &cr, &h) && bad++ < 5) printf("k %u accepted %s\n", k, x.c_str());
            }
    }
    printf("lookup keys: %ld of %ld bad\n", bad, n);
    return bad != 0;
}
