// Host-side check of the matcher probe's key arithmetic (kmer_internal.hpp:
// tab_code2_planar), for every k in 1..32: from the matcher's 2-bit code of a
// k-mer (first base most significant, A C G T = 0 1 2 3) it must give the
// planar codes that tab_bytes_code gives for the k-mer's bytes and for its
// reverse complement's.  Random codes plus all-A, all-T and the AT-repeats
// (palindromes at even k).  Built and run by tests/test_probe_keys.py.
#include "kmer_internal.hpp"
#include <cstdio>
#include <random>
#include <string>
#include <vector>
using namespace kmerhip;

static std::string rc_of(const std::string &x) {
    std::string r(x.rbegin(), x.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    return r;
}

// the matcher's pack_key (kmer_match.hip)
static uint64_t pack2(const std::string &x) {
    uint64_t v = 0;
    for (char c : x) v = (v << 2) | (uint64_t)(c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3);
    return v;
}

static std::string unpack2(uint64_t code, uint32_t k) {
    std::string x(k, 'A');
    for (uint32_t j = 0; j < k; ++j) x[j] = "ACGT"[(code >> (2 * (k - 1 - j))) & 3u];
    return x;
}

int main() {
    std::mt19937_64 g(11);
    long bad = 0, n = 0;
    for (uint32_t k = 1; k <= 32; ++k) {
        std::vector<std::string> keys;
        keys.push_back(std::string(k, 'A'));
        keys.push_back(std::string(k, 'T'));
        keys.push_back(std::string(k, 'C'));
        keys.push_back(std::string(k, 'G'));
        std::string at(k, 'A'), ta(k, 'T');
        for (uint32_t j = 1; j < k; j += 2) at[j] = 'T', ta[j] = 'A';
        keys.push_back(at);
        keys.push_back(ta);
        const uint64_t mask = k >= 32 ? ~0ull : ((1ull << (2 * k)) - 1);
        for (int it = 0; it < 3000; ++it) keys.push_back(unpack2(g() & mask, k));
        for (const std::string &x : keys) {
            ++n;
            const std::string r = rc_of(x);
            uint64_t cf = 0, cr = 0, wf = 0, wr = 0;
            bool ok = tab_bytes_code((const uint8_t *)x.data(), k, &wf);
            ok = ok && tab_bytes_code((const uint8_t *)r.data(), k, &wr);
            tab_code2_planar(pack2(x), k, &cf, &cr);
            ok = ok && cf == wf && cr == wr && unpack2(pack2(x), k) == x;
            if ((k % 2 == 0) && (x == at || x == ta)) ok = ok && cf == cr;   // a palindrome
            // and the other way round
            tab_code2_planar(pack2(r), k, &cf, &cr);
            ok = ok && cf == wr && cr == wf;
            if (!ok && bad++ < 5) printf("k %u key %s\n", k, x.c_str());
        }
    }
    printf("probe keys: %ld of %ld bad\n", bad, n);
    return bad != 0;
}
