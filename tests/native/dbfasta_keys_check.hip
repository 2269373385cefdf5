// Host-side check of "the keys of a window" of the FASTA route to a template
// DB (kmer_internal.hpp: dbf_window_keys over screen_window_codes) against a
// brute-force string model, for every k in 1..32, both modes and prefixes of
// length 0, 1, 5 and k: the emitted 2-bit codes (the matcher's: first base
// most significant, A C G T = 0 1 2 3) and their number.  Not canonical: w if
// it starts with the prefix, rc w if it does -- a self-complementary window
// gives its key twice.  Canonical: the smaller string of {w, rc w} if it
// starts with the prefix.  Windows: every window of length k for k <= 6 (all
// palindromes there are), random windows, constructed palindromes, the
// k-long prefixes themselves and their reverse complements.  Windows are taken
// as the kernel takes them: shifts of a line's bit planes.  Built and run by
// tests/test_dbfasta_keys.py.
#include "kmer_internal.hpp"
#include <algorithm>
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

static bool starts(const std::string &x, const std::string &p) {
    return p.size() <= x.size() && x.compare(0, p.size(), p) == 0;
}

static uint64_t code2(const std::string &x) {
    uint64_t v = 0;
    for (char c : x) v = (v << 2) | (uint64_t)(c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3);
    return v;
}

// the model: the keys of forward window w, as 2-bit codes (sorted)
static std::vector<uint64_t> model(const std::string &w, const std::string &p, bool canonical) {
    const std::string r = rc_of(w);
    std::vector<uint64_t> out;
    if (canonical) {
        const std::string &s = w < r ? w : r;
        if (starts(s, p)) out.push_back(code2(s));
    } else {
        if (starts(w, p)) out.push_back(code2(w));
        if (starts(r, p)) out.push_back(code2(r));
    }
    std::sort(out.begin(), out.end());
    return out;
}

int main() {
    std::mt19937_64 g(23);
    long bad = 0, n = 0, pal = 0, two = 0, twice = 0, none = 0;
    auto rnd = [&](uint32_t len) {
        std::string x(len, 'A');
        for (char &c : x) c = "ACGT"[g() & 3];
        return x;
    };
    for (uint32_t k = 1; k <= 32; ++k) {
        std::vector<std::string> prefixes = {"", "A", "T"};
        if (k >= 5) prefixes.push_back("ATGAC");
        const std::string pk = rnd(k);
        prefixes.push_back(pk);
        std::string ppal = rnd((k + 1) / 2);
        ppal = ppal + rc_of(ppal).substr(k & 1 ? 1 : 0);             // (odd k: no palindrome exists; a near one)
        ppal.resize(k, 'A');
        prefixes.push_back(ppal);
        std::vector<std::string> wins;
        if (k <= 6) {
            for (uint32_t v = 0; v < (1u << (2 * k)); ++v) {
                std::string x(k, 'A');
                for (uint32_t j = 0; j < k; ++j) x[j] = "ACGT"[(v >> (2 * (k - 1 - j))) & 3];
                wins.push_back(x);
            }
        }
        for (int it = 0; it < 400; ++it) wins.push_back(rnd(k));
        for (int it = 0; it < 100; ++it) {
            const std::string half = rnd((k + 1) / 2);
            std::string p = half + rc_of(half).substr(k & 1 ? 1 : 0);
            p.resize(k, 'A');
            wins.push_back(p);
        }
        for (int it = 0; it < 50 && k >= 5; ++it) wins.push_back("ATGAC" + rnd(k - 5));
        for (int it = 0; it < 50 && k >= 5; ++it) wins.push_back(rc_of("ATGAC" + rnd(k - 5)));
        wins.push_back(pk);
        wins.push_back(rc_of(pk));
        wins.push_back(ppal);
        wins.push_back(std::string(k, 'A'));
        wins.push_back(std::string(k, 'T'));
        for (const std::string &P : prefixes) {
            uint32_t plo = 0, phi = 0;
            for (size_t i = 0; i < P.size(); ++i) {
                const uint32_t ch = (uint8_t)P[i];
                plo |= (((ch >> 1) ^ (ch >> 2)) & 1u) << i;
                phi |= ((ch >> 2) & 1u) << i;
            }
            const uint32_t pmask = P.size() >= 32 ? ~0u : ((1u << P.size()) - 1u);
            for (size_t wi = 0; wi < wins.size(); ++wi) {
                // the window at offset m of a line, as a lane sees it
                const uint32_t m = (uint32_t)(wi % 16);
                const std::string x = rnd(m) + wins[wi] + rnd(15 - m);
                uint64_t LO = 0, HI = 0;
                for (size_t j = 0; j < x.size(); ++j) {
                    const uint64_t ch = (uint8_t)x[j];
                    LO |= (((ch >> 1) ^ (ch >> 2)) & 1u) << j;
                    HI |= ((ch >> 2) & 1u) << j;
                }
                uint64_t cf, cr;
                screen_window_codes(LO, HI, m, k, &cf, &cr);
                const std::string &w = wins[wi];
                for (int canonical = 0; canonical < 2; ++canonical) {
                    ++n;
                    uint64_t keys[2] = {~0ull, ~0ull};
                    const uint32_t c = dbf_window_keys(cf, cr, k, plo, phi, pmask, canonical != 0, keys);
                    std::vector<uint64_t> got(keys, keys + (c <= 2 ? c : 0));
                    std::sort(got.begin(), got.end());
                    const std::vector<uint64_t> want = model(w, P, canonical != 0);
                    bool dbl;
                    const bool good = c <= 2 && got == want &&
                                      c == screen_weight(cf, cr, k, plo, phi, pmask, canonical != 0, &dbl);
                    pal += w == rc_of(w) ? 1 : 0;
                    two += want.size() == 2 && want[0] != want[1] ? 1 : 0;
                    twice += want.size() == 2 && want[0] == want[1] ? 1 : 0;
                    none += want.empty() ? 1 : 0;
                    if (!good && bad++ < 8)
                        printf("k %u prefix '%s' canonical %d window %s: %u keys (model %zu)\n", k, P.c_str(), canonical,
                               w.c_str(), c, want.size());
                }
            }
        }
    }
    if (!pal || !two || !twice || !none) {
        printf("the cases do not cover palindromes (%ld), two keys (%ld), one key twice (%ld) and no key (%ld)\n", pal,
               two, twice, none);
        return 1;
    }
    printf("dbfasta keys: %ld of %ld bad\n", bad, n);
    return bad != 0;
}
