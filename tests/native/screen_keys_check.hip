// Host-side check of the read screen's window arithmetic (kmer_internal.hpp:
// screen_window_codes, screen_weight) against a brute-force string model, for
// every k in 1..32, both modes and the prefixes "", "A", "GT", "ATGAC": the
// class {w, rc w}, both prefix tests, palindromes (weight 2 f, the table's
// count doubled) and, in canonical mode, the smaller string of the class.
// Windows are taken as the keys kernel takes them -- shifts of a line's bit
// planes -- so the codes and the h of every window must equal tab_bytes_h's of
// its k bytes (wide and narrow keys, odd and even k, k = 32).  Random lines
// plus constructed palindromes, all-A, all-T and AT-repeats.  Built and run by
// tests/test_screen_keys.py.
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

static bool starts(const std::string &x, const std::string &p) { return x.compare(0, p.size(), p) == 0; }

// the model: weight of a forward window w and whether the table's count is doubled
static uint32_t model(const std::string &w, const std::string &p, bool canonical, bool *dbl) {
    const std::string r = rc_of(w);
    *dbl = false;
    if (canonical) return starts(w < r ? w : r, p) ? 1u : 0u;
    if (w == r) {
        *dbl = true;
        return starts(w, p) ? 2u : 0u;
    }
    return (starts(w, p) ? 1u : 0u) + (starts(r, p) ? 1u : 0u);
}

int main() {
    std::mt19937_64 g(11);
    long bad = 0, n = 0, pal = 0, w2 = 0, w0 = 0;
    const char *prefixes[] = {"", "A", "GT", "ATGAC"};
    for (uint32_t k = 1; k <= 32; ++k) {
        // lines of k + 15 bytes: 16 windows each, as one lane of the keys kernel takes them
        std::vector<std::string> lines;
        auto rnd = [&](uint32_t len) {
            std::string x(len, 'A');
            for (char &c : x) c = "ACGT"[g() & 3];
            return x;
        };
        for (int it = 0; it < 300; ++it) lines.push_back(rnd(k + 15));
        lines.push_back(std::string(k + 15, 'A'));
        lines.push_back(std::string(k + 15, 'T'));
        std::string at(k + 15, 'A');
        for (uint32_t j = 1; j < at.size(); j += 2) at[j] = 'T';
        lines.push_back(at);
        lines.push_back(at.substr(1) + "A");
        for (int it = 0; it < 200; ++it) {                      // a palindrome at window 0 .. 15 of a random line
            const std::string half = rnd((k + 1) / 2);
            std::string p = half + rc_of(half).substr(k & 1 ? 1 : 0);   // (odd k: no palindrome exists; a near one)
            p.resize(k, 'A');
            std::string x = rnd(k + 15);
            x.replace(it % 16, k, p);
            lines.push_back(x);
        }
        for (const char *ps : prefixes) {
            const std::string P(ps);
            if (P.size() > k) continue;
            uint32_t plo = 0, phi = 0;
            for (size_t i = 0; i < P.size(); ++i) {
                const uint32_t ch = (uint8_t)P[i];
                plo |= (((ch >> 1) ^ (ch >> 2)) & 1u) << i;
                phi |= ((ch >> 2) & 1u) << i;
            }
            const uint32_t pmask = (1u << P.size()) - 1u;
            for (const std::string &x : lines) {
                uint64_t LO = 0, HI = 0;
                for (size_t j = 0; j < x.size(); ++j) {
                    const uint64_t ch = (uint8_t)x[j];
                    LO |= (((ch >> 1) ^ (ch >> 2)) & 1u) << j;
                    HI |= ((ch >> 2) & 1u) << j;
                }
                for (uint32_t m = 0; m < 16; ++m) {
                    const std::string w = x.substr(m, k);
                    uint64_t cf, cr, bf, br, bh;
                    screen_window_codes(LO, HI, m, k, &cf, &cr);
                    bool ok = tab_bytes_h((const uint8_t *)w.data(), k, &bf, &br, &bh);
                    ok = ok && cf == bf && cr == br && tab_key_h(cf, cr, k) == bh;
                    for (int canonical = 0; canonical < 2; ++canonical) {
                        ++n;
                        bool dbl, mdbl, rdbl;
                        const uint32_t got = screen_weight(cf, cr, k, plo, phi, pmask, canonical != 0, &dbl);
                        const uint32_t want = model(w, P, canonical != 0, &mdbl);
                        // the weight belongs to the class: rc w gives the same
                        const uint32_t rgot = screen_weight(cr, cf, k, plo, phi, pmask, canonical != 0, &rdbl);
                        const bool good = ok && got == want && dbl == mdbl && rgot == got && rdbl == dbl;
                        pal += mdbl ? 1 : 0;
                        w2 += want == 2 ? 1 : 0;
                        w0 += want == 0 ? 1 : 0;
                        if (!good && bad++ < 8)
                            printf("k %u prefix '%s' canonical %d window %s: weight %u (model %u) dbl %d (%d)\n", k, ps,
                                   canonical, w.c_str(), got, want, (int)dbl, (int)mdbl);
                    }
                }
            }
        }
    }
    if (!pal || !w2 || !w0) {
        printf("the cases do not cover palindromes (%ld), weight 2 (%ld) and weight 0 (%ld)\n", pal, w2, w0);
        return 1;
    }
    printf("screen keys: %ld of %ld bad\n", bad, n);
    return bad != 0;
}
