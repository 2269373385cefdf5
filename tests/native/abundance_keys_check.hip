// Host-side check of the key arithmetic of the table's by-value readers
// (kmer_internal.hpp: tab_planar_code2, tab_entry_keys), for every k in 1..32
// (narrow keys, k <= 21, and wide keys):
//   tab_code2_planar(tab_planar_code2(c)) == c, and tab_planar_code2 of a
//   k-mer's planar code is the matcher's 2-bit code of its bytes;
//   tab_entry_keys(h) of a class's table key h names the Map keys that the
//   string route names: decode h to the strings key and rc key, compare the
//   prefix as bytes, compare key < rc key as strings (the loop body of
//   build_table_result), in table mode and in canonical mode.
// Random classes plus hand-made ones: all-A / all-T, AT-repeats (palindromes
// at even k), every middle base (odd narrow k picks the orientation by it),
// keys of the form A...T (both orientations start with A); prefixes that are a
// prefix of the key, of its reverse complement, of both or of neither.
// Built and run by tests/test_abundance_keys.py.
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

static std::string planar_str(uint64_t c, uint32_t k) {
    std::string x(k, 'A');
    for (uint32_t j = 0; j < k; ++j) x[j] = "ACGT"[(((c >> (k + j)) & 1u) << 1) | ((c >> j) & 1u)];
    return x;
}

static bool starts(const std::string &x, const std::string &p) { return x.compare(0, p.size(), p) == 0; }

int main() {
    std::mt19937_64 g(17);
    long bad = 0, n = 0, both = 0, neither = 0, pals = 0, one = 0;
    for (uint32_t k = 1; k <= 32; ++k) {
        std::vector<std::string> keys;
        keys.push_back(std::string(k, 'A'));
        keys.push_back(std::string(k, 'T'));
        keys.push_back(std::string(k, 'C'));
        std::string at(k, 'A'), ta(k, 'T');
        for (uint32_t j = 1; j < k; j += 2) at[j] = 'T', ta[j] = 'A';
        keys.push_back(at);
        keys.push_back(ta);
        const uint64_t mask = k >= 32 ? ~0ull : ((1ull << (2 * k)) - 1);
        for (int it = 0; it < 400; ++it) keys.push_back(unpack2(g() & mask, k));
        for (int it = 0; it < 64; ++it) {                       // every middle base; A...T
            std::string x = unpack2(g() & mask, k);
            x[k / 2] = "ACGT"[it & 3];
            if (it & 4) x[0] = 'A', x[k - 1] = 'T';
            keys.push_back(x);
        }
        for (int it = 0; it < 32 && k % 2 == 0; ++it) {         // random palindromes
            std::string x = unpack2(g() & mask, k), r = rc_of(x);
            for (uint32_t j = k / 2; j < k; ++j) x[j] = r[j];
            keys.push_back(x);
        }
        for (const std::string &x : keys) {
            const std::string r = rc_of(x);
            uint64_t cf = 0, cr = 0, h = 0;
            bool ok = tab_bytes_h((const uint8_t *)x.data(), k, &cf, &cr, &h);
            // the 2-bit code and back
            uint64_t bf = 0, br = 0;
            const uint64_t c2 = tab_planar_code2(cf, k);
            tab_code2_planar(c2, k, &bf, &br);
            ok = ok && c2 == pack2(x) && bf == cf && br == cr && tab_planar_code2(cr, k) == pack2(r);
            // the string route from h
            const std::string key = planar_str(tab_code(h, k, k <= TAB_NARROW_K, TAB_INV), k), rkey = rc_of(key);
            ok = ok && ((key == x && rkey == r) || (key == r && rkey == x));
            const bool pal = key == rkey;
            pals += pal;
            std::vector<std::string> prefixes = {""};
            for (uint32_t p = 1; p <= k && p <= 5; ++p) {
                prefixes.push_back(key.substr(0, p));
                prefixes.push_back(rkey.substr(0, p));
                prefixes.push_back(unpack2(g() & ((1ull << (2 * p)) - 1), p));
            }
            if (k > 6) prefixes.push_back(key.substr(0, k - 1)), prefixes.push_back(rkey);
            for (const std::string &P : prefixes) {
                uint32_t plo = 0, phi = 0;
                for (size_t i = 0; i < P.size(); ++i) {
                    const uint8_t ch = (uint8_t)P[i];
                    plo |= ((((uint32_t)ch >> 1) ^ ((uint32_t)ch >> 2)) & 1u) << i;
                    phi |= (((uint32_t)ch >> 2) & 1u) << i;
                }
                const uint32_t pmask = P.size() >= 32 ? ~0u : ((1u << P.size()) - 1u);
                for (int canonical = 0; canonical < 2; ++canonical) {
                    ++n;
                    std::vector<std::string> want;
                    bool wdbl = false;
                    if (canonical) {
                        const std::string &ck = key < rkey ? key : rkey;
                        if (starts(ck, P)) want.push_back(ck);
                    } else {
                        if (starts(key, P)) want.push_back(key);
                        if (!pal && starts(rkey, P)) want.push_back(rkey);
                        wdbl = pal;
                    }
                    uint64_t out[2] = {0, 0};
                    bool dbl = true;
                    const uint32_t m = tab_entry_keys(h, k, plo, phi, pmask, canonical != 0, out, &dbl);
                    bool same = ok && m == want.size() && dbl == wdbl;
                    for (uint32_t i = 0; i < m && same; ++i)
                        same = planar_str(out[i], k) == want[i] && unpack2(tab_planar_code2(out[i], k), k) == want[i];
                    both += !canonical && want.size() == 2;
                    one += want.size() == 1;
                    neither += want.empty();
                    if (!same && bad++ < 5) printf("k %u key %s prefix '%s' canonical %d\n", k, x.c_str(), P.c_str(), canonical);
                }
            }
        }
    }
    printf("cases: %ld with both orientations, %ld with one key, %ld with none, %ld palindromes\n", both, one, neither, pals);
    if (!both || !one || !neither || !pals) bad += 1;            // (the hand-made cases must be there)
    printf("abundance keys: %ld of %ld mismatches\n", bad, n);
    return bad != 0;
}
