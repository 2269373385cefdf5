// Host-side check of the plane scan's line context (kmer_internal.hpp:
// region_line_context) against a byte-by-byte model.
//   1. The function itself: every qrel 0..63 over structured masks (empty,
//      full, single bits at 0, 62 and 63, CRLF pairs) and a few thousand random
//      ones, pre in {0, 1, 65535}, prevnl in {-1, 0, 16383 - 64}; the model
//      walks the region's bytes.
//   2. The identity the kernel rests on: a window that becomes a hit record
//      holds no '\n' and holds the candidate position q (q = s0 on the forward
//      strand, s0 + k - plen on the reverse), so the context at q, taken from
//      the 64-byte region that holds q, is the context at the window start s0
//      as the scan defines it (s0 <= 0: count 0, no line start) -- for every
//      valid window of random tiles at k 5, 16, 32 and 64.
// Built and run by tests/test_scan_line_context.py.
#include "kmer_internal.hpp"
#include <cstdio>
#include <random>
#include <vector>
using namespace kmerhip;

// the model: '\n' count of bytes [0, pos) and one past the last of them (-1: none)
static void model_at(const uint8_t *tile, int pos, uint32_t *cnt, int32_t *lstart) {
    uint32_t c = 0;
    int32_t l = -1;
    for (int p = 0; p < pos; ++p)
        if (tile[p] == '\n') {
            ++c;
            l = p + 1;
        }
    *cnt = c;
    *lstart = l;
}

static long bad = 0, n = 0;

static void check_mask(uint64_t mask) {
    const uint32_t pres[] = {0u, 1u, 65535u};
    const int32_t prevs[] = {-1, 0, 16383 - 64};
    uint8_t region[64];
    for (int i = 0; i < 64; ++i) region[i] = (mask >> i) & 1 ? '\n' : "ACGT\r@+I"[i & 7];
    for (uint32_t pre : pres)
        for (int32_t prevnl : prevs) {
            const int32_t base = prevnl < 0 ? 0 : prevnl == 0 ? 64 : 16384 - 64;   // a region behind prevnl
            for (uint32_t qrel = 0; qrel < 64; ++qrel) {
                uint32_t mc, gc;
                int32_t ml, gl;
                model_at(region, (int)qrel, &mc, &ml);
                const uint32_t want_c = pre + mc;
                const int32_t want_l = ml >= 0 ? base + ml : prevnl >= 0 ? prevnl + 1 : -1;
                region_line_context(pre, prevnl, mask, qrel, base, &gc, &gl);
                ++n;
                if ((gc != want_c || gl != want_l) && bad++ < 8)
                    printf("mask %016llx pre %u prevnl %d qrel %u: c_local %u (model %u) lstart %d (model %d)\n",
                           (unsigned long long)mask, pre, prevnl, qrel, gc, want_c, gl, want_l);
            }
        }
}

int main() {
    std::mt19937_64 g(5);
    // ---- 1. the function ----
    std::vector<uint64_t> masks = {0ull, ~0ull, 1ull, 1ull << 62, 1ull << 63, 3ull, 3ull << 62,
                                   (1ull << 63) | 1ull, 1ull << 31, 1ull << 32, 3ull << 31};
    for (int i = 0; i < 63; ++i) masks.push_back(2ull << i);                      // CRLF: "\r\n" with '\n' at i + 1
    for (int i = 0; i + 3 < 64; ++i) masks.push_back((2ull << i) | (8ull << i));  // two CRLF pairs (a blank line)
    for (int it = 0; it < 3000; ++it) {
        uint64_t m = g();
        for (int s = (int)(g() % 6); s > 0; --s) m &= g();                         // dense to sparse
        masks.push_back(m);
    }
    for (uint64_t m : masks) check_mask(m);
    const long n1 = n;

    // ---- 2. context at q == context at s0, every valid window ----
    const int FRONT = 64;                        // bytes in front of the tile (a window may start there)
    long windows = 0, neg = 0, sameline = 0, nonl_before = 0;
    for (int t = 0; t < 6; ++t) {
        std::vector<uint8_t> store(FRONT + TILE + 80);
        uint8_t *tile = store.data() + FRONT;
        const int rate = t == 0 ? 0 : t == 1 ? 9000 : t == 2 ? 150 : t == 3 ? 40 : t == 4 ? 6 : 2;   // bytes per '\n'
        for (int p = -FRONT; p < TILE + 80; ++p)
            tile[p] = rate && g() % (uint64_t)rate == 0 ? (uint8_t)'\n' : (uint8_t)"ACGT"[g() & 3];
        if (t == 1) tile[-1] = tile[0] = tile[63] = tile[64] = tile[65] = tile[4095] = tile[4096] = tile[TILE - 1] = '\n';
        // per position: '\n' count before it and one past the last '\n' before it (the model, incrementally)
        std::vector<uint32_t> cnt(TILE + 1);
        std::vector<int32_t> lst(TILE + 1);
        {
            uint32_t c = 0;
            int32_t l = -1;
            for (int p = 0; p <= TILE; ++p) {
                cnt[p] = c;
                lst[p] = l;
                if (p < TILE && tile[p] == '\n') {
                    ++c;
                    l = p + 1;
                }
            }
            uint32_t mc;
            int32_t ml;
            model_at(tile, 777, &mc, &ml);       // (the incremental form is the model)
            if (mc != cnt[777] || ml != lst[777]) return 2;
        }
        const uint32_t ks[] = {5, 16, 32, 64};
        for (uint32_t k : ks) {
            const int plen = 5;
            for (int strand = 0; strand < 2; ++strand)
                for (int q = 0; q < TILE; ++q) {
                    const int s0 = strand ? q + plen - (int)k : q;
                    bool hasnl = false;
                    for (int b = 0; b < (int)k; ++b) hasnl |= tile[s0 + b] == '\n';
                    if (hasnl) continue;
                    // what the scan asks for: the context of the window start
                    const uint32_t want_c = s0 > 0 ? cnt[s0] : 0u;
                    const int32_t want_l = s0 > 0 ? lst[s0] : -1;
                    // what the finding thread has: its region's bytes, the count and the last '\n' before it
                    const int base = q & ~63;
                    uint64_t mask = 0;
                    for (int i = 0; i < 64; ++i) mask |= (uint64_t)(tile[base + i] == '\n') << i;
                    uint32_t gc;
                    int32_t gl;
                    region_line_context(cnt[base], lst[base] - (lst[base] >= 0 ? 1 : 0), mask, (uint32_t)(q & 63), base, &gc,
                                        &gl);
                    ++n;
                    ++windows;
                    neg += s0 <= 0;
                    sameline += want_l >= 0;
                    nonl_before += want_l < 0;
                    if ((gc != want_c || gl != want_l) && bad++ < 16)
                        printf("tile %d k %u strand %d q %d s0 %d: c_local %u (model %u) lstart %d (model %d)\n", t, k, strand,
                               q, s0, gc, want_c, gl, want_l);
                }
        }
    }
    if (!windows || !neg || !sameline || !nonl_before) {
        printf("the tiles do not cover windows (%ld), s0 <= 0 (%ld), a line start inside (%ld) and none (%ld)\n", windows, neg,
               sameline, nonl_before);
        return 1;
    }
    printf("scan line context: %ld of %ld bad (%ld function cases, %ld windows)\n", bad, n, n1, windows);
    return bad != 0;
}
