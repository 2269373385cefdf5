// Host model of the long-pair join of two buckets (kmer_setops.hip), built
// only from the __host__ __device__ helpers of kmer_internal.hpp: the first
// split depth (join_depth0), the range of a remainder (join_sig / join_sub),
// the depth-first order of the ranges (join_next; a range with more than
// JOIN_TILE staged entries is halved) and the slot hash (join_slot) with
// linear probing in the join_slots(entries) first slots of an array of
// JOIN_SLOTS, 0 = empty.
// Remainder sets of 0, 1, tile - 1, tile, tile + 1 and 5 x tile entries on
// each side, as
//   uniform 44-bit remainders,
//   remainders whose top 14 bits are equal (the split must deepen),
//   narrow remainders (low 23 bits zero: the significant bits are the top 21),
//   two identical sides, and two disjoint sides.
// The model must end, stage every S entry and probe every P entry exactly
// once, never hold more than JOIN_TILE entries in the slots, and its
// intersection, A-only and B-only sets must equal a std::set join.
// Built and run by tests/test_setops_keys.py.
#include "kmer_internal.hpp"
#include <algorithm>
#include <cstdio>
#include <random>
#include <set>
#include <vector>
using namespace kmerhip;

struct Joined {
    std::set<uint64_t> both, p_only, s_only;
    bool ok = true;
    uint32_t max_depth = 0;
    uint64_t ranges = 0;
};

// P probes S: what the kernel's wave does for one pair of buckets
static Joined model(const std::vector<uint64_t> &S, const std::vector<uint64_t> &P, bool narrow) {
    Joined r;
    const uint32_t W = join_width(narrow);
    std::vector<uint64_t> slots(JOIN_SLOTS);
    std::vector<uint8_t> staged(S.size(), 0), hit(S.size(), 0), probed(P.size(), 0);
    const uint32_t s0 = join_depth0(S.size());
    uint32_t s = s0;
    uint64_t t = 0;
    for (uint64_t guard = 0;; ++guard) {
        if (guard > (1u << 22)) {                                  // it must terminate
            r.ok = false;
            break;
        }
        uint64_t cs = 0;
        for (uint64_t x : S) cs += join_sub(join_sig(x, narrow), W, s) == t;
        if (cs > JOIN_TILE) {
            if (s >= W) {                                          // distinct remainders: never
                r.ok = false;
                break;
            }
            ++s;
            t <<= 1;
            continue;
        }
        ++r.ranges;
        r.max_depth = std::max(r.max_depth, s);
        const uint32_t used = join_slots((uint32_t)cs);
        r.ok = r.ok && used <= JOIN_SLOTS && used >= 2 * cs && (used & (used - 1)) == 0;
        std::fill(slots.begin(), slots.end(), 0);
        for (size_t i = 0; i < S.size(); ++i) {
            const uint64_t sig = join_sig(S[i], narrow);
            if (join_sub(sig, W, s) != t) continue;
            r.ok = r.ok && !staged[i];
            staged[i] = 1;
            uint32_t slot = join_slot(sig, used), tries = 0;
            for (; tries < used && slots[slot]; ++tries) slot = (slot + 1) & (used - 1);
            r.ok = r.ok && tries < used && slot < used;
            slots[slot] = (S[i] << 20) | (i + 1);                  // (an entry: remainder, a count field > 0)
        }
        for (size_t i = 0; i < P.size(); ++i) {
            const uint64_t sig = join_sig(P[i], narrow);
            if (join_sub(sig, W, s) != t) continue;
            r.ok = r.ok && !probed[i];
            probed[i] = 1;
            uint32_t slot = join_slot(sig, used), tries = 0;
            bool found = false;
            for (; tries < used && slots[slot]; ++tries) {
                if ((slots[slot] >> 20) == P[i]) {
                    found = true;
                    hit[(slots[slot] & 0xFFFFF) - 1] = 1;
                    break;
                }
                slot = (slot + 1) & (used - 1);
            }
            (found ? r.both : r.p_only).insert(P[i]);
        }
        if (!join_next(s0, &s, &t)) break;
    }
    for (size_t i = 0; i < S.size(); ++i) {
        r.ok = r.ok && staged[i];
        if (!hit[i]) r.s_only.insert(S[i]);
    }
    for (size_t i = 0; i < P.size(); ++i) r.ok = r.ok && probed[i];
    return r;
}

enum { UNIFORM = 0, TOP14 = 1, NARROW = 2, NVARIANTS = 3 };

static std::vector<uint64_t> draw(std::mt19937_64 &g, size_t n, int variant) {
    std::set<uint64_t> seen;
    std::vector<uint64_t> out;
    const uint64_t top = (g() & 0x3FFF) << 30;
    while (out.size() < n) {
        uint64_t x;
        if (variant == UNIFORM) x = g() & ((1ull << TAB_RBITS) - 1);
        else if (variant == TOP14) x = top | (g() & ((1ull << 30) - 1));
        else x = (g() & ((1ull << (TAB_RBITS - TAB_NSH)) - 1)) << TAB_NSH;
        if (seen.insert(x).second) out.push_back(x);
    }
    return out;
}

// The header's narrow-key inverse (k = 20: even, the key code is the smaller
// planar code), as tests/test_table_setops_gpu.py builds a long narrow bucket:
// f = q << 21 | r, z = f * MUL^-1 mod 2^41, c = z ^ (z >> 21); when c < 2^40 is
// the smaller code of its class, tab_key_h of its k-mer is (q << 21 | r) << 23.
static long narrow_inverse(long *n) {
    const uint32_t k = 20, q = 0x3C3C3;
    long bad = 0;
    for (uint64_t r = 0; r < (1u << 21); r += 5) {
        const uint64_t f = ((uint64_t)q << 21) | r;
        const uint64_t z = (f * TAB_INV) & ((1ull << 41) - 1), c = z ^ (z >> 21);
        if (c >= (1ull << (2 * k))) continue;
        const uint64_t rc = tab_rc_code(c, k);
        if (c > rc) continue;
        ++*n;
        const uint64_t h = tab_key_h(c, rc, k);
        if ((h >> TAB_RBITS) != q || join_sig(h & ((1ull << TAB_RBITS) - 1), true) != r || (h & ((1ull << TAB_NSH) - 1))) ++bad;
    }
    return bad;
}

int main() {
    std::mt19937_64 g(29);
    const size_t T = JOIN_TILE, sizes[6] = {0, 1, T - 1, T, T + 1, 5 * T};
    long bad = 0, n = 0, deep = 0, split = 0;
    auto check = [&](const std::vector<uint64_t> &A, const std::vector<uint64_t> &B, bool narrow, const char *what) {
        std::set<uint64_t> sa(A.begin(), A.end()), sb(B.begin(), B.end()), both, a_only, b_only;
        for (uint64_t x : sa) (sb.count(x) ? both : a_only).insert(x);
        for (uint64_t x : sb)
            if (!sa.count(x)) b_only.insert(x);
        for (int swap = 0; swap < 2; ++swap) {                      // A probes B, and B probes A
            ++n;
            const Joined r = swap ? model(A, B, narrow) : model(B, A, narrow);
            const bool same = r.ok && r.both == both && (swap ? r.s_only : r.p_only) == a_only &&
                              (swap ? r.p_only : r.s_only) == b_only;
            split += r.ranges > 1;
            deep += r.max_depth >= 14;
            if (!same && bad++ < 8) printf("%s: |A| %zu |B| %zu narrow %d swap %d\n", what, A.size(), B.size(), (int)narrow, swap);
        }
    };
    for (int variant = 0; variant < NVARIANTS; ++variant)
        for (size_t na : sizes)
            for (size_t nb : sizes) {
                // two draws with a shared part: the first third of B is taken from A
                std::vector<uint64_t> pool = draw(g, na + nb, variant);
                std::vector<uint64_t> A(pool.begin(), pool.begin() + na), B(pool.begin() + na, pool.end());
                for (size_t i = 0; i < std::min(na, nb) / 3; ++i) B[i] = A[2 * i];
                std::shuffle(B.begin(), B.end(), g);
                check(A, B, variant == NARROW, "shared third");
                if (na == nb) {
                    std::vector<uint64_t> C(A);
                    std::shuffle(C.begin(), C.end(), g);
                    check(A, C, variant == NARROW, "identical");
                    std::vector<uint64_t> D(pool.begin() + na, pool.end());
                    check(A, D, variant == NARROW, "disjoint");
                }
            }
    printf("cases: %ld with more than one range, %ld with a split of depth >= 14\n", split, deep);
    if (!split || !deep) bad += 1;                                  // (the deep and the split cases must be there)
    long nn = 0;
    const long nbad = narrow_inverse(&nn);
    printf("narrow inverse: %ld of %ld k-mers outside their bucket\n", nbad, nn);
    if (nbad || nn < 50000) bad += 1;
    printf("setops join: %ld of %ld mismatches\n", bad, n);
    return bad != 0;
}
