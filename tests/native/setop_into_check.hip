// Host model of the set operation whose result stays a table
// (kmer_table_setop_into; kmer_setops.hip, JM_TCOUNT / JM_TWRITE), built only
// from the __host__ __device__ helpers of kmer_internal.hpp: the value a walk
// gives a class (join_result), the class count behind it (join_class_count),
// the result's entry and its big-list test (join_entry), the slot check of the
// write pass (join_slot_ok), and the ranges of a long bucket (join_depth0 /
// join_sig / join_sub / join_next).
// Two tables of a few buckets each -- empty, short (the lane path), long (2.5
// tiles: the wave path, range by range, rounds of JOIN_UNROLL x 64 entries
// with an exclusive scan over the lanes), against empty, short and long ones,
// counts around TAB_CMAX, doubled (self-complementary) classes -- go through
// the model's count pass, scan and write pass, UNION as two walks with the
// offset carried in a per-bucket cursor.  Checked: the count pass and the
// write pass agree (every slot below nd[q] written exactly once, none
// refused), the entries and the big list equal a std::map join of the two
// Maps on the Map values with the thresholds tested there, for the three
// operations and several threshold pairs.
// Built and run by tests/test_setop_into_keys.py; it has its own main and may
// be built with host sanitizers.
#include "kmer_internal.hpp"
#include <algorithm>
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <vector>
using namespace kmerhip;

constexpr uint32_t UNROLL = 4;                                    // (JOIN_UNROLL of kmer_setops.hip)

struct Ent {
    uint64_t rem, count;                                           // the class count (big-list counts resolved)
    bool dbl;                                                      // a self-complementary class: Map value 2 x count
};
typedef std::vector<std::vector<Ent>> Table;                       // by bucket, in no order

struct Out {
    std::vector<uint32_t> nd, cur;
    std::vector<uint64_t> start, ent;
    std::vector<uint8_t> written;
    std::map<uint64_t, uint64_t> big;                              // h -> count
    uint64_t nbig_counted = 0, refused = 0, twice = 0;
};

static uint64_t value(const Ent &e) { return e.dbl ? 2 * e.count : e.count; }

static const Ent *find(const std::vector<Ent> &b, uint64_t rem) {
    for (const Ent &e : b)
        if (e.rem == rem) return &e;
    return nullptr;
}

// the class count of the result for P's entry ep (es: the staged side's, or null)
static uint64_t klass(uint32_t op, bool second, bool p_is_a, const Ent &ep, const Ent *es, uint64_t min_a, uint64_t min_b) {
    const uint64_t vp = value(ep), vs = es ? value(*es) : 0;
    const uint64_t r = join_result(op, second, p_is_a ? vp : vs, p_is_a ? vs : vp, min_a, min_b);
    return join_class_count(r, ep.dbl);
}

// one walk over bucket q: the probing side's entries in the order the kernel
// meets them (short pair: bucket order; long pair: range by range, rounds of
// UNROLL x 64 entries, lane by lane).  visit(e, ~0u): does e give a result?
// (every entry, once per walk); visit(e, off): its offset within the walk
template <typename F>
static void walk(const std::vector<Ent> &P, const std::vector<Ent> &S, bool narrow, F &&visit) {
    if (P.size() <= JOIN_LANE_MAX && S.size() <= JOIN_LANE_MAX) {
        uint32_t off = 0;
        for (const Ent &e : P)
            if (visit(e, ~0u)) visit(e, off++);
        return;
    }
    const uint32_t W = join_width(narrow), s0 = join_depth0(S.size());
    uint32_t s = s0, woff = 0;
    uint64_t t = 0;
    for (;;) {
        uint64_t cs = 0;
        for (const Ent &e : S) cs += join_sub(join_sig(e.rem, narrow), W, s) == t;
        if (cs > JOIN_TILE) {
            ++s;
            t <<= 1;
            continue;
        }
        for (size_t o = 0; o < P.size(); o += 64 * UNROLL) {       // a round: lane l holds entries o + u 64 + l
            uint32_t nt[64] = {0};
            std::vector<std::pair<uint32_t, const Ent *>> held;    // (lane, entry) with a result, lane-major below
            for (uint32_t lane = 0; lane < 64; ++lane)
                for (uint32_t u = 0; u < UNROLL; ++u) {
                    const size_t p = o + u * 64 + lane;
                    if (p >= P.size() || join_sub(join_sig(P[p].rem, narrow), W, s) != t) continue;
                    held.emplace_back(lane, &P[p]);
                }
            // first the lanes learn whether they hold a result (offset unknown), then the scan, then the writes
            std::vector<uint32_t> has(held.size());
            for (size_t i = 0; i < held.size(); ++i) nt[held[i].first] += has[i] = visit(*held[i].second, ~0u);
            uint32_t incl = 0, base[64];
            for (uint32_t lane = 0; lane < 64; ++lane) {
                incl += nt[lane];
                base[lane] = woff + (incl - nt[lane]);
            }
            woff += incl;
            for (size_t i = 0; i < held.size(); ++i)
                if (has[i]) visit(*held[i].second, base[held[i].first]++);
        }
        if (!join_next(s0, &s, &t)) break;
    }
}

static Out run(const Table &A, const Table &B, uint32_t op, uint64_t min_a, uint64_t min_b, bool narrow) {
    const uint32_t nq = (uint32_t)A.size(), walks = op == JOIN_UNION ? 2 : 1;
    Out o;
    o.nd.assign(nq, 0);
    o.cur.assign(nq, 0);
    auto sides = [&](uint32_t q, bool second, const std::vector<Ent> **P, const std::vector<Ent> **S, bool *p_is_a) {
        const bool swap = op == JOIN_UNION && second;
        const bool longp = A[q].size() > JOIN_LANE_MAX || B[q].size() > JOIN_LANE_MAX;
        *p_is_a = op == JOIN_INTERSECT && longp ? A[q].size() >= B[q].size() : !swap;
        *P = *p_is_a ? &A[q] : &B[q];
        *S = *p_is_a ? &B[q] : &A[q];
    };
    for (uint32_t second = 0; second < walks; ++second)          // the count pass
        for (uint32_t q = 0; q < nq; ++q) {
            const std::vector<Ent> *P, *S;
            bool p_is_a;
            sides(q, second != 0, &P, &S, &p_is_a);
            uint32_t c = 0;
            walk(*P, *S, narrow, [&](const Ent &e, uint32_t off) -> uint32_t {
                const uint64_t C = klass(op, second != 0, p_is_a, e, find(*S, e.rem), min_a, min_b);
                if (off == ~0u) {
                    c += C != 0;
                    o.nbig_counted += C >= TAB_CMAX;
                }
                return C != 0;
            });
            o.nd[q] = (second ? o.nd[q] : 0) + c;
        }
    o.start.assign(nq + 1, 0);                                     // the scan
    for (uint32_t q = 0; q < nq; ++q) o.start[q + 1] = o.start[q] + o.nd[q];
    const uint64_t cap = o.start[nq];
    o.ent.assign(cap, 0);
    o.written.assign(cap, 0);
    for (uint32_t second = 0; second < walks; ++second)          // the write pass
        for (uint32_t q = 0; q < nq; ++q) {
            const std::vector<Ent> *P, *S;
            bool p_is_a;
            sides(q, second != 0, &P, &S, &p_is_a);
            const uint32_t off0 = second ? o.cur[q] : 0;
            uint32_t end = off0;
            walk(*P, *S, narrow, [&](const Ent &e, uint32_t off) -> uint32_t {
                const uint64_t C = klass(op, second != 0, p_is_a, e, find(*S, e.rem), min_a, min_b);
                if (!C || off == ~0u) return C != 0;
                bool big;
                const uint64_t word = join_entry(e.rem, C, &big);
                const uint32_t at = off0 + off;
                if (join_slot_ok(o.start[q], at, o.nd[q], cap)) {
                    o.twice += o.written[o.start[q] + at];
                    o.written[o.start[q] + at] = 1;
                    o.ent[o.start[q] + at] = word;
                } else {
                    ++o.refused;
                }
                if (big) o.big[((uint64_t)q << TAB_RBITS) | e.rem] = C;
                end = std::max(end, at + 1);
                return 1;
            });
            o.cur[q] = end;
        }
    return o;
}

// the Maps' join, class by class: h -> class count of the result
static std::map<uint64_t, uint64_t> want(const Table &A, const Table &B, uint32_t op, uint64_t min_a, uint64_t min_b) {
    std::map<uint64_t, uint64_t> out;
    for (uint32_t q = 0; q < A.size(); ++q) {
        std::map<uint64_t, std::pair<const Ent *, const Ent *>> cls;
        for (const Ent &e : A[q]) cls[e.rem].first = &e;
        for (const Ent &e : B[q]) cls[e.rem].second = &e;
        for (auto &kv : cls) {
            const Ent *a = kv.second.first, *b = kv.second.second;
            const bool dbl = a ? a->dbl : b->dbl;
            const uint64_t va = a ? value(*a) : 0, vb = b ? value(*b) : 0;
            const bool in_a = va >= min_a, in_b = vb >= min_b;
            uint64_t v = 0;
            if (op == JOIN_INTERSECT) v = in_a && in_b ? std::min(va, vb) : 0;
            else if (op == JOIN_SUBTRACT) v = in_a && !in_b ? va : 0;
            else v = (in_a ? va : 0) + (in_b ? vb : 0);
            if (v) out[((uint64_t)q << TAB_RBITS) | kv.first] = dbl ? v / 2 : v;
        }
    }
    return out;
}

static std::vector<Ent> bucket(std::mt19937_64 &g, size_t n, bool narrow, const std::vector<Ent> *share, size_t shared) {
    std::set<uint64_t> seen;
    std::vector<Ent> out;
    for (size_t i = 0; share && i < shared && i < share->size(); ++i) {   // the same classes, other counts
        Ent e = (*share)[(i * 7) % share->size()];
        if (!seen.insert(e.rem).second) continue;
        e.count = 1 + g() % 5;
        if (i % 11 == 0) e.count = TAB_CMAX - 2 + g() % 5;                // around the 20-bit field
        out.push_back(e);
    }
    while (out.size() < n) {
        uint64_t rem = g() & ((1ull << TAB_RBITS) - 1);
        if (narrow) rem &= ~((1ull << TAB_NSH) - 1);
        if (!seen.insert(rem).second) continue;
        Ent e{rem, 1 + g() % 4, g() % 13 == 0};
        if (g() % 17 == 0) e.count = TAB_CMAX - 3 + g() % 6;
        if (g() % 97 == 0) e.count = (1ull << 33) + g() % 1000;
        out.push_back(e);
    }
    std::shuffle(out.begin(), out.end(), g);
    return out;
}

int main() {
    std::mt19937_64 g(31);
    const size_t T = JOIN_TILE, sizes[5] = {0, 3, JOIN_LANE_MAX, JOIN_LANE_MAX + 1, T * 5 / 2};
    long bad = 0, n = 0, bigs = 0, made_big = 0, carried = 0;
    for (int narrow = 0; narrow < 2; ++narrow) {
        Table A, B;
        for (size_t na : sizes)
            for (size_t nb : sizes) {                              // every pair of sizes is one bucket
                A.push_back(bucket(g, na, narrow != 0, nullptr, 0));
                B.push_back(bucket(g, nb, narrow != 0, &A.back(), std::min(na, nb) / 2));
            }
        const uint64_t mins[4][2] = {{1, 1}, {2, 1}, {1, 3}, {TAB_CMAX, 2}};
        for (uint32_t op = 0; op <= JOIN_UNION; ++op)
            for (auto &m : mins)
                for (int self = 0; self < 2; ++self) {
                    const Table &Bx = self ? A : B;
                    ++n;
                    const Out o = run(A, Bx, op, m[0], m[1], narrow != 0);
                    const auto w = want(A, Bx, op, m[0], m[1]);
                    std::map<uint64_t, uint64_t> got, wbig;
                    bool ok = o.refused == 0 && o.twice == 0 && o.start.back() == w.size();
                    for (uint64_t x : o.written) ok = ok && x;
                    for (uint32_t q = 0; q < A.size(); ++q)
                        for (uint32_t i = 0; i < o.nd[q]; ++i) {
                            const uint64_t e = o.ent[o.start[q] + i], h = ((uint64_t)q << TAB_RBITS) | (e >> 20);
                            ok = ok && (e & TAB_CMAX) && !got.count(h);
                            got[h] = (e & TAB_CMAX) == TAB_CMAX ? (o.big.count(h) ? o.big.at(h) : 0) : (e & TAB_CMAX);
                        }
                    for (auto &kv : w)
                        if (kv.second >= TAB_CMAX) wbig[kv.first] = kv.second;
                    ok = ok && got == w && o.big == wbig && o.nbig_counted == wbig.size();
                    bigs += (long)wbig.size();
                    if (op == JOIN_UNION) {
                        for (uint32_t q = 0; q < A.size(); ++q) carried += o.cur[q] == o.nd[q] && A[q].size() > T && Bx[q].size() > T;
                        for (auto &kv : wbig) {                  // a big count from two small ones
                            const uint32_t q = (uint32_t)(kv.first >> TAB_RBITS);
                            const Ent *a = find(A[q], kv.first & ((1ull << TAB_RBITS) - 1));
                            const Ent *b = find(Bx[q], kv.first & ((1ull << TAB_RBITS) - 1));
                            made_big += a && b && a->count < TAB_CMAX && b->count < TAB_CMAX;
                        }
                    }
                    if (!ok && bad++ < 8)
                        printf("op %u min (%llu, %llu) narrow %d self %d: refused %llu twice %llu entries %llu of %zu\n", op,
                               (unsigned long long)m[0], (unsigned long long)m[1], narrow, self,
                               (unsigned long long)o.refused, (unsigned long long)o.twice,
                               (unsigned long long)o.start.back(), w.size());
                }
    }
    // the slot check itself: the last slot, the first one past the bucket, a bucket past the table
    if (!join_slot_ok(10, 4, 5, 15) || join_slot_ok(10, 5, 5, 15) || join_slot_ok(10, 4, 5, 14) || join_slot_ok(16, 0, 1, 15) ||
        join_slot_ok(0, 0, 0, 0))
        bad += 1;
    bool big = false;
    if (join_entry(5, TAB_CMAX - 1, &big) != ((5ull << 20) | (TAB_CMAX - 1)) || big) bad += 1;
    if (join_entry(5, TAB_CMAX, &big) != ((5ull << 20) | TAB_CMAX) || !big) bad += 1;
    if (join_entry(5, 1ull << 40, &big) != ((5ull << 20) | TAB_CMAX) || !big) bad += 1;
    printf("cases: %ld big counts, %ld made by a UNION of two small ones, %ld long pairs carried across two walks\n", bigs,
           made_big, carried);
    if (!bigs || !made_big || !carried) bad += 1;                  // (the cases the model is there for)
    printf("setop into: %ld of %ld mismatches\n", bad, n);
    return bad != 0;
}
