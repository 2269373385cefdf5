// kmer_setops.hip — two finished tables related to each other (gfx950):
// kmer_table_compare (the eight sums of kmer_table_overlap) and
// kmer_table_setop* (INTERSECT / SUBTRACT / UNION as (2-bit code, value) pairs
// for the extract's sort and decode).  Read-only on both tables (TabView).
//
// Two tables of one k share the hash and the 2^20 buckets, so bucket q of A
// meets bucket q of B only: one walk (tab_join_kernel<MODE>), that of
// tab_abund_kernel.  A wave takes 64 consecutive buckets, lane i the pair of
// bucket 64 g + i, and reads both extents (start[q], nd[q]).
//   short pair   both sides <= JOIN_LANE_MAX entries (every bucket of a small
//                table): the pair's own lane joins them with a nested loop,
//                no cross-lane reads inside
//   long pair    the whole wave, one pair after the other.  The staged side S
//                goes into the wave's own LDS slice, an open-addressing table
//                of at most JOIN_SLOTS 64-bit slots keyed by remainder (as
//                many as keep the load <= 1/2: join_slots; slot 0 = empty;
//                linear probing; LDS compare-and-swap; the slots used are
//                zeroed again after the probes), the probing side P is
//                streamed strided, JOIN_UNROLL 512-byte wave loads in flight
//                per round, each lane probing its own entries.  A
//                side S of more than JOIN_TILE entries is taken range by range
//                (kmer_internal.hpp: join_depth0 / join_sub / join_next): a
//                counting pass over S and P per range, the range halved while
//                it holds more than JOIN_TILE entries of S, both sides re-read
//                per range (L2 hits).  A P entry lies in exactly one range, so
//                hit or miss is decided in one place.
// Which side is staged: compare and INTERSECT the shorter one, SUBTRACT B,
// UNION B in the first walk (A's keys, vB added on a hit) and A in the second
// (B's keys that are not in A).
// Every ballot, readlane and DPP scan sits at the wave-uniform level of the
// loops; the loops over a bucket have wave-uniform trip counts.  No global
// atomic per entry: compare keeps its eight sums in registers (one wave
// reduction and one atomic per sum per wave at the end), count one sum, write
// one returning atomic per round of a wave.
//
// The result as a table (kmer_table_setop_into; JM_TCOUNT / JM_TWRITE).  Buckets
// are unsorted and remainders within one are distinct, so bucket q of the
// result is written straight from the join of bucket q of A and B: no sort, no
// decode to key bytes.  The count walk leaves nd_dst[q], a register of the
// pair's lane (short pair) or a wave sum (long pair) stored once, UNION's
// second walk adding to the first's; the host scans nd_dst into start_dst;
// the write walk puts bucket q's entries (rem << 20 | min(C, TAB_CMAX)) at
// start_dst[q] + a running offset: the lane's own (short pair), or the wave's
// plus a DPP scan over the lanes that hold a result in the round (long pair),
// carried across the ranges of a split bucket and, through cur_dst[q], across
// UNION's two walks.  A slot at or past nd_dst[q] is refused.  Counts >=
// TAB_CMAX go to the result's big list, one returning atomic per wave round
// that has any; the statistics are summed in registers.
#include "kmer_device.hpp"

namespace kmerhip {

constexpr uint32_t JOIN_UNROLL = 4;      // wave loads (64 entries, 512 B each) in flight per round
constexpr uint32_t JOIN_GROUPS = TAB_NQ / 64;
constexpr uint32_t JOIN_WAVES = 4;       // waves of a workgroup: 4 slices of 16 KiB, two workgroups per CU
// (JM_TCOUNT / JM_TWRITE: the result as a table -- entries per bucket, then the entries themselves)
enum { JM_COMPARE = 0, JM_COUNT = 1, JM_WRITE = 2, JM_TCOUNT = 3, JM_TWRITE = 4 };

// LDS traffic of one wave's lanes to each other's slots: ordered here
__device__ __forceinline__ void join_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t join_wave_sum(uint32_t x) { return readlane32(wave_incl_sum(x), 63); }

// the Map value of entry e (class h) on one side
__device__ __forceinline__ uint64_t join_value(const TabJoin &j, bool is_a, uint64_t e, uint64_t h, bool dbl) {
    return tab_value(is_a ? j.a.big : j.b.big, is_a ? j.a.n_big : j.b.n_big, true, e, h, dbl);
}

// One class seen from the probing side: ep its entry there, es its entry on the
// staged side (0: none).  compare: the probing side's own sums and the sums
// over the keys in both; setop: the keys to emit (the return value) and their
// value.  No prefix and (canonical mode or odd k): every class is w0 Map keys,
// never doubled, and nothing is decoded (DECODE false; not for the write pass,
// which needs the keys).
template <int MODE, bool DECODE>
__device__ __forceinline__ uint32_t join_visit(const TabJoin &j, bool p_is_a, uint32_t q, uint64_t ep, uint64_t es,
                                               uint64_t (&acc)[8], uint64_t keys[2], uint64_t *val) {
    *val = 0;
    if (!(ep & TAB_CMAX)) return 0;
    const uint64_t h = ((uint64_t)q << TAB_RBITS) | (ep >> 20);
    bool dbl = false;
    uint32_t n = j.a.canonical ? 1u : 2u;
    if (DECODE) n = tab_entry_keys(h, j.a.k, j.a.plo, j.a.phi, j.a.pmask, j.a.canonical != 0, keys, &dbl);
    if (!n) return 0;
    const uint64_t vp = join_value(j, p_is_a, ep, h, dbl);
    const uint64_t vs = es ? join_value(j, !p_is_a, es, h, dbl) : 0;
    const uint64_t va = p_is_a ? vp : vs, vb = p_is_a ? vs : vp;
    const bool in_a = va >= j.min_a, in_b = vb >= j.min_b;
    if (MODE == JM_COMPARE) {
        const uint64_t na = p_is_a && in_a ? n : 0u, nb = !p_is_a && in_b ? n : 0u, nab = in_a && in_b ? n : 0u;
        acc[0] += na;
        acc[1] += nb;
        acc[2] += nab;
        acc[3] += na * va;
        acc[4] += nb * vb;
        acc[5] += nab * va;
        acc[6] += nab * vb;
        acc[7] += nab * (va < vb ? va : vb);
        return 0;
    }
    uint64_t v;
    if (j.op == JOIN_INTERSECT) v = in_a && in_b ? (va < vb ? va : vb) : 0;
    else if (j.op == JOIN_SUBTRACT) v = in_a && !in_b ? va : 0;
    else if (!j.second) v = in_a ? va + (in_b ? vb : 0) : 0;
    else v = in_b && !in_a ? vb : 0;
    *val = v;
    return v ? n : 0u;
}

// The result as a table: one class seen from the probing side, ep its entry
// there, es its entry on the staged side (0: none).  Returns the class count C
// of the result's entry (0: no entry), *nk its Map keys and *v their value.
// Both sides double a self-complementary class alike (tab_entry_keys), so the
// operation on the Map values is the operation on the class counts, with the
// thresholds tested on the Map value.  A class without a Map key (canonical
// mode with a prefix that only the larger string starts with) has its class
// count for a value: a count holds it, and so does a UNION.
template <bool DECODE>
__device__ __forceinline__ uint64_t join_class(const TabJoin &j, bool p_is_a, uint32_t q, uint64_t ep, uint64_t es,
                                               uint32_t *nk, uint64_t *v) {
    *nk = 0;
    *v = 0;
    if (!(ep & TAB_CMAX)) return 0;
    const uint64_t h = ((uint64_t)q << TAB_RBITS) | (ep >> 20);
    uint64_t keys[2];
    bool dbl = false;
    uint32_t n = j.a.canonical ? 1u : 2u;
    if (DECODE) n = tab_entry_keys(h, j.a.k, j.a.plo, j.a.phi, j.a.pmask, j.a.canonical != 0, keys, &dbl);
    const uint64_t vp = join_value(j, p_is_a, ep, h, dbl);
    const uint64_t vs = es ? join_value(j, !p_is_a, es, h, dbl) : 0;
    const uint64_t r = join_result(j.op, j.second != 0, p_is_a ? vp : vs, p_is_a ? vs : vp, j.min_a, j.min_b);
    *nk = r ? n : 0u;
    *v = r;
    return join_class_count(r, dbl);
}

// the result as a table: one entry at slot `off` of its bucket (start sd, nd entries)
__device__ __forceinline__ void join_put_entry(const TabJoin &j, uint64_t sd, uint32_t off, uint32_t nd, uint64_t word) {
    if (join_slot_ok(sd, off, nd, j.cap_dst)) j.ent_dst[sd + off] = word;
    else atomicOr(j.err, ERR_TAB_EXTRACT);                       // count and write passes disagree: a defect
}

__device__ __forceinline__ void join_put_big(const TabJoin &j, uint64_t slot, uint64_t h, uint64_t C) {
    if (slot < j.big_cap) {
        j.big_dst[slot].h = h;
        j.big_dst[slot].count = C;
    } else {
        atomicOr(j.err, ERR_TAB_EXTRACT);
    }
}

// compare: the staged side's own sums (its keys and their values)
template <bool DECODE>
__device__ __forceinline__ void join_own(const TabJoin &j, bool is_a, uint32_t q, uint64_t e, uint64_t (&acc)[8]) {
    if (!(e & TAB_CMAX)) return;
    const uint64_t h = ((uint64_t)q << TAB_RBITS) | (e >> 20);
    uint64_t keys[2];
    bool dbl = false;
    uint32_t n = j.a.canonical ? 1u : 2u;
    if (DECODE) n = tab_entry_keys(h, j.a.k, j.a.plo, j.a.phi, j.a.pmask, j.a.canonical != 0, keys, &dbl);
    const uint64_t v = join_value(j, is_a, e, h, dbl);
    const uint64_t na = is_a && v >= j.min_a ? n : 0u, nb = !is_a && v >= j.min_b ? n : 0u;
    acc[0] += na;
    acc[1] += nb;
    acc[3] += na * v;
    acc[4] += nb * v;
}

// short pair: the entry of remainder rem among len entries (0: none)
__device__ __forceinline__ uint64_t join_find(const uint64_t *ent, uint64_t base, uint32_t len, uint64_t rem) {
    uint64_t es = 0;
    for (uint32_t i = 0; i < len; ++i) {
        const uint64_t x = ent[base + i];
        if ((x >> 20) == rem && (x & TAB_CMAX)) es = x;
    }
    return es;
}

__device__ __forceinline__ void join_put(const TabJoin &j, uint64_t slot, uint64_t key, uint64_t v) {
    if (slot < j.cap_out) {
        j.codes[slot] = tab_planar_code2(key, j.a.k);
        j.vals[slot] = v;
    } else {
        atomicOr(j.err, ERR_TAB_EXTRACT);                        // count and write passes disagree: a defect
    }
}

// a bucket's extent on one side (0 entries: an empty table, an empty bucket, or
// an extent past the table, which is not read)
__device__ __forceinline__ uint32_t join_extent(const TabJoin &j, const TabView &v, uint64_t end, uint32_t q,
                                                uint32_t side, uint64_t *base) {
    *base = 0;
    if (!v.nd) return 0;
    const uint32_t L = v.nd[q];
    if (!L) return 0;
    const uint64_t b = v.start[q];
    if (b > end || L > end - b) {
        atomicOr(j.err, ERR_TAB_LOOKUP);
        j.badq[0] = q;
        j.badq[1] = side;
        return 0;
    }
    *base = b;
    return L;
}

template <int MODE, bool DECODE>
__global__ __launch_bounds__(64 * JOIN_WAVES) void tab_join_kernel(const TabJoin j) {
    __shared__ unsigned long long slices[JOIN_WAVES * JOIN_SLOTS];
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long *tab = slices + (threadIdx.x >> 6) * JOIN_SLOTS;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    const uint64_t end_a = j.a.nd ? tab_end(j.a) : 0;
    const uint64_t end_b = j.b.nd ? tab_end(j.b) : 0;
    const bool narrow = j.a.k <= TAB_NARROW_K;
    const uint32_t W = join_width(narrow);
    const bool swap = MODE != JM_COMPARE && j.op == JOIN_UNION && j.second;   // the lane path probes with B
    uint64_t acc[8];
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) acc[i] = 0;
    uint64_t mine = 0;                                           // count: this lane's keys
    for (uint32_t i = lane; i < JOIN_SLOTS; i += 64) tab[i] = 0; // the slice is empty between two joins
    join_sync();
    for (uint32_t g = wave; g < JOIN_GROUPS; g += nwaves) {      // (wave-uniform)
        const uint32_t q = (g << 6) + lane;
        uint64_t base_a, base_b;
        const uint32_t len_a = join_extent(j, j.a, end_a, q, 0, &base_a);
        const uint32_t len_b = join_extent(j, j.b, end_b, q, 1, &base_b);
        const bool shortp = len_a <= JOIN_LANE_MAX && len_b <= JOIN_LANE_MAX;
        // the result as a table: bucket q's entries so far (count), its extent and the offset reached (write)
        uint32_t nd_q = 0, off_q = 0;
        uint64_t sd_q = 0;
        if (MODE == JM_TCOUNT) nd_q = j.second ? j.nd_dst[q] : 0u;
        if (MODE == JM_TWRITE) {
            nd_q = j.nd_dst[q];
            sd_q = j.start_dst[q];
            off_q = j.second ? j.cur_dst[q] : 0u;
        }
        const bool carry = MODE == JM_TWRITE && j.op == JOIN_UNION && !j.second;   // the second walk goes on from here
        {   // lane-per-pair: no cross-lane reads inside the loops
            const uint64_t *ent_p = swap ? j.b.ent : j.a.ent, *ent_s = swap ? j.a.ent : j.b.ent;
            const uint64_t bp = swap ? base_b : base_a, bs = swap ? base_a : base_b;
            const uint32_t lp = shortp ? (swap ? len_b : len_a) : 0u, ls = shortp ? (swap ? len_a : len_b) : 0u;
            uint64_t keys[2], v;
            if (MODE == JM_COMPARE) {
                for (uint32_t i = 0; i < lp; ++i) {
                    const uint64_t ep = ent_p[bp + i];
                    join_visit<MODE, DECODE>(j, true, q, ep, join_find(ent_s, bs, ls, ep >> 20), acc, keys, &v);
                }
                for (uint32_t i = 0; i < ls; ++i) join_own<DECODE>(j, false, q, ent_s[bs + i], acc);
            } else if (MODE == JM_COUNT) {
                for (uint32_t i = 0; i < lp; ++i) {
                    const uint64_t ep = ent_p[bp + i];
                    mine += join_visit<MODE, DECODE>(j, !swap, q, ep, join_find(ent_s, bs, ls, ep >> 20), acc, keys, &v);
                }
            } else if (MODE == JM_WRITE) {
                uint32_t t = 0;
                for (uint32_t i = 0; i < lp; ++i) {
                    const uint64_t ep = ent_p[bp + i];
                    t += join_visit<MODE, DECODE>(j, !swap, q, ep, join_find(ent_s, bs, ls, ep >> 20), acc, keys, &v);
                }
                uint64_t slot = wave_reserve(j.n_out, t, lane);
                for (uint32_t i = 0; i < lp; ++i) {
                    const uint64_t ep = ent_p[bp + i];
                    const uint32_t n = join_visit<MODE, DECODE>(j, !swap, q, ep, join_find(ent_s, bs, ls, ep >> 20), acc, keys, &v);
                    for (uint32_t x = 0; x < n; ++x) join_put(j, slot++, keys[x], v);
                }
            } else if (MODE == JM_TCOUNT) {                      // the bucket's count: a register, stored once
                uint32_t c = 0, nk;
                for (uint32_t i = 0; i < lp; ++i) {
                    const uint64_t ep = ent_p[bp + i];
                    const uint64_t C = join_class<DECODE>(j, !swap, q, ep, join_find(ent_s, bs, ls, ep >> 20), &nk, &v);
                    c += C != 0;
                    mine += C >= TAB_CMAX;
                }
                if (shortp) j.nd_dst[q] = nd_q + c;
            } else {                                             // JM_TWRITE: the entries in bucket order of P
                uint32_t off = off_q, nb = 0, nk;
                for (uint32_t i = 0; i < lp; ++i) {
                    const uint64_t ep = ent_p[bp + i];
                    const uint64_t C = join_class<DECODE>(j, !swap, q, ep, join_find(ent_s, bs, ls, ep >> 20), &nk, &v);
                    if (!C) continue;
                    bool big;
                    const uint64_t word = join_entry(ep >> 20, C, &big);
                    join_put_entry(j, sd_q, off++, nd_q, word);
                    nb += big;
                    acc[0] += 1;
                    acc[1] += nk;
                    acc[2] += nk * v;
                }
                if (shortp && carry) j.cur_dst[q] = off;
                uint64_t slot = wave_reserve(j.n_out, nb, lane);   // (big counts: one returning atomic if the wave has any)
                for (uint32_t i = 0; nb && i < lp; ++i) {
                    const uint64_t ep = ent_p[bp + i];
                    const uint64_t C = join_class<DECODE>(j, !swap, q, ep, join_find(ent_s, bs, ls, ep >> 20), &nk, &v);
                    if (C >= TAB_CMAX) join_put_big(j, slot++, ((uint64_t)q << TAB_RBITS) | (ep >> 20), C);
                }
            }
        }
        uint64_t todo = __ballot(!shortp);                       // pairs the wave joins together
        while (todo) {                                           // (wave-uniform)
            const uint32_t jx = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1;
            const uint32_t qj = (g << 6) + jx;
            const uint64_t ba = readlane64(base_a, jx), bb = readlane64(base_b, jx);
            const uint32_t la = readlane32(len_a, jx), lb = readlane32(len_b, jx);
            // the probing side: compare / INTERSECT the longer one, SUBTRACT A, UNION A then B
            const bool p_is_a = MODE == JM_COMPARE || j.op == JOIN_INTERSECT ? la >= lb : !swap;
            const uint64_t *ent_p = p_is_a ? j.a.ent : j.b.ent, *ent_s = p_is_a ? j.b.ent : j.a.ent;
            const uint64_t bp = p_is_a ? ba : bb, bs = p_is_a ? bb : ba;
            const uint32_t LP = p_is_a ? la : lb, LS = p_is_a ? lb : la;
            // the result as a table: the pair's count / running offset, wave-uniform; it carries
            // across the ranges of a split bucket
            const uint32_t nd_j = readlane32(nd_q, jx);
            const uint64_t sd_j = readlane64(sd_q, jx);
            uint32_t woff = readlane32(off_q, jx), pc = 0;
            if (MODE != JM_COMPARE && (LP == 0 || (j.op == JOIN_INTERSECT && LS == 0))) {
                if (MODE == JM_TCOUNT && lane == 0) j.nd_dst[qj] = nd_j;
                if (carry && lane == 0) j.cur_dst[qj] = woff;
                continue;
            }
            const uint32_t s0 = join_depth0(LS);
            uint32_t s = s0;
            uint64_t t = 0;
            for (;;) {                                           // the ranges of S, depth first (wave-uniform)
                uint32_t cs = LS, cp = LP;
                if (s) {                                         // counting pass: entries of range (s, t) on both sides
                    uint32_t ns = 0, np = 0;
                    for (uint32_t o = 0; o < LS; o += 64 * JOIN_UNROLL) {
                        uint64_t e[JOIN_UNROLL];
#pragma unroll
                        for (uint32_t u = 0; u < JOIN_UNROLL; ++u) {
                            const uint32_t p = o + u * 64 + lane;
                            e[u] = p < LS ? ent_s[bs + p] : 0;
                        }
#pragma unroll
                        for (uint32_t u = 0; u < JOIN_UNROLL; ++u)
                            ns += o + u * 64 + lane < LS && join_sub(join_sig(e[u] >> 20, narrow), W, s) == t;
                    }
                    for (uint32_t o = 0; o < LP; o += 64 * JOIN_UNROLL) {
                        uint64_t e[JOIN_UNROLL];
#pragma unroll
                        for (uint32_t u = 0; u < JOIN_UNROLL; ++u) {
                            const uint32_t p = o + u * 64 + lane;
                            e[u] = p < LP ? ent_p[bp + p] : 0;
                        }
#pragma unroll
                        for (uint32_t u = 0; u < JOIN_UNROLL; ++u)
                            np += o + u * 64 + lane < LP && join_sub(join_sig(e[u] >> 20, narrow), W, s) == t;
                    }
                    cs = join_wave_sum(ns);
                    cp = join_wave_sum(np);
                }
                if (cs > JOIN_TILE) {                            // halve the range; distinct remainders: s <= W
                    if (s >= W) {                                // (equal remainders in one bucket: not a table)
                        if (lane == 0) {
                            atomicOr(j.err, ERR_TAB_LOOKUP);
                            j.badq[0] = qj;
                            j.badq[1] = p_is_a ? 1u : 0u;
                        }
                        break;
                    }
                    ++s;
                    t <<= 1;
                    continue;
                }
                const bool stage = cs && cp;                     // (no probes: nothing to stage for)
                const uint32_t used = join_slots(cs);            // slots of this range's table: load <= 1/2
                if (stage || (MODE == JM_COMPARE && cs)) {
                    for (uint32_t o = 0; o < LS; o += 64 * JOIN_UNROLL) {   // (wave-uniform trip count)
                        uint64_t e[JOIN_UNROLL];
#pragma unroll
                        for (uint32_t u = 0; u < JOIN_UNROLL; ++u) {
                            const uint32_t p = o + u * 64 + lane;
                            e[u] = p < LS ? ent_s[bs + p] : 0;
                        }
#pragma unroll
                        for (uint32_t u = 0; u < JOIN_UNROLL; ++u) {
                            const uint64_t sig = join_sig(e[u] >> 20, narrow);
                            if (!(e[u] & TAB_CMAX) || join_sub(sig, W, s) != t) continue;   // (past the end: 0)
                            if (MODE == JM_COMPARE) join_own<DECODE>(j, !p_is_a, qj, e[u], acc);
                            if (!stage) continue;
                            uint32_t slot = join_slot(sig, used);
                            for (uint32_t tries = 0; tries < used; ++tries) {   // (<= used / 2 staged: a free slot)
                                if (atomicCAS(&tab[slot], 0ull, (unsigned long long)e[u]) == 0ull) break;
                                slot = (slot + 1) & (used - 1);
                            }
                        }
                    }
                    if (stage) join_sync();
                }
                for (uint32_t o = 0; cp && o < LP; o += 64 * JOIN_UNROLL) {   // (wave-uniform trip count)
                    uint64_t e[JOIN_UNROLL], ev[JOIN_UNROLL];
#pragma unroll
                    for (uint32_t u = 0; u < JOIN_UNROLL; ++u) {
                        const uint32_t p = o + u * 64 + lane;
                        e[u] = p < LP ? ent_p[bp + p] : 0;
                    }
                    uint32_t nt = 0, nb = 0;
#pragma unroll
                    for (uint32_t u = 0; u < JOIN_UNROLL; ++u) {
                        ev[u] = 0;
                        const uint64_t rem = e[u] >> 20, sig = join_sig(rem, narrow);
                        if (!(e[u] & TAB_CMAX) || join_sub(sig, W, s) != t) continue;
                        uint64_t es = 0;
                        uint32_t slot = join_slot(sig, used);
                        for (uint32_t tries = 0; stage && tries < used; ++tries) {   // (nothing staged: a miss)
                            const uint64_t x = __hip_atomic_load(&tab[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                            if (!x) break;
                            if ((x >> 20) == rem) {
                                es = x;
                                break;
                            }
                            slot = (slot + 1) & (used - 1);
                        }
                        uint64_t keys[2], v;
                        if (MODE == JM_TCOUNT || MODE == JM_TWRITE) {
                            uint32_t nk;
                            const uint64_t C = join_class<DECODE>(j, p_is_a, qj, e[u], es, &nk, &v);
                            if (MODE == JM_TCOUNT) {
                                pc += C != 0;
                                mine += C >= TAB_CMAX;
                            } else if (C) {
                                ev[u] = C;
                                nt += 1;
                                nb += C >= TAB_CMAX;
                                acc[0] += 1;
                                acc[1] += nk;
                                acc[2] += nk * v;
                            }
                            continue;
                        }
                        const uint32_t n = join_visit<MODE, DECODE>(j, p_is_a, qj, e[u], es, acc, keys, &v);
                        if (MODE == JM_COUNT) mine += n;
                        if (MODE == JM_WRITE) {
                            ev[u] = n ? v : 0;
                            nt += n;
                        }
                    }
                    if (MODE == JM_TWRITE) {                     // one scan over the lanes that hold a result
                        const uint32_t incl = wave_incl_sum(nt);
                        uint32_t off = woff + (incl - nt);
                        woff += readlane32(incl, 63);
                        uint64_t slot = wave_reserve(j.n_out, nb, lane);   // (one returning atomic if the round has big counts)
#pragma unroll
                        for (uint32_t u = 0; u < JOIN_UNROLL; ++u) {
                            if (!ev[u]) continue;
                            bool big;
                            const uint64_t word = join_entry(e[u] >> 20, ev[u], &big);
                            join_put_entry(j, sd_j, off++, nd_j, word);
                            if (big) join_put_big(j, slot++, ((uint64_t)qj << TAB_RBITS) | (e[u] >> 20), ev[u]);
                        }
                    }
                    if (MODE == JM_WRITE) {
                        uint64_t slot = wave_reserve(j.n_out, nt, lane);
#pragma unroll
                        for (uint32_t u = 0; u < JOIN_UNROLL; ++u) {
                            if (!ev[u]) continue;
                            uint64_t keys[2];
                            bool dbl;
                            const uint64_t h = ((uint64_t)qj << TAB_RBITS) | (e[u] >> 20);
                            const uint32_t n = tab_entry_keys(h, j.a.k, j.a.plo, j.a.phi, j.a.pmask, j.a.canonical != 0, keys, &dbl);
                            for (uint32_t x = 0; x < n; ++x) join_put(j, slot++, keys[x], ev[u]);
                        }
                    }
                }
                if (stage) {                                     // the slots used are empty again
                    join_sync();
                    for (uint32_t i = lane; i < used; i += 64) tab[i] = 0;
                    join_sync();
                }
                if (!join_next(s0, &s, &t)) break;
            }
            if (MODE == JM_TCOUNT) {                             // the wave's count of the pair, stored once
                const uint32_t tot = join_wave_sum(pc);
                if (lane == 0) j.nd_dst[qj] = nd_j + tot;
            }
            if (carry && lane == 0) j.cur_dst[qj] = woff;
        }
    }
    if (MODE == JM_COMPARE) {
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i) {
            const uint64_t x = wave_sum(acc[i]);
            if (lane == 0 && x) atomicAdd(&j.sums[i], (unsigned long long)x);
        }
    } else if (MODE == JM_COUNT || MODE == JM_TCOUNT) {          // (TCOUNT: the result's big counts)
        mine = wave_sum(mine);
        if (lane == 0 && mine) atomicAdd(j.n_out, (unsigned long long)mine);
    } else if (MODE == JM_TWRITE) {                              // the result's statistics: classes, Map keys, their sum
#pragma unroll
        for (uint32_t i = 0; i < 3; ++i) {
            const uint64_t x = wave_sum(acc[i]);
            if (lane == 0 && x) atomicAdd(&j.stats[i], (unsigned long long)x);
        }
    }
}

// one group of 64 bucket pairs per wave: workgroups beyond the resident ones
// start as others end, which evens out unequal groups
constexpr uint32_t JOIN_GRID = JOIN_GROUPS / JOIN_WAVES;

// no prefix, no palindromes: nothing to decode (as launch_tab_spectrum)
static bool join_plain(const TabJoin &j) { return j.a.pmask == 0 && (j.a.canonical || (j.a.k & 1)); }

hipError_t launch_tab_join_compare(const TabJoin &j, hipStream_t s) {
    if (join_plain(j))
        hipLaunchKernelGGL((tab_join_kernel<JM_COMPARE, false>), dim3(JOIN_GRID), dim3(64 * JOIN_WAVES), 0, s, j);
    else
        hipLaunchKernelGGL((tab_join_kernel<JM_COMPARE, true>), dim3(JOIN_GRID), dim3(64 * JOIN_WAVES), 0, s, j);
    return hipGetLastError();
}

hipError_t launch_tab_join_count(const TabJoin &j, hipStream_t s) {
    if (join_plain(j))
        hipLaunchKernelGGL((tab_join_kernel<JM_COUNT, false>), dim3(JOIN_GRID), dim3(64 * JOIN_WAVES), 0, s, j);
    else
        hipLaunchKernelGGL((tab_join_kernel<JM_COUNT, true>), dim3(JOIN_GRID), dim3(64 * JOIN_WAVES), 0, s, j);
    return hipGetLastError();
}

hipError_t launch_tab_join_write(const TabJoin &j, hipStream_t s) {
    hipLaunchKernelGGL((tab_join_kernel<JM_WRITE, true>), dim3(JOIN_GRID), dim3(64 * JOIN_WAVES), 0, s, j);
    return hipGetLastError();
}

// the result as a table: nd_dst[q], then (after the scan of nd_dst) the entries,
// the big list and the statistics.  Neither needs the keys, so a plain table
// decodes nothing in either.
hipError_t launch_tab_join_tcount(const TabJoin &j, hipStream_t s) {
    if (join_plain(j))
        hipLaunchKernelGGL((tab_join_kernel<JM_TCOUNT, false>), dim3(JOIN_GRID), dim3(64 * JOIN_WAVES), 0, s, j);
    else
        hipLaunchKernelGGL((tab_join_kernel<JM_TCOUNT, true>), dim3(JOIN_GRID), dim3(64 * JOIN_WAVES), 0, s, j);
    return hipGetLastError();
}

hipError_t launch_tab_join_twrite(const TabJoin &j, hipStream_t s) {
    if (join_plain(j))
        hipLaunchKernelGGL((tab_join_kernel<JM_TWRITE, false>), dim3(JOIN_GRID), dim3(64 * JOIN_WAVES), 0, s, j);
    else
        hipLaunchKernelGGL((tab_join_kernel<JM_TWRITE, true>), dim3(JOIN_GRID), dim3(64 * JOIN_WAVES), 0, s, j);
    return hipGetLastError();
}

}  // namespace kmerhip
