// kmer_device.hpp — device helpers shared by the kernel translation units
// (kmer_kernels.hip, kmer_table.hip, kmer_dense.hip, kmer_fasta.hip,
// kmer_lookup.hip, kmer_probe.hip, kmer_abundance.hip, kmer_setops.hip,
// kmer_screen.hip, kmer_filter.hip, kmer_dbfasta.hip): one definition of each
// primitive that more than one kernel uses: wave reductions and scans, record
// append, tile staging, and what the readers of a finished table share
// (bucket extent, lane scan, the wave's find, entry value, plane nibbles,
// window walk: the last section).  The host/device contract (structs,
// constants, launch_* declarations) is kmer_internal.hpp.
#pragma once
#include "kmer_internal.hpp"

namespace kmerhip {

// Inclusive wave64 prefix sum with DPP (row_shr 1/2/4/8 inside rows of 16,
// then row_bcast 15 / 31 across rows): no LDS round trips on the critical path.
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, true);   // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, true);   // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, true);   // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, true);   // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);  // row_bcast:15
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);  // row_bcast:31
    return x;
}

// Inclusive wave64 prefix maximum (unsigned; 0 is the identity), same steps.
__device__ __forceinline__ uint32_t wave_incl_max(uint32_t x) {
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, true));   // row_shr:1
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, true));   // row_shr:2
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, true));   // row_shr:4
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, true));   // row_shr:8
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false));  // row_bcast:15
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false));  // row_bcast:31
    return x;
}

// lane i's value of v (i wave-uniform)
__device__ __forceinline__ uint32_t readlane32(uint32_t v, uint32_t i) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)i);
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, uint32_t i) {
    return ((uint64_t)readlane32((uint32_t)(v >> 32), i) << 32) | readlane32((uint32_t)v, i);
}

// sum of x over the wave, in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += (uint32_t)__shfl_xor((int)x, o);
    return x;
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += (uint64_t)__shfl_xor((long long)x, o);
    return x;
}

// t slots for this lane at an append cursor, one returning atomic for the wave (wave-uniform call)
__device__ __forceinline__ uint64_t wave_reserve(unsigned long long *cursor, uint32_t t, uint32_t lane) {
    const uint32_t incl = wave_incl_sum(t);
    const uint32_t total = readlane32(incl, 63);
    uint64_t base = 0;
    if (total && lane == 0) base = atomicAdd(cursor, (unsigned long long)total);
    return readlane64(base, 0) + (incl - t);
}

// Append one record to the list (its key bytes are gathered later); a full
// list is reported with ERR_REC_OVERFLOW and the host redoes the chunk.
__device__ __forceinline__ void append_record(Record *recs, unsigned long long *rec_count, uint64_t rec_cap,
                                              unsigned int *err, uint64_t order, uint64_t pos, uint32_t len,
                                              uint32_t strand) {
    const unsigned long long n = atomicAdd(rec_count, 1ull);
    if (n < rec_cap) {
        Record rec;
        rec.order = order;
        rec.pos = pos;
        rec.len = len;
        rec.strand = strand;
        recs[n] = rec;
    } else {
        atomicOr(err, ERR_REC_OVERFLOW);
    }
}

// per-byte 0x80 flag for bytes equal to '\n'; exact for ASCII bytes (< 0x80)
__device__ __forceinline__ uint32_t nl_flags(uint32_t x) {
    uint32_t t = x ^ 0x0A0A0A0Au;
    return ~(t + 0x7F7F7F7Fu) & 0x80808080u;
}

// the same for the word's first n bytes only (n <= 0: none, n >= 4: all)
__device__ __forceinline__ uint32_t nl_flags_below(uint32_t x, int64_t n) {
    const uint32_t z = nl_flags(x);
    return n <= 0 ? 0u : n < 4 ? (z & ((1u << (8 * n)) - 1u)) : z;
}

// ---------------------------------------------------------------------------
// tile staging
// ---------------------------------------------------------------------------
constexpr int NCH_MAIN = TILE / 16;          // 1024 16-byte chunks
constexpr int NCH_FRONT = FH / 16;           // 4
constexpr int NCH_BACK = BH / 16;            // 5
constexpr int BUFSZ = FH + TILE + BH;

// bytes outside [0, len) read as '\n' (a line boundary that is never a window byte)
__device__ __noinline__ inline uint4 load_chunk_edge(const uint8_t *data, int64_t g, uint64_t len) {
    uint32_t w[4];
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
        uint32_t x = 0;
        for (int b = 0; b < 4; ++b) {
            const int64_t p = g + i * 4 + b;
            const uint32_t c = (p >= 0 && (uint64_t)p < len) ? data[p] : (uint32_t)'\n';
            x |= c << (8 * b);
        }
        w[i] = x;
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ uint4 load_chunk(const uint8_t *data, int64_t g, uint64_t len) {
    if (g >= 0 && (uint64_t)g + 16 <= len) return *(const uint4 *)(data + g);
    return load_chunk_edge(data, g, len);
}

// Staging of tile [g0, g0 + TILE) and its FH / BH halos in LDS, 16 B per lane,
// coalesced, in two halves so that a kernel can put work of its own (the reset
// of its shared state) behind the loads in flight: load_tile issues the
// global loads, store_tile writes them to buf (BUFSZ bytes; tile byte p at
// buf[FH + p]) and returns the OR of this thread's tile words (bit 7 of a byte
// set: non-ASCII input).  The caller's barrier makes buf visible.
struct TileRegs {
    uint4 v[4];                  // chunks tid + TPB * i of the tile
    uint4 vh;                    // threads < NCH_FRONT + NCH_BACK: halo chunk hc (chunk 0 = byte g0 - FH)
    int hc;
};

// NT: the tile's own chunks with non-temporal loads -- for a kernel whose
// input is read once per launch and is far larger than the caches (the halo
// chunks, which the neighbouring tiles read as well, stay plain loads).
template <bool NT = false>
__device__ __forceinline__ void load_tile(const uint8_t *data, uint64_t len, int64_t g0, TileRegs &r) {
    const int tid = threadIdx.x;
    const bool halo = tid < NCH_FRONT + NCH_BACK;
    const int hc = tid < NCH_FRONT ? tid : NCH_FRONT + NCH_MAIN + (tid - NCH_FRONT);
    r.hc = hc;
    r.vh = make_uint4(0, 0, 0, 0);
    // every tile but the first / last has its halos inside [0, len): plain
    // 16-B loads with no per-chunk bounds logic, all issued back to back
    if (g0 - FH >= 0 && (uint64_t)(g0 + TILE + BH) <= len) {
        const uint8_t *src = data + g0 + 16 * tid;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (NT) {
                typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                const u32x4 t = __builtin_nontemporal_load((const u32x4 *)(src + 16 * TPB * i));
                r.v[i] = make_uint4(t.x, t.y, t.z, t.w);
            } else {
                r.v[i] = *(const uint4 *)(src + 16 * TPB * i);
            }
        }
        // every lane loads (lanes >= 9 repeat chunk 0): no divergent load, so no early wait
        r.vh = *(const uint4 *)(data + g0 - FH + 16 * (halo ? hc : 0));
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) r.v[i] = load_chunk(data, g0 + (int64_t)(tid + TPB * i) * 16, len);
        if (halo) r.vh = load_chunk(data, g0 - FH + (int64_t)hc * 16, len);
    }
}

__device__ __forceinline__ uint32_t store_tile(const TileRegs &r, uint8_t *buf) {
    const int tid = threadIdx.x;
    uint32_t orall = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        orall |= r.v[i].x | r.v[i].y | r.v[i].z | r.v[i].w;
        *(uint4 *)(buf + FH + (tid + TPB * i) * 16) = r.v[i];
    }
    if (tid < NCH_FRONT + NCH_BACK) *(uint4 *)(buf + r.hc * 16) = r.vh;
    return orall;
}

// A thread's 64 bytes at p (LDS, 16-byte aligned) and the 4 bytes after them.
__device__ __forceinline__ void load_thread_words(const uint8_t *p, uint32_t (&w)[17]) {
    const uint4 *src = (const uint4 *)p;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint4 x = src[j];
        w[4 * j] = x.x;
        w[4 * j + 1] = x.y;
        w[4 * j + 2] = x.z;
        w[4 * j + 3] = x.w;
    }
    w[16] = *(const uint32_t *)(p + 64);
}

// ---------------------------------------------------------------------------
// readers of a finished table (TabView) and of an input's windows (WinWalk)
// ---------------------------------------------------------------------------
constexpr uint32_t TAB_LANE_MAX = 16;    // bucket entries up to which one lane scans the bucket on its own
constexpr uint32_t TAB_UNROLL = 8;       // wave loads (64 entries, 512 B each) in flight per round of a wave scan
constexpr uint32_t TAB_WG_PER_CU = 7;    // workgroups of 4 waves per CU (7 waves per SIMD: the probing kernels' occupancy)

// where the table's entries end
__device__ __forceinline__ uint64_t tab_end(const TabView &v) { return v.start[TAB_NQ] < v.cap ? v.start[TAB_NQ] : v.cap; }

// Bucket q's entries: their number, the first at ent[base].  An extent past the
// table is not read: it is reported (ERR_TAB_LOOKUP, *badq) and counts as empty.
__device__ __forceinline__ uint32_t tab_extent(const TabView &v, uint64_t table_end, uint32_t q, uint64_t &base) {
    base = 0;
    const uint32_t L = v.nd[q];
    if (!L) return 0;
    base = v.start[q];
    if (base > table_end || L > table_end - base) {
        atomicOr(v.err, ERR_TAB_LOOKUP);
        *v.badq = q;
        return 0;
    }
    return L;
}

// A bucket of <= TAB_LANE_MAX entries scanned by the probe's own lane (a longer
// one is not touched): the entry of remainder rem.  No cross-lane reads inside.
__device__ __forceinline__ bool tab_lane_find(const TabView &v, uint64_t base, uint32_t len, uint64_t rem,
                                              uint64_t &word) {
    bool found = false;
    word = 0;
    if (len <= TAB_LANE_MAX) {
        for (uint32_t j = 0; j < len; ++j) {
            const uint64_t e = v.ent[base + j];
            if ((e >> 20) == rem) {
                found = true;
                word = e;
            }
        }
    }
    return found;
}

// The entry of class h in bucket q, for the 64 probes of a wave at once: called
// by all 64 lanes at the wave-uniform level of the caller's loop, a lane
// without a probe with q = TAB_NQ (it touches no table memory).  Buckets are
// unsorted, so a scan is linear.  A bucket of <= TAB_LANE_MAX entries (every
// bucket of a small table) is scanned by the probe's own lane.  The longer
// ones: the wave walks the runs of neighbouring probes of one bucket (a ballot
// of run heads), all 64 lanes stream the bucket strided, TAB_UNROLL wave loads
// in flight per round, and every loaded entry is compared against every probe
// of the bucket that is still unanswered -- sorted probes read a bucket once
// per wave, not once per probe, and the scan ends when they are answered.  In
// any other order a later run of the same bucket is answered by the first
// one's scan, and its own ends at once.  Two probes may carry the same
// remainder (x and rc x of one class): each is answered on its own.  A run
// that straddles two waves is scanned by both.
// Every cross-lane read (readlane, ballot, shuffle) sits at the wave-uniform
// level of the loops, outside the per-lane branches; the loops over a bucket
// and over a run have wave-uniform trip counts.
__device__ __forceinline__ bool tab_wave_find(const TabView &v, uint64_t table_end, uint32_t lane, uint32_t q,
                                              uint64_t h, uint64_t &word) {
    const uint64_t rem = h & ((1ull << TAB_RBITS) - 1);
    uint64_t base = 0;
    const uint32_t len = q < TAB_NQ ? tab_extent(v, table_end, q, base) : 0u;   // entries to scan (0: not found)
    bool found = tab_lane_find(v, base, len, rem, word);
    const bool wide = len > TAB_LANE_MAX;
    const uint32_t qprev = (uint32_t)__shfl_up((int)q, 1);
    uint64_t heads = __ballot(wide && (lane == 0 || qprev != q));
    while (heads) {                                              // (wave-uniform)
        const uint32_t j = (uint32_t)__builtin_ctzll(heads);
        heads &= heads - 1;
        const uint32_t qj = readlane32(q, j), L = readlane32(len, j);
        const uint64_t b = readlane64(base, j);
        uint64_t pend = __ballot(wide && q == qj && !found);     // the bucket's probes not answered yet
        for (uint32_t o = 0; o < L && pend; o += 64 * TAB_UNROLL) {   // (wave-uniform trip count)
            uint64_t e[TAB_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < TAB_UNROLL; ++u) {
                const uint32_t x = o + u * 64 + lane;
                e[u] = x < L ? v.ent[b + x] : 0;
            }
            uint64_t todo = pend;
            while (todo) {                                       // (wave-uniform: every pending probe in turn)
                const uint32_t t = (uint32_t)__builtin_ctzll(todo);
                todo &= todo - 1;
                const uint64_t r = readlane64(rem, t);
                bool f = false;
                uint64_t mine = 0;
#pragma unroll
                for (uint32_t u = 0; u < TAB_UNROLL; ++u) {
                    const uint32_t x = o + u * 64 + lane;
                    if (x < L && (e[u] >> 20) == r) {
                        f = true;
                        mine = e[u];
                    }
                }
                const uint64_t mm = __ballot(f);                 // (keys of a bucket are distinct: one match at most)
                const uint64_t w = readlane64(mine, mm ? (uint32_t)__builtin_ctzll(mm) : 0u);
                if (mm) pend &= ~(1ull << t);
                if (mm && lane == t) {
                    found = true;
                    word = w;
                }
            }
        }
    }
    return found;
}

// The Map value of class h from its entry word: the 20-bit count field, or the
// big list (tiny: linear) when the field is full; doubled for a
// self-complementary key that holds both strands' windows.  Not found: 0.
__device__ __forceinline__ uint64_t tab_value(const TabBig *big, uint64_t n_big, bool found, uint64_t word, uint64_t h,
                                              bool dbl) {
    if (!found) return 0;
    uint64_t cnt = word & TAB_CMAX;
    if (cnt == TAB_CMAX) {
        cnt = 0;
        for (uint64_t t = 0; t < n_big; ++t)
            if (big[t].h == h) cnt = big[t].count;
    }
    return dbl ? 2 * cnt : cnt;
}

// The plane nibbles of a dword's four bytes (bit j: byte j): the low and high
// code bit, and ex4 = the byte is outside A/C/G/T
__device__ __forceinline__ void dword_planes(uint32_t x, uint32_t &lo4, uint32_t &hi4, uint32_t &ex4) {
    lo4 = __builtin_amdgcn_udot4((x ^ (x >> 1)) & 0x02020202u, 0x08040201u, 0u, false) >> 1;
    hi4 = __builtin_amdgcn_udot4(x & 0x04040404u, 0x08040201u, 0u, false) >> 2;
    const uint32_t cc = ((x >> 1) ^ (x >> 2)) & 0x03030303u;
    const uint32_t ne = __builtin_amdgcn_perm(0u, 0x54474341u, cc) ^ x;      // 0 where the byte is A/C/G/T
    const uint32_t nz = (((ne & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | ne) & 0x80808080u;
    ex4 = __builtin_amdgcn_udot4(nz >> 7, 0x08040201u, 0u, false);
}

// index of line r's first window (r == n: the total)
__device__ __forceinline__ uint64_t walk_base(const WinWalk &a, uint64_t r) {
    return r < a.n ? a.wbase2[r] >> 1 : a.total;
}

// A lane's WALK_NS consecutive windows [g WALK_NS, ...) of the piece: it finds
// their line (a binary search in the window bases), loads the bytes they span
// as aligned dwords -- none before the buffer, none past its end: the edge
// dwords are patched byte by byte --, turns them into bit planes as pass 1
// does (kmer_table.hip tab_round), and every window is a shift of the planes:
// body(w, r, LO, HI, m, acgt) for window w of the piece, window m of planes LO /
// HI (screen_window_codes) in line r; acgt false: a byte outside A/C/G/T.
template <class Body>
__device__ __forceinline__ void walk_windows(const WinWalk &a, uint32_t k, uint64_t g, Body &&body) {
    const uint32_t kmask = k >= 32 ? ~0u : ((1u << k) - 1u);
    const uint8_t *const end = a.data + a.len;
    uint64_t i = g * WALK_NS;                                    // window of the piece
    const uint64_t iend = i + WALK_NS < a.m ? i + WALK_NS : a.m;
    uint64_t p = a.p0 + i;                                       // ... of the input
    // the line of window p: the last r with its base <= p (lines without
    // windows share their successor's base and are passed over)
    uint64_t lo = 0, hi = a.n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (walk_base(a, mid) <= p) lo = mid + 1;
        else hi = mid;
    }
    uint64_t r = lo ? lo - 1 : 0;
    while (i < iend && r < a.n) {
        const uint64_t b = walk_base(a, r), e = walk_base(a, r + 1);
        if (e <= p) {                                            // (a line without windows)
            ++r;
            continue;
        }
        const uint64_t w0 = p - b;
        const uint32_t nv = (uint32_t)(e - p < iend - i ? e - p : iend - i);   // 1 .. WALK_NS
        // planes of the bytes [st + w0, st + w0 + nv + k - 1), from aligned dwords
        const uint8_t *src = a.data + a.lines[r].start + w0;
        const uint32_t off = (uint32_t)((uintptr_t)src & 3u);
        const uint8_t *q0 = src - off;
        const uint32_t span = off + nv + k - 1;                  // (<= 3 + 16 + 31)
        uint64_t LO = 0, HI = 0, EX = 0;
        constexpr int NDW = (WALK_NS + 31 + 3 + 3) / 4;
#pragma unroll
        for (int d = 0; d < NDW; ++d) {
            uint32_t x = 0x41414141u;                            // ('A': outside the windows, never looked at)
            const uint8_t *q = q0 + 4 * d;
            if ((uint32_t)(4 * d) < span && q < end) {
                if (q >= a.data && q + 4 <= end) {
                    x = *(const uint32_t *)q;
                } else {                                         // the buffer's first / last dword: no read outside it
                    for (int j = 0; j < 4; ++j)
                        if (q + j >= a.data && q + j < end)
                            x = (x & ~(0xFFu << (8 * j))) | ((uint32_t)q[j] << (8 * j));
                }
            }
            uint32_t lo4, hi4, ex4;
            dword_planes(x, lo4, hi4, ex4);
            LO |= (uint64_t)lo4 << (4 * d);
            HI |= (uint64_t)hi4 << (4 * d);
            EX |= (uint64_t)ex4 << (4 * d);
        }
        LO >>= off;
        HI >>= off;
        EX >>= off;
#pragma unroll
        for (uint32_t m = 0; m < WALK_NS; ++m)
            if (m < nv) body(i + m, r, LO, HI, m, ((uint32_t)(EX >> m) & kmask) == 0);
        i += nv;
        p += nv;
        ++r;
    }
}

}  // namespace kmerhip
