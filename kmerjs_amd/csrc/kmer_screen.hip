// kmer_screen.hip — reads screened against a finished table (gfx950):
// kmer_table_screen / kmer_table_screen_device.  Read-only on the table, like
// kmer_lookup.hip and kmer_probe.hip, whose view of it (TabView) this shares.
//
// The windows of all reads are numbered in input order (wbase: the exclusive
// scan of the reads' window counts) and worked in pieces of consecutive
// windows; a piece may end inside a read.
//
//   keys    a lane takes SC_NS consecutive windows: it finds their read (a
//           binary search in wbase), loads the bytes they span as aligned
//           dwords -- none before the buffer, none past its end: the edge
//           dwords are patched byte by byte --, turns them into bit planes as
//           pass 1 does (kmer_table.hip tab_round), and every window is a
//           shift of the planes: h[p] (tab_key_h) and the window's code
//           (screen_weight: 0, 1, 2, doubled, or skipped)
//   sort    (sorted route only) (bucket, window) pairs by bucket, one radix
//           sort over 21 bits; windows of weight 0 and skipped ones sort last
//   probe   the scheme of kmer_probe.hip's tab_probe_kernel with h given: a
//           wave takes 64 probes; a bucket of <= SC_LANE_MAX entries is scanned
//           by the probe's own lane; the longer ones: the wave walks the
//           DISTINCT buckets among its probes, streams each once and answers
//           every probe of the run.  In window order (direct route) runs have
//           length 1 and this is the lookup's scan; after the sort a long
//           bucket is read once per run.  Probes of weight 0 and skipped ones
//           touch no table memory.
//   reduce  per read, the sum over its windows in the piece, added to its row:
//           a read of more than SC_OWN_MAX windows by the whole wave, a shorter
//           one by its own lane.  Pieces follow each other in stream order, so
//           a read cut by a piece edge is accumulated over consecutive pieces.
// Every cross-lane read (readlane, ballot, shuffle) sits at the wave-uniform
// level of the loops, outside the per-lane branches; the loops over a bucket
// and over a run have wave-uniform trip counts.  One writer per output slot,
// no atomics (but the error word).
#include "kmer_device.hpp"

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>

namespace kmerhip {

constexpr uint32_t SC_LANE_MAX = 16;     // bucket entries up to which the probe's own lane scans
constexpr uint32_t SC_UNROLL = 8;        // wave loads (64 entries, 512 B each) in flight per round of a wave scan
constexpr uint32_t SC_WG_PER_CU = 7;     // workgroups of 4 waves per CU
constexpr uint32_t SC_OWN_MAX = 8;       // windows of a read (in the piece) up to which its own lane sums them

namespace {

// index of read r's first window (r == n_reads: the total)
__device__ __forceinline__ uint64_t sc_wb(const TabScreen &a, uint64_t r) {
    return r < a.n_reads ? a.wbase2[r] >> 1 : a.total;
}

__device__ __forceinline__ uint32_t wave_sum32(uint32_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += (uint32_t)__shfl_xor((int)x, o);
    return x;
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), o);
        x += ((uint64_t)hi << 32) | lo;
    }
    return x;
}

}  // namespace

__global__ __launch_bounds__(256) void screen_keys_kernel(const TabScreen a) {
    const uint32_t k = a.k;
    const uint32_t kmask = k >= 32 ? ~0u : ((1u << k) - 1u);
    const uint8_t *const end = a.data + a.len;
    const uint64_t ngroups = (a.m + SC_NS - 1) / SC_NS;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t i = g * SC_NS;                                  // window of the piece
        const uint64_t iend = i + SC_NS < a.m ? i + SC_NS : a.m;
        uint64_t p = a.p0 + i;                                   // ... of the call
        // the read of window p: the last r with wbase[r] <= p (reads without
        // windows share their successor's base and are passed over)
        uint64_t lo = 0, hi = a.n_reads;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (sc_wb(a, mid) <= p) lo = mid + 1;
            else hi = mid;
        }
        uint64_t r = lo ? lo - 1 : 0;
        while (i < iend && r < a.n_reads) {
            const uint64_t b = sc_wb(a, r), e = sc_wb(a, r + 1);
            if (e <= p) {                                        // (a read without windows)
                ++r;
                continue;
            }
            const uint64_t w0 = p - b;
            const uint32_t nv = (uint32_t)(e - p < iend - i ? e - p : iend - i);   // 1 .. SC_NS
            // planes of the bytes [st + w0, st + w0 + nv + k - 1), from aligned dwords
            const uint8_t *src = a.data + a.lines[r].start + w0;
            const uint32_t off = (uint32_t)((uintptr_t)src & 3u);
            const uint8_t *q0 = src - off;
            const uint32_t span = off + nv + k - 1;              // (<= 3 + 16 + 31)
            uint64_t LO = 0, HI = 0, EX = 0;
            constexpr int NDW = (SC_NS + 31 + 3 + 3) / 4;
#pragma unroll
            for (int d = 0; d < NDW; ++d) {
                uint32_t x = 0x41414141u;                        // ('A': outside the windows, never looked at)
                const uint8_t *q = q0 + 4 * d;
                if ((uint32_t)(4 * d) < span && q < end) {
                    if (q >= a.data && q + 4 <= end) {
                        x = *(const uint32_t *)q;
                    } else {                                     // the buffer's first / last dword: no read outside it
                        for (int j = 0; j < 4; ++j)
                            if (q + j >= a.data && q + j < end)
                                x = (x & ~(0xFFu << (8 * j))) | ((uint32_t)q[j] << (8 * j));
                    }
                }
                const uint32_t lo4 = __builtin_amdgcn_udot4((x ^ (x >> 1)) & 0x02020202u, 0x08040201u, 0u, false) >> 1;
                const uint32_t hi4 = __builtin_amdgcn_udot4(x & 0x04040404u, 0x08040201u, 0u, false) >> 2;
                const uint32_t cc = ((x >> 1) ^ (x >> 2)) & 0x03030303u;
                const uint32_t ne = __builtin_amdgcn_perm(0u, 0x54474341u, cc) ^ x;      // 0 where the byte is A/C/G/T
                const uint32_t nz = (((ne & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | ne) & 0x80808080u;
                const uint32_t ex4 = __builtin_amdgcn_udot4(nz >> 7, 0x08040201u, 0u, false);
                LO |= (uint64_t)lo4 << (4 * d);
                HI |= (uint64_t)hi4 << (4 * d);
                EX |= (uint64_t)ex4 << (4 * d);
            }
            LO >>= off;
            HI >>= off;
            EX >>= off;
#pragma unroll
            for (uint32_t m = 0; m < SC_NS; ++m) {
                if (m >= nv) continue;
                const uint32_t fx = (uint32_t)(EX >> m) & kmask;
                uint64_t h = 0;
                uint8_t cd = SC_SKIP;
                if (fx == 0) {
                    uint64_t cf, cr;
                    bool dbl;
                    screen_window_codes(LO, HI, m, k, &cf, &cr);
                    const uint32_t wt = screen_weight(cf, cr, k, a.plo, a.phi, a.pmask, a.canonical != 0, &dbl);
                    h = tab_key_h(cf, cr, k);
                    cd = (uint8_t)(wt | (dbl ? SC_DBL : 0u));
                }
                a.h[i + m] = h;
                a.code[i + m] = cd;
                if (a.bkt) {
                    a.bkt[i + m] = (cd & SC_WMASK) ? (uint32_t)(h >> TAB_RBITS) : TAB_NQ;
                    a.idx[i + m] = (uint32_t)(i + m);
                }
            }
            i += nv;
            p += nv;
            ++r;
        }
    }
}

// sb / si: the probes' buckets (ascending; TAB_NQ: no probe) and windows, or
// null: probe p is window p of the piece
__global__ __launch_bounds__(256) void screen_probe_kernel(const TabScreen a, const uint32_t *sb, const uint32_t *si) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t table_end = a.start[TAB_NQ] < a.cap ? a.start[TAB_NQ] : a.cap;
    const uint64_t ngroups = (a.m + 63) >> 6;
    for (uint64_t g = wave; g < ngroups; g += nwaves) {          // (wave-uniform)
        const uint64_t p = (g << 6) + lane;
        uint32_t q = TAB_NQ, i = 0;
        uint64_t h = 0;
        bool dbl = false;
        if (p < a.m) {
            if (sb) {
                q = sb[p];
                i = si[p];
                if (q < TAB_NQ) {
                    h = a.h[i];
                    dbl = (a.code[i] & SC_DBL) != 0;
                }
            } else {
                i = (uint32_t)p;
                const uint8_t cd = a.code[i];
                if (cd & SC_WMASK) {                             // (a skipped window's weight bits are 0)
                    h = a.h[i];
                    q = (uint32_t)(h >> TAB_RBITS);
                    dbl = (cd & SC_DBL) != 0;
                }
            }
        }
        uint64_t rem = 0, base = 0;
        uint32_t len = 0;                                        // entries to scan (0: the answer is 0)
        if (q < TAB_NQ) {
            rem = h & ((1ull << TAB_RBITS) - 1);
            const uint32_t L = a.nd[q];
            if (L) {
                base = a.start[q];
                if (base > table_end || L > table_end - base) {  // an extent past the table is not read
                    atomicOr(a.err, ERR_TAB_LOOKUP);
                    *a.badq = q;
                } else {
                    len = L;
                }
            }
        }
        bool found = false;
        uint64_t word = 0;
        if (len <= SC_LANE_MAX) {                                // lane-per-probe: no cross-lane reads inside
            for (uint32_t j = 0; j < len; ++j) {
                const uint64_t e = a.ent[base + j];
                if ((e >> 20) == rem) {
                    found = true;
                    word = e;
                }
            }
        }
        // the probes of one bucket that are neighbours share its extent: the
        // first lane of each run of a long bucket
        const bool wide = len > SC_LANE_MAX;
        const uint32_t qprev = (uint32_t)__shfl_up((int)q, 1);
        uint64_t heads = __ballot(wide && (lane == 0 || qprev != q));
        while (heads) {                                          // (wave-uniform)
            const uint32_t j = (uint32_t)__builtin_ctzll(heads);
            heads &= heads - 1;
            const uint32_t qj = readlane32(q, j), L = readlane32(len, j);
            const uint64_t b = readlane64(base, j);
            // the run's probes not answered yet (in window order a later run of
            // the same bucket is answered here too, and its own scan ends at once)
            uint64_t pend = __ballot(wide && q == qj && !found);
            for (uint32_t o = 0; o < L && pend; o += 64 * SC_UNROLL) {   // (wave-uniform trip count)
                uint64_t e[SC_UNROLL];
#pragma unroll
                for (uint32_t u = 0; u < SC_UNROLL; ++u) {
                    const uint32_t x = o + u * 64 + lane;
                    e[u] = x < L ? a.ent[b + x] : 0;
                }
                uint64_t todo = pend;
                while (todo) {                                   // (wave-uniform: every probe of the run in turn)
                    const uint32_t t = (uint32_t)__builtin_ctzll(todo);
                    todo &= todo - 1;
                    const uint64_t r = readlane64(rem, t);
                    bool f = false;
                    uint64_t mine = 0;
#pragma unroll
                    for (uint32_t u = 0; u < SC_UNROLL; ++u) {
                        const uint32_t x = o + u * 64 + lane;
                        if (x < L && (e[u] >> 20) == r) {
                            f = true;
                            mine = e[u];
                        }
                    }
                    const uint64_t mm = __ballot(f);             // (keys of a bucket are distinct: one match at most)
                    const uint64_t w = readlane64(mine, mm ? (uint32_t)__builtin_ctzll(mm) : 0u);
                    if (mm) pend &= ~(1ull << t);
                    if (mm && lane == t) {
                        found = true;
                        word = w;
                    }
                }
            }
        }
        uint64_t cnt = 0;
        if (found) {
            cnt = word & TAB_CMAX;
            if (cnt == TAB_CMAX) {                               // the count is in the big list (tiny: linear)
                cnt = 0;
                for (uint64_t t = 0; t < a.n_big; ++t)
                    if (a.big[t].h == h) cnt = a.big[t].count;
            }
            if (dbl) cnt *= 2;
        }
        if (p < a.m) a.val[i] = cnt;                             // the one writer of window i's value
    }
}

__global__ __launch_bounds__(256) void screen_reduce_kernel(const TabScreen a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t p1 = a.p0 + a.m;
    const uint64_t ngroups = (a.n_reads + 63) >> 6;
    for (uint64_t g = wave; g < ngroups; g += nwaves) {          // (wave-uniform)
        const uint64_t r = (g << 6) + lane;
        uint64_t b = 0, e = 0;                                   // the read's windows in the piece
        if (r < a.n_reads) {
            b = sc_wb(a, r);
            e = sc_wb(a, r + 1);
            b = b > a.p0 ? b : a.p0;
            e = e < p1 ? e : p1;
            if (e < b) e = b;
        }
        uint32_t w = 0, ht = 0, sk = 0;                          // (a piece holds <= 2^26 windows of weight <= 2)
        uint64_t sm = 0;
        auto take = [&](uint64_t x, uint32_t &w_, uint32_t &ht_, uint32_t &sk_, uint64_t &sm_) {
            const uint8_t cd = a.code[x - a.p0];
            const uint32_t m = cd & SC_WMASK;
            sk_ += (cd & SC_SKIP) ? 1u : 0u;
            w_ += m;
            if (m) {
                const uint64_t v = a.val[x - a.p0];
                if (v >= a.min_count) {
                    ht_ += m;
                    sm_ += (uint64_t)m * v;
                }
            }
        };
        const bool lng = e - b > SC_OWN_MAX;
        if (!lng)
            for (uint64_t x = b; x < e; ++x) take(x, w, ht, sk, sm);
        uint64_t todo = __ballot(lng);
        while (todo) {                                           // (wave-uniform: every long read in turn)
            const uint32_t j = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1;
            const uint64_t bj = readlane64(b, j), ej = readlane64(e, j);
            uint32_t w2 = 0, ht2 = 0, sk2 = 0;
            uint64_t sm2 = 0;
            for (uint64_t x = bj + lane; x < ej; x += 64) take(x, w2, ht2, sk2, sm2);
            w2 = wave_sum32(w2);
            ht2 = wave_sum32(ht2);
            sk2 = wave_sum32(sk2);
            sm2 = wave_sum64(sm2);
            if (lane == j) {
                w = w2;
                ht = ht2;
                sk = sk2;
                sm = sm2;
            }
        }
        if (e > b) {                                             // the one writer of row r in this piece
            ScreenRow row = a.rows[r];
            row.windows += w;
            row.hits += ht;
            row.skipped += sk;
            row.sum += sm;
            a.rows[r] = row;
        }
    }
}

hipError_t launch_screen_keys(const TabScreen &a, uint32_t n_cu, hipStream_t s) {
    if (a.m == 0) return hipSuccess;
    const uint64_t groups = (a.m + SC_NS - 1) / SC_NS;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((groups + 255) / 256, (uint64_t)std::max(n_cu, 1u) * 16);
    hipLaunchKernelGGL(screen_keys_kernel, dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_screen_probe(const TabScreen &a, const uint32_t *sb, const uint32_t *si, uint32_t n_cu,
                               hipStream_t s) {
    if (a.m == 0) return hipSuccess;
    const uint64_t wgs = (((a.m + 63) >> 6) + 3) >> 2;           // 4 waves of 64 probes per workgroup
    const uint32_t grid = (uint32_t)std::min<uint64_t>(wgs, (uint64_t)std::max(n_cu, 1u) * SC_WG_PER_CU);
    hipLaunchKernelGGL(screen_probe_kernel, dim3(grid), dim3(256), 0, s, a, sb, si);
    return hipGetLastError();
}

hipError_t launch_screen_reduce(const TabScreen &a, hipStream_t s) {
    if (a.m == 0 || a.n_reads == 0) return hipSuccess;
    const uint64_t wgs = (((a.n_reads + 63) >> 6) + 3) >> 2;     // 4 waves of 64 reads per workgroup
    const uint32_t grid = (uint32_t)std::min<uint64_t>(wgs, 1u << 16);
    hipLaunchKernelGGL(screen_reduce_kernel, dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t screen_sort_bytes(uint64_t m, size_t *bytes) {
    rocprim::double_buffer<uint32_t> kb(nullptr, nullptr), vb(nullptr, nullptr);
    *bytes = 0;
    return rocprim::radix_sort_pairs(nullptr, *bytes, kb, vb, (size_t)std::max<uint64_t>(m, 1), 0, SC_BITS, nullptr);
}

hipError_t launch_screen_sort(uint32_t *bkt, uint32_t *bkt2, uint32_t *idx, uint32_t *idx2, uint64_t m, void *tmp,
                              size_t tmp_bytes, const uint32_t **sb, const uint32_t **si, hipStream_t s) {
    rocprim::double_buffer<uint32_t> kb(bkt, bkt2), vb(idx, idx2);
    size_t bytes = tmp_bytes;
    const hipError_t e = rocprim::radix_sort_pairs(tmp, bytes, kb, vb, (size_t)m, 0, SC_BITS, s);
    *sb = kb.current();
    *si = vb.current();
    return e;
}

}  // namespace kmerhip
