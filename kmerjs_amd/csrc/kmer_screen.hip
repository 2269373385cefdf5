// kmer_screen.hip — reads screened against a finished table (gfx950):
// kmer_table_screen / kmer_table_screen_device.  Read-only on the table, like
// kmer_lookup.hip and kmer_probe.hip, whose view of it (TabView) this shares.
//
// The windows of all reads are numbered in input order (wbase: the exclusive
// scan of the reads' window counts) and worked in pieces of consecutive
// windows; a piece may end inside a read.
//
//   keys    a lane takes WALK_NS consecutive windows (kmer_device.hpp:
//           walk_windows): per window h[p] (tab_key_h) and the window's code
//           (screen_weight: 0, 1, 2, doubled, or skipped)
//   sort    (sorted route only) (bucket, window) pairs by bucket, the
//           bucket-pair sort of kmer_probe.hip; windows of weight 0 and
//           skipped ones sort last
//   probe   a wave takes 64 probes and finds their entries together
//           (kmer_device.hpp: tab_wave_find).  In window order (direct route)
//           its runs have length 1; after the sort a long bucket is read once
//           per run.  Probes of weight 0 and skipped ones touch no table
//           memory.
//   reduce  per read, the sum over its windows in the piece, added to its row:
//           a read of more than SC_OWN_MAX windows by the whole wave, a shorter
//           one by its own lane.  Pieces follow each other in stream order, so
//           a read cut by a piece edge is accumulated over consecutive pieces.
// Every cross-lane read of the reduce (readlane, ballot, shuffle) sits at the
// wave-uniform level of its loops, outside the per-lane branches.  One writer
// per output slot, no atomics (but the error word).
#include "kmer_device.hpp"

#include <algorithm>

namespace kmerhip {

constexpr uint32_t SC_OWN_MAX = 8;       // windows of a read (in the piece) up to which its own lane sums them

__global__ __launch_bounds__(256) void screen_keys_kernel(const TabScreen a) {
    const uint32_t k = a.k;
    const uint64_t ngroups = (a.m + WALK_NS - 1) / WALK_NS;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (uint64_t)gridDim.x * blockDim.x) {
        walk_windows(a, k, g, [&](uint64_t w, uint64_t, uint64_t LO, uint64_t HI, uint32_t m, bool acgt) {
            uint64_t h = 0;
            uint8_t cd = SC_SKIP;
            if (acgt) {
                uint64_t cf, cr;
                bool dbl;
                screen_window_codes(LO, HI, m, k, &cf, &cr);
                const uint32_t wt = screen_weight(cf, cr, k, a.plo, a.phi, a.pmask, a.canonical != 0, &dbl);
                h = tab_key_h(cf, cr, k);
                cd = (uint8_t)(wt | (dbl ? SC_DBL : 0u));
            }
            a.h[w] = h;
            a.code[w] = cd;
            if (a.bkt) {
                a.bkt[w] = (cd & SC_WMASK) ? (uint32_t)(h >> TAB_RBITS) : TAB_NQ;
                a.idx[w] = (uint32_t)w;
            }
        });
    }
}

// sb / si: the probes' buckets (ascending; TAB_NQ: no probe) and windows, or
// null: probe p is window p of the piece
__global__ __launch_bounds__(256) void screen_probe_kernel(const TabScreen a, const uint32_t *sb, const uint32_t *si) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t table_end = tab_end(a);
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
        uint64_t word;
        const bool found = tab_wave_find(a, table_end, lane, q, h, word);
        const uint64_t cnt = tab_value(a.big, a.n_big, found, word, h, dbl);
        if (p < a.m) a.val[i] = cnt;                             // the one writer of window i's value
    }
}

__global__ __launch_bounds__(256) void screen_reduce_kernel(const TabScreen a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t p1 = a.p0 + a.m;
    const uint64_t ngroups = (a.n + 63) >> 6;
    for (uint64_t g = wave; g < ngroups; g += nwaves) {          // (wave-uniform)
        const uint64_t r = (g << 6) + lane;
        uint64_t b = 0, e = 0;                                   // the read's windows in the piece
        if (r < a.n) {
            b = walk_base(a, r);
            e = walk_base(a, r + 1);
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
            w2 = wave_sum(w2);
            ht2 = wave_sum(ht2);
            sk2 = wave_sum(sk2);
            sm2 = wave_sum(sm2);
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
    const uint64_t groups = (a.m + WALK_NS - 1) / WALK_NS;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((groups + 255) / 256, (uint64_t)std::max(n_cu, 1u) * 16);
    hipLaunchKernelGGL(screen_keys_kernel, dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_screen_probe(const TabScreen &a, const uint32_t *sb, const uint32_t *si, uint32_t n_cu,
                               hipStream_t s) {
    if (a.m == 0) return hipSuccess;
    const uint64_t wgs = (((a.m + 63) >> 6) + 3) >> 2;           // 4 waves of 64 probes per workgroup
    const uint32_t grid = (uint32_t)std::min<uint64_t>(wgs, (uint64_t)std::max(n_cu, 1u) * TAB_WG_PER_CU);
    hipLaunchKernelGGL(screen_probe_kernel, dim3(grid), dim3(256), 0, s, a, sb, si);
    return hipGetLastError();
}

hipError_t launch_screen_reduce(const TabScreen &a, hipStream_t s) {
    if (a.m == 0 || a.n == 0) return hipSuccess;
    const uint64_t wgs = (((a.n + 63) >> 6) + 3) >> 2;     // 4 waves of 64 reads per workgroup
    const uint32_t grid = (uint32_t)std::min<uint64_t>(wgs, 1u << 16);
    hipLaunchKernelGGL(screen_reduce_kernel, dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace kmerhip
