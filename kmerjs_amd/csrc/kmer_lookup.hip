// kmer_lookup.hip — batched lookup against a finished table (gfx950):
// kmer_table_lookup / kmer_table_lookup_device.  Read-only: the table, its
// bucket index and the big list are as the final kernels of kmer_table.hip
// left them.
//
// A wave takes 64 queries at a time.  Each lane turns its query's k bytes into
// the class's h (kmer_internal.hpp: tab_bytes_h), tests the prefix and, in
// canonical mode, that the key is the smaller string of its class, and reads
// its bucket's extent (start[q], nd[q]).  Buckets are unsorted, so the scan
// is linear: a short bucket (<= LK_LANE_MAX entries, every bucket of a small
// table) is scanned by its own lane; a longer one by the whole wave -- the
// wave walks the lanes that hold one, reads that lane's extent and remainder
// with v_readlane, and all 64 lanes read the bucket strided, LK_UNROLL
// 512-byte wave loads in flight per round, until a ballot finds the match.
// Every cross-lane read (readlane, ballot) sits at the wave-uniform level of
// the loops, outside the per-lane branches; the loops over a bucket have
// wave-uniform trip counts.  One writer per output slot, no atomics (but the
// error word).
#include "kmer_device.hpp"

#include <algorithm>

namespace kmerhip {

constexpr uint32_t LK_LANE_MAX = 16;     // bucket entries up to which the query's own lane scans
constexpr uint32_t LK_UNROLL = 8;        // wave loads (64 entries, 512 B each) in flight per round of a wave scan
constexpr uint32_t LK_WG_PER_CU = 7;     // workgroups of 4 waves per CU (7 waves per SIMD: the kernel's occupancy)

__global__ __launch_bounds__(256) void tab_lookup_kernel(const TabLookup a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t table_end = a.start[TAB_NQ] < a.cap ? a.start[TAB_NQ] : a.cap;
    const uint64_t ngroups = (a.n + 63) >> 6;
    const uint32_t km = a.k >= 32 ? ~0u : ((1u << a.k) - 1u);
    for (uint64_t g = wave; g < ngroups; g += nwaves) {          // (wave-uniform)
        const uint64_t i = (g << 6) + lane;
        uint64_t h = 0, rem = 0, base = 0;
        uint32_t len = 0;                                        // entries to scan (0: the answer is 0)
        bool dbl = false;
        if (i < a.n) {
            uint64_t cf, cr;
            bool ok = tab_bytes_h(a.keys + i * a.k, a.k, &cf, &cr, &h);
            const uint32_t lo = (uint32_t)cf & km, hi = (uint32_t)(cf >> a.k) & km;
            ok = ok && (((lo ^ a.plo) | (hi ^ a.phi)) & a.pmask) == 0;
            if (a.canonical) ok = ok && tab_str_le(cf, cr, a.k);
            else dbl = cf == cr;                                 // a self-complementary key holds both strands' windows
            if (ok) {
                const uint32_t q = (uint32_t)(h >> TAB_RBITS);
                rem = h & ((1ull << TAB_RBITS) - 1);
                const uint32_t L = a.nd[q];
                if (L) {
                    base = a.start[q];
                    if (base > table_end || L > table_end - base) {   // an extent past the table is not read
                        atomicOr(a.err, ERR_TAB_LOOKUP);
                        *a.badq = q;
                    } else {
                        len = L;
                    }
                }
            }
        }
        bool found = false;
        uint64_t word = 0;
        if (len <= LK_LANE_MAX) {                                // lane-per-query: no cross-lane reads inside
            for (uint32_t j = 0; j < len; ++j) {
                const uint64_t e = a.ent[base + j];
                if ((e >> 20) == rem) {
                    found = true;
                    word = e;
                }
            }
        }
        uint64_t todo = __ballot(len > LK_LANE_MAX);             // lanes whose bucket the wave scans together
        while (todo) {                                           // (wave-uniform)
            const uint32_t j = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1;
            const uint64_t b = readlane64(base, j), r = readlane64(rem, j);
            const uint32_t L = readlane32(len, j);
            bool f = false;
            uint64_t mine = 0;
            for (uint32_t o = 0; o < L; o += 64 * LK_UNROLL) {   // (wave-uniform trip count)
                uint64_t e[LK_UNROLL];
#pragma unroll
                for (uint32_t u = 0; u < LK_UNROLL; ++u) {
                    const uint32_t p = o + u * 64 + lane;
                    e[u] = p < L ? a.ent[b + p] : 0;
                }
#pragma unroll
                for (uint32_t u = 0; u < LK_UNROLL; ++u) {
                    const uint32_t p = o + u * 64 + lane;
                    if (p < L && (e[u] >> 20) == r) {
                        f = true;
                        mine = e[u];
                    }
                }
                if (__ballot(f)) break;                          // (keys of a bucket are distinct: one match at most)
            }
            const uint64_t m = __ballot(f);
            const uint32_t src = m ? (uint32_t)__builtin_ctzll(m) : 0u;
            const uint64_t w = readlane64(mine, src);
            if (lane == j) {
                found = m != 0;
                word = w;
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
        if (i < a.n) a.counts[i] = cnt;
    }
}

hipError_t launch_tab_lookup(const TabLookup &a, uint32_t n_cu, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const uint64_t wgs = (((a.n + 63) >> 6) + 3) >> 2;           // 4 waves of 64 queries per workgroup
    const uint32_t grid = (uint32_t)std::min<uint64_t>(wgs, (uint64_t)std::max(n_cu, 1u) * LK_WG_PER_CU);
    hipLaunchKernelGGL(tab_lookup_kernel, dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace kmerhip
