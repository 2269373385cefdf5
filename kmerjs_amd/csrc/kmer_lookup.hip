// kmer_lookup.hip — batched lookup against a finished table (gfx950):
// kmer_table_lookup / kmer_table_lookup_device.  Read-only: the table, its
// bucket index and the big list are as the final kernels of kmer_table.hip
// left them.
//
// A wave takes 64 queries at a time.  Each lane turns its query's k bytes into
// the class's h (kmer_internal.hpp: tab_bytes_h), tests the prefix and, in
// canonical mode, that the key is the smaller string of its class, and reads
// its bucket's extent (kmer_device.hpp: tab_extent).  A short bucket is scanned
// by its own lane (tab_lane_find).  A longer one by the whole wave: the wave
// walks the lanes that hold one, reads that lane's extent and remainder with
// v_readlane, and all 64 lanes read the bucket strided, TAB_UNROLL 512-byte wave
// loads in flight per round, until a ballot finds the match.  Queries come in
// any order, so this walk has no runs to share a scan among, unlike the one of
// the sorted probers (tab_wave_find), which measured about 1 % slower here
// (profiles/table_readers_shared.md).  Every cross-lane read (readlane, ballot)
// sits at the wave-uniform level of the loops, outside the per-lane branches;
// the loop over a bucket has a wave-uniform trip count.
// One writer per output slot, no atomics (but the error word).
#include "kmer_device.hpp"

#include <algorithm>

namespace kmerhip {

__global__ __launch_bounds__(256) void tab_lookup_kernel(const TabLookup a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t table_end = tab_end(a);
    const uint64_t ngroups = (a.n + 63) >> 6;
    const uint32_t km = a.k >= 32 ? ~0u : ((1u << a.k) - 1u);
    for (uint64_t g = wave; g < ngroups; g += nwaves) {          // (wave-uniform)
        const uint64_t i = (g << 6) + lane;
        uint64_t h = 0;
        uint32_t q = TAB_NQ;                                     // (no probe: the answer is 0)
        bool dbl = false;
        if (i < a.n) {
            uint64_t cf, cr;
            bool ok = tab_bytes_h(a.keys + i * a.k, a.k, &cf, &cr, &h);
            const uint32_t lo = (uint32_t)cf & km, hi = (uint32_t)(cf >> a.k) & km;
            ok = ok && (((lo ^ a.plo) | (hi ^ a.phi)) & a.pmask) == 0;
            if (a.canonical) ok = ok && tab_str_le(cf, cr, a.k);
            else dbl = cf == cr;                                 // a self-complementary key holds both strands' windows
            if (ok) q = (uint32_t)(h >> TAB_RBITS);
        }
        const uint64_t rem = h & ((1ull << TAB_RBITS) - 1);
        uint64_t base = 0, word;
        const uint32_t len = q < TAB_NQ ? tab_extent(a, table_end, q, base) : 0u;   // entries to scan (0: the answer is 0)
        bool found = tab_lane_find(a, base, len, rem, word);
        uint64_t todo = __ballot(len > TAB_LANE_MAX);            // lanes whose bucket the wave scans together
        while (todo) {                                           // (wave-uniform)
            const uint32_t j = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1;
            const uint64_t b = readlane64(base, j), r = readlane64(rem, j);
            const uint32_t L = readlane32(len, j);
            bool f = false;
            uint64_t mine = 0;
            for (uint32_t o = 0; o < L; o += 64 * TAB_UNROLL) {  // (wave-uniform trip count)
                uint64_t e[TAB_UNROLL];
#pragma unroll
                for (uint32_t u = 0; u < TAB_UNROLL; ++u) {
                    const uint32_t p = o + u * 64 + lane;
                    e[u] = p < L ? a.ent[b + p] : 0;
                }
#pragma unroll
                for (uint32_t u = 0; u < TAB_UNROLL; ++u) {
                    const uint32_t p = o + u * 64 + lane;
                    if (p < L && (e[u] >> 20) == r) {
                        f = true;
                        mine = e[u];
                    }
                }
                if (__ballot(f)) break;                          // (keys of a bucket are distinct: one match at most)
            }
            const uint64_t m = __ballot(f);
            const uint64_t w = readlane64(mine, m ? (uint32_t)__builtin_ctzll(m) : 0u);
            if (lane == j) {
                found = m != 0;
                word = w;
            }
        }
        if (i < a.n) a.counts[i] = tab_value(a.big, a.n_big, found, word, h, dbl);
    }
}

hipError_t launch_tab_lookup(const TabLookup &a, uint32_t n_cu, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const uint64_t wgs = (((a.n + 63) >> 6) + 3) >> 2;           // 4 waves of 64 queries per workgroup
    const uint32_t grid = (uint32_t)std::min<uint64_t>(wgs, (uint64_t)std::max(n_cu, 1u) * TAB_WG_PER_CU);
    hipLaunchKernelGGL(tab_lookup_kernel, dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace kmerhip
