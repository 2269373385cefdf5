// kmer_probe.hip — the matcher's probe of a finished table (gfx950):
// kmer_match_open_table.  The join is driven from the small side: each
// distinct k-mer of the template DB is looked up once in the table, where the
// table lies.  Read-only on the table, like kmer_lookup.hip, whose view of it
// (TabView) this shares.
//
//   keys    DB k-mer i -> its class's bucket (kmer_internal.hpp:
//           tab_code2_planar, tab_key_h) or TAB_NQ when it fails the prefix
//           or, in canonical mode, is not the smaller string of its class: such
//           a key touches no table memory
//   sort    (bucket, i) pairs by bucket, one radix sort over 21 bits
//   probe   a wave takes 64 consecutive sorted probes.  Buckets are unsorted,
//           so a scan is linear; a short bucket (<= PB_LANE_MAX entries) is
//           scanned by the probe's own lane.  The longer ones: the wave walks
//           the DISTINCT buckets among its probes (a ballot of run heads),
//           all 64 lanes stream the bucket strided, PB_UNROLL wave loads in
//           flight per round, and every loaded entry is compared against every
//           probe of the bucket's run that is still unanswered -- the bucket is
//           read once per wave, not once per probe, and the scan ends when the
//           run is answered.  Two probes of a run may carry the same remainder
//           (x and rc x of one class): each is answered on its own.  A run that
//           straddles two waves is scanned by both.
// Every cross-lane read (readlane, ballot, shuffle) sits at the wave-uniform
// level of the loops, outside the per-lane branches; the loops over a bucket
// and over a run have wave-uniform trip counts.  One writer per output slot,
// no atomics (but the error word).
#include "kmer_device.hpp"

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>

namespace kmerhip {

constexpr uint32_t PB_LANE_MAX = 16;     // bucket entries up to which the probe's own lane scans
constexpr uint32_t PB_UNROLL = 8;        // wave loads (64 entries, 512 B each) in flight per round of a wave scan
constexpr uint32_t PB_WG_PER_CU = 7;     // workgroups of 4 waves per CU
constexpr uint32_t PB_BITS = TAB_L1 + TAB_L2 + 1;   // sort key: the bucket, or TAB_NQ (no probe)
constexpr uint32_t PB_NONE = 0xFFFFFFFFu;

__global__ __launch_bounds__(256) void tab_probe_keys_kernel(const TabProbe a) {
    const uint32_t km = a.k >= 32 ? ~0u : ((1u << a.k) - 1u);
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < a.m; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t cf, cr;
        tab_code2_planar(a.U[i], a.k, &cf, &cr);
        const uint32_t lo = (uint32_t)cf & km, hi = (uint32_t)(cf >> a.k) & km;
        bool ok = (((lo ^ a.plo) | (hi ^ a.phi)) & a.pmask) == 0;
        if (a.canonical) ok = ok && tab_str_le(cf, cr, a.k);
        a.bkt[i] = ok ? (uint32_t)(tab_key_h(cf, cr, a.k) >> TAB_RBITS) : TAB_NQ;
        a.idx[i] = (uint32_t)i;
    }
}

// sb / si: the probes' buckets (ascending; TAB_NQ: no probe) and DB indices
__global__ __launch_bounds__(256) void tab_probe_kernel(const TabProbe a, const uint32_t *sb, const uint32_t *si) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t table_end = a.start[TAB_NQ] < a.cap ? a.start[TAB_NQ] : a.cap;
    const uint64_t ngroups = (a.m + 63) >> 6;
    for (uint64_t g = wave; g < ngroups; g += nwaves) {          // (wave-uniform)
        const uint64_t p = (g << 6) + lane;
        const uint32_t q = p < a.m ? sb[p] : TAB_NQ;
        const uint32_t i = p < a.m ? si[p] : 0u;
        uint64_t h = 0, rem = 0, base = 0;
        uint32_t len = 0;                                        // entries to scan (0: the answer is 0)
        bool dbl = false;
        if (q < TAB_NQ) {
            uint64_t cf, cr;
            tab_code2_planar(a.U[i], a.k, &cf, &cr);
            h = tab_key_h(cf, cr, a.k);
            rem = h & ((1ull << TAB_RBITS) - 1);
            dbl = !a.canonical && cf == cr;                      // a self-complementary key holds both strands' windows
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
        if (len <= PB_LANE_MAX) {                                // lane-per-probe: no cross-lane reads inside
            for (uint32_t j = 0; j < len; ++j) {
                const uint64_t e = a.ent[base + j];
                if ((e >> 20) == rem) {
                    found = true;
                    word = e;
                }
            }
        }
        // the probes of one bucket are neighbours and share its extent: the
        // first lane of each run of a long bucket
        const bool wide = len > PB_LANE_MAX;
        const uint32_t qprev = (uint32_t)__shfl_up((int)q, 1);
        uint64_t heads = __ballot(wide && (lane == 0 || qprev != q));
        while (heads) {                                          // (wave-uniform)
            const uint32_t j = (uint32_t)__builtin_ctzll(heads);
            heads &= heads - 1;
            const uint32_t qj = readlane32(q, j), L = readlane32(len, j);
            const uint64_t b = readlane64(base, j);
            uint64_t pend = __ballot(wide && q == qj);           // the run's probes not answered yet
            for (uint32_t o = 0; o < L && pend; o += 64 * PB_UNROLL) {   // (wave-uniform trip count)
                uint64_t e[PB_UNROLL];
#pragma unroll
                for (uint32_t u = 0; u < PB_UNROLL; ++u) {
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
                    for (uint32_t u = 0; u < PB_UNROLL; ++u) {
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
        if (p < a.m) {                                           // the one writer of DB k-mer i's slots
            const bool in = cnt != 0;
            a.qidx[i] = in ? i : PB_NONE;
            a.hc[i] = in ? a.O[i + 1] - a.O[i] : 0;
            a.present[i] = in ? 1u : 0u;
            a.cnt[i] = cnt;
        }
    }
}

hipError_t tab_probe_temp_bytes(uint64_t m, size_t *bytes) {
    rocprim::double_buffer<uint32_t> kb(nullptr, nullptr), vb(nullptr, nullptr);
    *bytes = 0;
    return rocprim::radix_sort_pairs(nullptr, *bytes, kb, vb, (size_t)std::max<uint64_t>(m, 1), 0, PB_BITS, nullptr);
}

hipError_t launch_tab_probe(const TabProbe &a, uint32_t n_cu, hipStream_t s) {
    if (a.m == 0) return hipSuccess;
    const uint32_t cus = std::max(n_cu, 1u);
    const uint32_t kgrid = (uint32_t)std::min<uint64_t>((a.m + 255) / 256, (uint64_t)cus * 8);
    hipLaunchKernelGGL(tab_probe_keys_kernel, dim3(kgrid), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    rocprim::double_buffer<uint32_t> kb(a.bkt, a.bkt2), vb(a.idx, a.idx2);
    size_t bytes = a.tmp_bytes;
    e = rocprim::radix_sort_pairs(a.tmp, bytes, kb, vb, (size_t)a.m, 0, PB_BITS, s);
    if (e != hipSuccess) return e;
    const uint64_t wgs = (((a.m + 63) >> 6) + 3) >> 2;           // 4 waves of 64 probes per workgroup
    const uint32_t grid = (uint32_t)std::min<uint64_t>(wgs, (uint64_t)cus * PB_WG_PER_CU);
    hipLaunchKernelGGL(tab_probe_kernel, dim3(grid), dim3(256), 0, s, a, (const uint32_t *)kb.current(),
                       (const uint32_t *)vb.current());
    return hipGetLastError();
}

}  // namespace kmerhip
