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
//   sort    (bucket, i) pairs by bucket, one radix sort over 21 bits (the
//           bucket-pair sort below, which the screen's sorted route shares)
//   probe   a wave takes 64 consecutive sorted probes and finds their entries
//           together (kmer_device.hpp: tab_wave_find): the probes of one bucket
//           are neighbours, so a long bucket is read once per wave
// One writer per output slot, no atomics (but the error word).
#include "kmer_device.hpp"

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>

namespace kmerhip {

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
    const uint64_t table_end = tab_end(a);
    const uint64_t ngroups = (a.m + 63) >> 6;
    for (uint64_t g = wave; g < ngroups; g += nwaves) {          // (wave-uniform)
        const uint64_t p = (g << 6) + lane;
        const uint32_t q = p < a.m ? sb[p] : TAB_NQ;
        const uint32_t i = p < a.m ? si[p] : 0u;
        uint64_t h = 0;
        bool dbl = false;
        if (q < TAB_NQ) {
            uint64_t cf, cr;
            tab_code2_planar(a.U[i], a.k, &cf, &cr);
            h = tab_key_h(cf, cr, a.k);
            dbl = !a.canonical && cf == cr;                      // a self-complementary key holds both strands' windows
        }
        uint64_t word;
        const bool found = tab_wave_find(a, table_end, lane, q, h, word);
        const uint64_t cnt = tab_value(a.big, a.n_big, found, word, h, dbl);
        if (p < a.m) {                                           // the one writer of DB k-mer i's slots
            const bool in = cnt != 0;
            a.qidx[i] = in ? i : PB_NONE;
            a.hc[i] = in ? a.O[i + 1] - a.O[i] : 0;
            a.present[i] = in ? 1u : 0u;
            a.cnt[i] = cnt;
        }
    }
}

hipError_t bucket_sort_bytes(uint64_t m, size_t *bytes) {
    rocprim::double_buffer<uint32_t> kb(nullptr, nullptr), vb(nullptr, nullptr);
    *bytes = 0;
    return rocprim::radix_sort_pairs(nullptr, *bytes, kb, vb, (size_t)std::max<uint64_t>(m, 1), 0, TAB_QBITS, nullptr);
}

hipError_t launch_bucket_sort(uint32_t *bkt, uint32_t *bkt2, uint32_t *idx, uint32_t *idx2, uint64_t m, void *tmp,
                              size_t tmp_bytes, const uint32_t **sb, const uint32_t **si, hipStream_t s) {
    rocprim::double_buffer<uint32_t> kb(bkt, bkt2), vb(idx, idx2);
    size_t bytes = tmp_bytes;
    const hipError_t e = rocprim::radix_sort_pairs(tmp, bytes, kb, vb, (size_t)m, 0, TAB_QBITS, s);
    *sb = kb.current();
    *si = vb.current();
    return e;
}

hipError_t launch_tab_probe(const TabProbe &a, uint32_t n_cu, hipStream_t s) {
    if (a.m == 0) return hipSuccess;
    const uint32_t cus = std::max(n_cu, 1u);
    const uint32_t kgrid = (uint32_t)std::min<uint64_t>((a.m + 255) / 256, (uint64_t)cus * 8);
    hipLaunchKernelGGL(tab_probe_keys_kernel, dim3(kgrid), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t *sb = nullptr, *si = nullptr;
    e = launch_bucket_sort(a.bkt, a.bkt2, a.idx, a.idx2, a.m, a.tmp, a.tmp_bytes, &sb, &si, s);
    if (e != hipSuccess) return e;
    const uint64_t wgs = (((a.m + 63) >> 6) + 3) >> 2;           // 4 waves of 64 probes per workgroup
    const uint32_t grid = (uint32_t)std::min<uint64_t>(wgs, (uint64_t)cus * TAB_WG_PER_CU);
    hipLaunchKernelGGL(tab_probe_kernel, dim3(grid), dim3(256), 0, s, a, sb, si);
    return hipGetLastError();
}

}  // namespace kmerhip
