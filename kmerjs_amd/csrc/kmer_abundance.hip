// kmer_abundance.hip — the by-value readers of a finished table (gfx950):
// kmer_table_spectrum (distinct Map keys per value) and kmer_table_extract*
// (the Map keys whose value lies in a range, sorted by key bytes).  Read-only
// on the table, whose view (TabView) they share with kmer_lookup.hip and
// kmer_probe.hip.
//
// One walk serves all three kernels (tab_abund_kernel<MODE>).  A wave takes 64
// consecutive buckets, lane i bucket 64 g + i, and reads its extent
// (kmer_device.hpp: tab_extent).  A short bucket (<= TAB_LANE_MAX entries, every
// bucket of a small table) is walked by its own lane; the longer ones by the
// whole wave, one after the other: all 64 lanes stream the bucket strided,
// TAB_UNROLL 512-byte wave loads in flight per round.  Every cross-lane read
// (ballot, readlane, shuffle, DPP scan) sits at the wave-uniform level of the
// loops, outside the per-lane branches; the loops over a bucket have
// wave-uniform trip counts.
//
//   spectrum  value v of an entry, weight w = its Map keys (0, 1 or 2):
//             v <= AB_REGS          per-lane registers, wave-reduced at the end
//             v <  AB_LDS_BINS      the workgroup's LDS histogram (32-bit bins,
//                                   non-returning adds)
//             otherwise             the device histogram, a global atomic
//             A wave that has walked AB_FLUSH entries' worth of weight moves
//             the LDS bins to the device histogram (atomic exchange: no
//             barrier, the other waves keep adding), so a bin holds less than
//             4 (AB_FLUSH + a round) < 2^32.  No prefix and (canonical mode or
//             odd k): w is a constant and no key is decoded.  Entries whose
//             count is in the big list are left to the host.
//   count     the keys in range, one atomic per wave
//   write     (2-bit code, value) pairs appended in no order: per round one
//             wave scan and one returning atomic; a slot past the counted total
//             is refused (ERR_TAB_EXTRACT), never written
// then one radix sort of the pairs over 2 k bits and a decode to key bytes.
#include "kmer_device.hpp"

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>

namespace kmerhip {

constexpr uint32_t AB_FLUSH = 1u << 29;  // weight a wave adds before it moves the LDS bins out
constexpr uint32_t AB_GROUPS = TAB_NQ / 64;
enum { AB_SPECTRUM = 0, AB_COUNT = 1, AB_WRITE = 2 };

// spectrum: one entry's weight at its value
template <bool DECODE>
__device__ __forceinline__ void ab_spec_entry(const TabAbund &a, uint64_t e, uint32_t q, uint32_t w0,
                                              uint64_t (&r)[AB_REGS], uint32_t *bins) {
    const uint32_t c = (uint32_t)(e & TAB_CMAX);
    if (c == (uint32_t)TAB_CMAX || c == 0) return;               // (the big list: the host adds it)
    uint32_t w = w0, v = c;
    if (DECODE) {
        uint64_t keys[2];
        bool dbl;
        w = tab_entry_keys(((uint64_t)q << TAB_RBITS) | (e >> 20), a.k, a.plo, a.phi, a.pmask, a.canonical != 0, keys, &dbl);
        v = dbl ? 2 * c : c;
        if (!w) return;
    }
    if (v <= AB_REGS) {
#pragma unroll
        for (uint32_t i = 0; i < AB_REGS; ++i) r[i] += v == i + 1 ? w : 0u;
    } else if (v < AB_LDS_BINS) {
        atomicAdd(&bins[v], w);
    } else {
        atomicAdd(&a.hist[v], (unsigned long long)w);            // (v < 2^21: count < 2^20 - 1, doubled at most)
    }
}

// spectrum: the workgroup's LDS bins moved to the device histogram by one wave,
// while the other waves keep adding (an exchange takes what is there)
__device__ __forceinline__ void ab_flush(const TabAbund &a, uint32_t *bins, uint32_t lane) {
    for (uint32_t i = lane; i < AB_LDS_BINS; i += 64) {
        const uint32_t x = atomicExch(&bins[i], 0u);
        if (x) atomicAdd(&a.hist[i], (unsigned long long)x);
    }
}

// extract: an entry's Map keys (planar codes) and value; 0 keys when the value is out of range
__device__ __forceinline__ uint32_t ab_ext_entry(const TabAbund &a, uint64_t e, uint32_t q, uint64_t keys[2], uint64_t *v) {
    const uint64_t h = ((uint64_t)q << TAB_RBITS) | (e >> 20);
    bool dbl;
    const uint32_t n = tab_entry_keys(h, a.k, a.plo, a.phi, a.pmask, a.canonical != 0, keys, &dbl);
    *v = tab_value(a.big, a.n_big, true, e, h, dbl);
    return *v >= a.lo && *v <= a.hi ? n : 0u;
}

__device__ __forceinline__ void ab_put(const TabAbund &a, uint64_t slot, uint64_t key, uint64_t v) {
    if (slot < a.cap_out) {
        a.codes[slot] = tab_planar_code2(key, a.k);
        a.vals[slot] = v;
    } else {
        atomicOr(a.err, ERR_TAB_EXTRACT);                        // count and write passes disagree: a defect
    }
}

template <int MODE, bool DECODE>
__global__ __launch_bounds__(256) void tab_abund_kernel(const TabAbund a) {
    __shared__ uint32_t bins[MODE == AB_SPECTRUM ? AB_LDS_BINS : 1];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    const uint64_t table_end = tab_end(a);
    const uint32_t w0 = a.canonical ? 1u : 2u;                   // (no decode: every entry is w0 Map keys)
    if (MODE == AB_SPECTRUM) {
        for (uint32_t i = threadIdx.x; i < AB_LDS_BINS; i += blockDim.x) bins[i] = 0;
        __syncthreads();
    }
    uint64_t r[AB_REGS];
#pragma unroll
    for (uint32_t i = 0; i < AB_REGS; ++i) r[i] = 0;
    uint64_t mine = 0;                                           // count: this lane's keys in range
    uint32_t seen = 0;                                           // spectrum: weight since the wave's last flush (a bound)
    for (uint32_t g = wave; g < AB_GROUPS; g += nwaves) {        // (wave-uniform)
        const uint32_t q = (g << 6) + lane;
        uint64_t base;
        const uint32_t len = tab_extent(a, table_end, q, base);
        const uint32_t own = len <= TAB_LANE_MAX ? len : 0u;      // lane-per-bucket: no cross-lane reads inside
        if (MODE == AB_SPECTRUM) {
            for (uint32_t j = 0; j < own; ++j) ab_spec_entry<DECODE>(a, a.ent[base + j], q, w0, r, bins);
            seen += 64 * TAB_LANE_MAX * 2;
            if (seen >= AB_FLUSH) {                              // (wave-uniform)
                ab_flush(a, bins, lane);
                seen = 0;
            }
        } else if (MODE == AB_COUNT) {
            for (uint32_t j = 0; j < own; ++j) {
                uint64_t keys[2], v;
                mine += ab_ext_entry(a, a.ent[base + j], q, keys, &v);
            }
        } else {
            uint32_t t = 0;
            for (uint32_t j = 0; j < own; ++j) {
                uint64_t keys[2], v;
                t += ab_ext_entry(a, a.ent[base + j], q, keys, &v);
            }
            uint64_t slot = wave_reserve(a.n_out, t, lane);
            for (uint32_t j = 0; j < own; ++j) {
                uint64_t keys[2], v;
                const uint32_t n = ab_ext_entry(a, a.ent[base + j], q, keys, &v);
                for (uint32_t i = 0; i < n; ++i) ab_put(a, slot++, keys[i], v);
            }
        }
        uint64_t todo = __ballot(len > TAB_LANE_MAX);             // buckets the wave walks together
        while (todo) {                                           // (wave-uniform)
            const uint32_t j = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1;
            const uint64_t b = readlane64(base, j);
            const uint64_t Lj = readlane32(len, j);
            const uint32_t qj = (g << 6) + j;
            for (uint64_t o = 0; o < Lj; o += 64 * TAB_UNROLL) {  // (wave-uniform trip count)
                uint64_t e[TAB_UNROLL];
#pragma unroll
                for (uint32_t u = 0; u < TAB_UNROLL; ++u) {
                    const uint64_t p = o + u * 64 + lane;
                    e[u] = p < Lj ? a.ent[b + p] : 0;
                }
                if (MODE == AB_SPECTRUM) {
#pragma unroll
                    for (uint32_t u = 0; u < TAB_UNROLL; ++u)
                        if (o + u * 64 + lane < Lj) ab_spec_entry<DECODE>(a, e[u], qj, w0, r, bins);
                    seen += 64 * TAB_UNROLL * 2;
                    if (seen >= AB_FLUSH) {                      // (wave-uniform) before a bin can wrap
                        ab_flush(a, bins, lane);
                        seen = 0;
                    }
                } else if (MODE == AB_COUNT) {
#pragma unroll
                    for (uint32_t u = 0; u < TAB_UNROLL; ++u) {
                        uint64_t keys[2], v;
                        if (o + u * 64 + lane < Lj) mine += ab_ext_entry(a, e[u], qj, keys, &v);
                    }
                } else {
                    uint32_t t = 0;
#pragma unroll
                    for (uint32_t u = 0; u < TAB_UNROLL; ++u) {
                        uint64_t keys[2], v;
                        if (o + u * 64 + lane < Lj) t += ab_ext_entry(a, e[u], qj, keys, &v);
                    }
                    uint64_t slot = wave_reserve(a.n_out, t, lane);
#pragma unroll
                    for (uint32_t u = 0; u < TAB_UNROLL; ++u) {
                        uint64_t keys[2], v;
                        if (o + u * 64 + lane < Lj) {
                            const uint32_t n = ab_ext_entry(a, e[u], qj, keys, &v);
                            for (uint32_t i = 0; i < n; ++i) ab_put(a, slot++, keys[i], v);
                        }
                    }
                }
            }
        }
    }
    if (MODE == AB_SPECTRUM) {
#pragma unroll
        for (uint32_t i = 0; i < AB_REGS; ++i) {
            const uint64_t x = wave_sum(r[i]);
            if (lane == 0 && x) atomicAdd(&a.hist[i + 1], (unsigned long long)x);
        }
        __syncthreads();                                         // every wave's LDS adds are in
        for (uint32_t i = threadIdx.x; i < AB_LDS_BINS; i += blockDim.x) {
            const uint32_t x = bins[i];
            if (x) atomicAdd(&a.hist[i], (unsigned long long)x);
        }
    } else if (MODE == AB_COUNT) {
        mine = wave_sum(mine);
        if (lane == 0 && mine) atomicAdd(a.n_out, (unsigned long long)mine);
    }
}

// out[0] = sum of hist[from ..], out[1] = sum of v hist[v] over the same bins (the spectrum's last bin)
__global__ __launch_bounds__(256) void tab_spectrum_tail_kernel(const unsigned long long *hist, uint32_t from,
                                                                unsigned long long *out) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t n = 0, s = 0;
    for (uint32_t v = from + blockIdx.x * blockDim.x + threadIdx.x; v < AB_HIST_BINS; v += gridDim.x * blockDim.x) {
        const uint64_t x = hist[v];
        n += x;
        s += x * v;
    }
    n = wave_sum(n);
    s = wave_sum(s);
    if (lane == 0 && n) {
        atomicAdd(&out[0], (unsigned long long)n);
        atomicAdd(&out[1], (unsigned long long)s);
    }
}

// keys[i k .. (i + 1) k) = the bytes of 2-bit code codes[i]; a thread writes 4 bytes
__global__ __launch_bounds__(256) void tab_extract_decode_kernel(const uint64_t *codes, uint64_t n, uint32_t k,
                                                                 uint8_t *keys) {
    const uint64_t bytes = n * k;
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t * 4 < bytes; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p = t * 4;
        uint64_t i = p / k;
        uint32_t j = (uint32_t)(p - i * k);
        uint64_t c = codes[i];
        uint32_t word = 0, m = 0;
        for (; m < 4 && p + m < bytes; ++m) {
            const uint32_t d = (uint32_t)(c >> (2 * (k - 1 - j))) & 3u;
            word |= ((0x54474341u >> (8 * d)) & 0xFFu) << (8 * m);   // "ACGT"[d]
            if (++j == k && p + m + 1 < bytes) {
                j = 0;
                c = codes[++i];
            }
        }
        if (m == 4) {
            *(uint32_t *)(keys + p) = word;
        } else {
            for (uint32_t x = 0; x < m; ++x) keys[p + x] = (uint8_t)(word >> (8 * x));
        }
    }
}

// one group of 64 buckets per wave: workgroups beyond the resident ones start
// as others end, which evens out unequal groups
constexpr uint32_t AB_GRID = AB_GROUPS / 4;

hipError_t launch_tab_spectrum(const TabAbund &a, hipStream_t s) {
    const bool plain = a.pmask == 0 && (a.canonical || (a.k & 1));   // no prefix, no palindromes: nothing to decode
    if (plain)
        hipLaunchKernelGGL((tab_abund_kernel<AB_SPECTRUM, false>), dim3(AB_GRID), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((tab_abund_kernel<AB_SPECTRUM, true>), dim3(AB_GRID), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tab_spectrum_tail(const unsigned long long *hist, uint32_t from, unsigned long long *out,
                                    hipStream_t s) {
    if (from >= AB_HIST_BINS) return hipSuccess;
    const uint32_t grid = std::min<uint32_t>((AB_HIST_BINS - from + 255) / 256, 1024);
    hipLaunchKernelGGL(tab_spectrum_tail_kernel, dim3(grid), dim3(256), 0, s, hist, from, out);
    return hipGetLastError();
}

hipError_t launch_tab_extract_count(const TabAbund &a, hipStream_t s) {
    hipLaunchKernelGGL((tab_abund_kernel<AB_COUNT, true>), dim3(AB_GRID), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tab_extract_write(const TabAbund &a, hipStream_t s) {
    hipLaunchKernelGGL((tab_abund_kernel<AB_WRITE, true>), dim3(AB_GRID), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t tab_extract_sort_bytes(uint64_t n, uint32_t k, size_t *bytes) {
    rocprim::double_buffer<uint64_t> kb(nullptr, nullptr), vb(nullptr, nullptr);
    *bytes = 0;
    return rocprim::radix_sort_pairs(nullptr, *bytes, kb, vb, (size_t)std::max<uint64_t>(n, 1), 0, 2 * k, nullptr);
}

hipError_t launch_tab_extract_sort(uint64_t *codes, uint64_t *codes2, uint64_t *vals, uint64_t *vals2, uint64_t n,
                                   uint32_t k, void *tmp, size_t tmp_bytes, const uint64_t **sorted_codes,
                                   const uint64_t **sorted_vals, hipStream_t s) {
    rocprim::double_buffer<uint64_t> kb(codes, codes2), vb(vals, vals2);
    const hipError_t e = rocprim::radix_sort_pairs(tmp, tmp_bytes, kb, vb, (size_t)n, 0, 2 * k, s);
    *sorted_codes = kb.current();
    *sorted_vals = vb.current();
    return e;
}

hipError_t launch_tab_extract_decode(const uint64_t *codes, uint64_t n, uint32_t k, uint8_t *keys, uint32_t n_cu,
                                     hipStream_t s) {
    if (!n) return hipSuccess;
    const uint64_t threads = (n * k + 3) / 4;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((threads + 255) / 256, (uint64_t)std::max(n_cu, 1u) * 16);
    hipLaunchKernelGGL(tab_extract_decode_kernel, dim3(grid), dim3(256), 0, s, codes, n, k, keys);
    return hipGetLastError();
}

}  // namespace kmerhip
