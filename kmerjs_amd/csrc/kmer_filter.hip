// kmer_filter.hip — the records of screened reads, kept or dropped by their
// rows and compacted on the device (gfx950): kmer_table_filter /
// kmer_table_filter_device.  The screen itself (kmer_screen.hip) runs first and
// unchanged; this file works from its rows and from the '\n' positions the
// line finder (chunk_lines) left behind.
//
//   ends      rend[r]: the end of record r -- one past '\n' number 4r + 3, or
//             the input's end when there is none.  From the per-tile slots (a
//             wave per tile, as seq_lines_slots_kernel) or from the flat
//             position array (a lane per record, as seq_lines_kernel),
//             whichever chunk_lines produced.  Record r begins at rend[r - 1].
//   mark      keep[r] from the shared predicate (filter_match) on the read's
//             row, the mate's row under FILTER_PAIRED, negated under
//             FILTER_DROP; and per record (kept, kept bytes, "a kept run begins
//             here"), which the host scans (rocprim, FilterScanPlus).
//   segments  a maximal run of kept records is one contiguous source range:
//             its (source begin, output begin) at the run's index; the entry
//             after the last holds out_len.
//   copy      organised from the output: a workgroup tile is FL_TILE output
//             bytes, a lane produces one aligned 16-byte store.  The tile's
//             segments [j0, j1] are found once per tile by wave-uniform binary
//             searches (scalar loads), their bounds are staged in LDS, and a
//             lane of a tile with several segments searches LDS only.  A chunk
//             inside one segment loads five aligned source dwords and shifts
//             them into place; a chunk across a segment boundary, at the
//             output's end, or whose dwords would touch bytes outside the
//             input takes the byte path.  One writer per output byte, no
//             atomics; no load outside [data, data + len); stores end at
//             out_len rounded up to 16, inside the padded buffer.
// No cross-lane operation but the workgroup barriers, which sit at the
// wave-uniform level of the tile loop.
#include "kmer_device.hpp"

#include <algorithm>

namespace kmerhip {

constexpr uint32_t FL_WG_PER_CU = 8;     // workgroups of the copy per CU

namespace {

__device__ __forceinline__ bool fl_keep(const FilterArgs &a, uint64_t r) {
    const ScreenRow x = a.rows[r];
    bool m = filter_match(x.hits, x.windows, a.min_hits, a.frac_num, a.frac_den);
    if ((a.flags & FILTER_PAIRED) && (r ^ 1) < a.n_reads) {      // (a last record without a mate: judged alone)
        const ScreenRow y = a.rows[r ^ 1];
        m = m || filter_match(y.hits, y.windows, a.min_hits, a.frac_num, a.frac_den);
    }
    return m != ((a.flags & FILTER_DROP) != 0);
}

}  // namespace

__global__ __launch_bounds__(256) void filter_ends_kernel(const FilterArgs a) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nthr = (uint64_t)gridDim.x * blockDim.x;
    // the last record when '\n' number 4 (n_reads - 1) + 3 does not exist: it runs to the input's end
    if (gid == 0 && a.n_reads && 4 * a.n_reads > a.n_nl) a.rend[a.n_reads - 1] = a.len;
    if (a.slots) {
        const uint32_t lane = threadIdx.x & 63u;
        for (uint64_t tile = gid >> 6; tile < a.n_tiles; tile += nthr >> 6) {   // (wave-uniform)
            const uint32_t n = a.tcount[tile];
            const uint64_t rb = a.tbase[tile];
            const uint16_t *src = a.slots + tile * a.cap;
            for (uint32_t i = lane; i < n; i += 64) {
                const uint64_t q = rb + i;                               // '\n' number q ends line q
                if ((q & 3) == 3) a.rend[q >> 2] = tile * TILE + src[i] + 1;
            }
        }
    } else {
        for (uint64_t r = gid; r < a.n_reads; r += nthr) {
            const uint64_t q = 4 * r + 3;
            if (q < a.n_nl) a.rend[r] = a.nl[q] + 1;
        }
    }
}

__global__ __launch_bounds__(256) void filter_mark_kernel(const FilterArgs a) {
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.n_reads;
         r += (uint64_t)gridDim.x * blockDim.x) {
        const bool k = fl_keep(a, r);
        const bool head = k && !(r && fl_keep(a, r - 1));
        const uint64_t b = r ? a.rend[r - 1] : 0;
        FilterScan f;
        f.kept = k ? 1 : 0;
        f.bytes = k ? a.rend[r] - b : 0;
        f.segs = head ? 1 : 0;
        a.keep[r] = k ? 1 : 0;
        a.scan[r] = f;
    }
}

// (after the inclusive scan of a.scan)
__global__ __launch_bounds__(256) void filter_segments_kernel(const FilterArgs a) {
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.n_reads;
         r += (uint64_t)gridDim.x * blockDim.x) {
        const FilterScan f = a.scan[r];
        if (a.keep[r] && !(r && a.keep[r - 1])) {                // the one writer of run f.segs - 1
            const uint64_t b = r ? a.rend[r - 1] : 0;
            a.seg_src[f.segs - 1] = b;
            a.seg_out[f.segs - 1] = f.bytes - (a.rend[r] - b);
        }
        if (r == a.n_reads - 1) a.seg_out[f.segs] = f.bytes;
    }
}

__global__ __launch_bounds__(256) void filter_copy_kernel(const FilterArgs a) {
    __shared__ uint64_t s_out[FL_SEGS], s_src[FL_SEGS];
    const uint32_t tid = threadIdx.x;
    const uint64_t n_tiles = (a.out_len + FL_TILE - 1) / FL_TILE;
    const uint64_t base = (uint64_t)(uintptr_t)a.data, end = base + a.len;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {         // (workgroup-uniform)
        const uint64_t tb = t * FL_TILE;
        const uint64_t te = tb + FL_TILE < a.out_len ? tb + FL_TILE : a.out_len;
        // j0: the segment that holds output byte tb (seg_out[0] = 0, seg_out[n_segs] = out_len > tb)
        uint64_t lo = 0, hi = a.n_segs;
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (a.seg_out[mid] <= tb) lo = mid;
            else hi = mid;
        }
        const uint64_t j0 = lo;
        // j1: the segment that holds byte te - 1; one segment for the whole tile is the common case
        uint64_t j1 = j0;
        if (a.seg_out[j0 + 1] < te) {
            lo = j0 + 1;
            hi = a.n_segs;                                               // seg_out[lo] < te <= seg_out[hi]
            while (hi - lo > 1) {
                const uint64_t mid = (lo + hi) >> 1;
                if (a.seg_out[mid] < te) lo = mid;
                else hi = mid;
            }
            j1 = lo;
        }
        // (a segment is >= 4 bytes, so a tile holds <= FL_TILE / 4 + 1 of them; the clamp only guards the LDS arrays)
        const uint32_t ns = (uint32_t)(j1 - j0 + 1 < FL_SEGS - 1 ? j1 - j0 + 1 : FL_SEGS - 1);
        for (uint32_t i = tid; i <= ns; i += 256) {
            s_out[i] = a.seg_out[j0 + i];
            if (i < ns) s_src[i] = a.seg_src[j0 + i];
        }
        __syncthreads();
        const uint64_t o = tb + 16 * tid;
        if (o < te) {
            uint32_t ls = 0;                                             // the segment of output byte o
            if (ns > 1) {
                uint32_t l2 = 0, h2 = ns;                                // s_out[l2] <= o < s_out[h2]
                while (h2 - l2 > 1) {
                    const uint32_t mid = (l2 + h2) >> 1;
                    if (s_out[mid] <= o) l2 = mid;
                    else h2 = mid;
                }
                ls = l2;
            }
            uint32_t w[4] = {0, 0, 0, 0};
            const uint64_t src = s_src[ls] + (o - s_out[ls]);
            const uint64_t al = (base + src) & ~3ull;
            if (o + 16 <= s_out[ls + 1] && al >= base && al + 20 <= end) {
                const uint32_t *p = (const uint32_t *)(uintptr_t)al;
                const uint32_t sh = 8 * (uint32_t)((base + src) & 3);
                uint32_t x[5];
#pragma unroll
                for (int i = 0; i < 5; ++i) x[i] = p[i];
#pragma unroll
                for (int i = 0; i < 4; ++i) w[i] = (uint32_t)((((uint64_t)x[i + 1] << 32) | x[i]) >> sh);
            } else {
                uint32_t i = ls;
                for (uint32_t b = 0; b < 16; ++b) {
                    const uint64_t ob = o + b;
                    if (ob >= te) break;
                    while (i + 1 < ns && ob >= s_out[i + 1]) ++i;
                    w[b >> 2] |= (uint32_t)a.data[s_src[i] + (ob - s_out[i])] << (8 * (b & 3));
                }
            }
            *(uint4 *)(a.out + o) = make_uint4(w[0], w[1], w[2], w[3]);
        }
        __syncthreads();                                                 // (the next tile restages s_out / s_src)
    }
}

static uint32_t fl_grid(uint64_t n) {
    return (uint32_t)std::min<uint64_t>((n + 255) / 256, 1u << 14);
}

hipError_t launch_filter_ends(const FilterArgs &a, hipStream_t s) {
    if (a.n_reads == 0) return hipSuccess;
    const uint64_t n = a.slots ? (uint64_t)a.n_tiles * 64 : a.n_reads;
    hipLaunchKernelGGL(filter_ends_kernel, dim3(fl_grid(n)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_filter_mark(const FilterArgs &a, hipStream_t s) {
    if (a.n_reads == 0) return hipSuccess;
    hipLaunchKernelGGL(filter_mark_kernel, dim3(fl_grid(a.n_reads)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_filter_segments(const FilterArgs &a, hipStream_t s) {
    if (a.n_reads == 0) return hipSuccess;
    hipLaunchKernelGGL(filter_segments_kernel, dim3(fl_grid(a.n_reads)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_filter_copy(const FilterArgs &a, uint32_t n_cu, hipStream_t s) {
    if (a.out_len == 0 || a.n_segs == 0) return hipSuccess;
    const uint64_t tiles = (a.out_len + FL_TILE - 1) / FL_TILE;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(tiles, (uint64_t)std::max(n_cu, 1u) * FL_WG_PER_CU);
    hipLaunchKernelGGL(filter_copy_kernel, dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace kmerhip
