// kmer_device.hpp — device helpers shared by the kernel translation units
// (kmer_kernels.hip, kmer_table.hip, kmer_dense.hip, kmer_fasta.hip,
// kmer_lookup.hip, kmer_probe.hip, kmer_abundance.hip, kmer_setops.hip,
// kmer_screen.hip, kmer_filter.hip, kmer_dbfasta.hip): one
// definition of each primitive that more than one kernel uses.  The
// host/device contract (structs, constants, launch_* declarations) is
// kmer_internal.hpp.
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

}  // namespace kmerhip
