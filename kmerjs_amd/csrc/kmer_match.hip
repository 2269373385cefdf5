// kmer_match.hip — k-mer -> template matching on the GPU (include/kmer_match.h).
//
// kmerFinder scores reference genomes ("templates") by the query k-mers they
// share (lib/kmerFinderServer.js:171-226, :736-849).  The reference does one
// Redis lrange per query k-mer and folds the lists into a JS Map, then loops
// winner-takes-all: the template with the most shared k-mers wins, its k-mers
// leave the query, everything is re-scored.  Here:
//
//   DB (once):  k-mers packed to 2-bit codes, (code, template) pairs radix
//               sorted (stable: a k-mer's templates stay in DB order), dedup,
//               CSR: U[m] sorted distinct codes, O[m + 1] list offsets, T[] templates.
//               The pairs come from the caller's host strings (kmer_db_open:
//               upload + pack) or from FASTA genomes on the device
//               (kmer_db_open_fasta*: kmer_dbfasta.hip gathers them over a
//               counting context); everything from the sort on is shared
//               (build_from_pairs).
//   round 1:    each query key packed and binary-searched in U; hits expanded to
//               (template, query) pairs in (query, list) order, radix sorted by
//               template (stable) -> per-template segments of query indices:
//               uScore = segment length, tScore = sum of counts (one wave per
//               template), first hit = the segment's first query.  Templates
//               ranked by (first query, template) = the Redis Map's insertion order.
//               A table-mode count as the query (kmer_match_open_table): the
//               join runs from the DB's side -- every U[i] is probed in the
//               count's device table (kmer_probe.hip) and query index i IS DB
//               k-mer i; everything from the hit counts' scan on is shared.
//   winner:     one workgroup: max of uScore << 32 | ~rank.
//   remove:     the winner's segment: each query k-mer still present is
//               removed (atomic exchange) and its templates' scores drop.
//
// All integer work; the join is a few random reads per query key and the
// remove touches only the winner's k-mers.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kmer_match.h"
#include "kmer_internal.hpp"

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;
thread_local std::string g_err;

kmer_status set_err(kmer_status s, const std::string &msg) {
    g_err = msg;
    return s;
}

#define MCHK(x)                                                                      \
    do {                                                                             \
        hipError_t e_ = (x);                                                         \
        if (e_ != hipSuccess) return set_err(KMER_E_DEVICE, std::string("HIP error: ") + hipGetErrorString(e_) + " at " #x); \
    } while (0)

template <typename T>
hipError_t dalloc(T **p, uint64_t n) {
    return hipMalloc((void **)p, std::max<uint64_t>(n, 1) * sizeof(T));
}

struct Temp {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) cap = n;
        return e;
    }
    ~Temp() {
        if (p) (void)hipFree(p);
    }
};

// grow-only device array (buffers are reused by the next match on the DB)
template <typename T>
struct DArr {
    T *p = nullptr;
    uint64_t cap = 0;
    hipError_t ensure(uint64_t n) {
        n = std::max<uint64_t>(n, 1);
        if (n <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipMalloc((void **)&p, std::max(n, cap + cap / 2) * sizeof(T));
        if (e == hipSuccess) cap = std::max(n, cap + cap / 2);
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

#define MROC(tmp, CALL)                       \
    do {                                      \
        size_t b = 0;                         \
        void *t = nullptr;                    \
        MCHK(CALL);                           \
        MCHK((tmp).ensure(b + 16));           \
        t = (tmp).p;                          \
        MCHK(CALL);                           \
    } while (0)

int bit_width64(uint64_t x) {
    int b = 0;
    while (x) {
        ++b;
        x >>= 1;
    }
    return b;
}

__device__ __forceinline__ int base2(uint32_t c) {
    return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
}

__device__ __forceinline__ bool pack_key(const uint8_t *p, uint32_t k, uint64_t *code) {
    uint64_t v = 0;
    bool ok = true;
    for (uint32_t i = 0; i < k; ++i) {
        const int b = base2(p[i]);
        ok &= b >= 0;
        v = (v << 2) | (uint64_t)(b & 3);
    }
    *code = v;
    return ok;
}

// ---------------------------------------------------------------------------
// DB kernels
// ---------------------------------------------------------------------------
__global__ void db_pack_kernel(const uint8_t *keys, uint64_t n, uint32_t k, uint64_t *codes, uint32_t *bad) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t c;
        if (!pack_key(keys + i * k, k, &c)) atomicOr(bad, 1u);
        codes[i] = c;
    }
}

// entry -> template (template t owns [ts[t], ts[t + 1]))
__global__ void db_tmpl_kernel(const uint64_t *ts, uint32_t nt, uint32_t *tmpl) {
    for (uint32_t t = blockIdx.x; t < nt; t += gridDim.x)
        for (uint64_t i = ts[t] + threadIdx.x; i < ts[t + 1]; i += blockDim.x) tmpl[i] = t;
}

// after the (code, template) sort: keep = not a repeated pair, head = first of its code
struct KeepHead {
    const uint64_t *c;
    const uint32_t *t;
    __device__ uint64_t operator()(uint64_t i) const {
        const bool head = i == 0 || c[i] != c[i - 1];
        const bool keep = head || t[i] != t[i - 1];
        return (keep ? 1ull : 0ull) | (head ? 1ull << 32 : 0ull);
    }
};

__global__ void db_csr_kernel(const uint64_t *c, const uint32_t *t, uint64_t n, const uint64_t *pos, uint64_t *U,
                              uint64_t *O, uint32_t *T) {
    KeepHead kh{c, t};
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t f = kh(i), p = pos[i];
        const uint64_t e = p & 0xFFFFFFFFull, u = p >> 32;
        if (f & 1) T[e] = t[i];
        if (f >> 32) {
            U[u] = c[i];
            O[u] = e;
        }
    }
}

// dir[p] = first U index whose code >> dsh is >= (dlo >> dsh) + p (p = 0 .. np)
__global__ void db_dir_kernel(const uint64_t *U, uint64_t m, uint64_t dlo, uint32_t dsh, uint64_t np, uint32_t *dir) {
    for (uint64_t p = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; p <= np; p += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t cell = (dlo >> dsh) + p;
        uint64_t lo = 0, hi = m;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if ((U[mid] >> dsh) < cell) lo = mid + 1;
            else hi = mid;
        }
        dir[p] = (uint32_t)lo;
    }
}

// ---------------------------------------------------------------------------
// query kernels
// ---------------------------------------------------------------------------
// pack + directory + binary search: qidx = DB k-mer index or NONE, hc = its
// list length.  The directory cell of a code (its bits above dsh, relative to
// the smallest DB code) bounds the search to a few entries.
__global__ void q_lookup_kernel(const uint8_t *keys, const uint64_t *offs, uint32_t klen, uint64_t n, uint32_t k,
                                const uint64_t *U, uint64_t m, const uint64_t *O, const uint32_t *dir, uint64_t dlo,
                                uint64_t dhi, uint32_t dsh, uint32_t *qidx, uint64_t *hc, uint32_t *present) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t b = offs ? offs[i] : i * klen;
        const uint64_t len = offs ? offs[i + 1] - b : klen;
        uint32_t idx = NONE;
        uint64_t code;
        if (len == k && m && pack_key(keys + b, k, &code) && code >= dlo && code <= dhi) {
            const uint64_t p = (code >> dsh) - (dlo >> dsh);
            uint64_t lo = dir[p], hi = dir[p + 1];      // first U[j] >= code, inside its directory cell
            while (lo < hi) {
                const uint64_t mid = (lo + hi) >> 1;
                if (U[mid] < code) lo = mid + 1;
                else hi = mid;
            }
            if (lo < m && U[lo] == code) idx = (uint32_t)lo;
        }
        qidx[i] = idx;
        hc[i] = idx == NONE ? 0 : O[idx + 1] - O[idx];
        present[i] = idx == NONE ? 0u : 1u;
    }
}

// hits in (query, list) order as (template, query) pairs, load-balanced: a
// wave takes 64 consecutive query keys and its lanes walk the wave's hits in
// order (lane-strided), each finding its owner key by a 6-step search over
// the lanes' hit offsets -- coalesced stores, no per-key loop imbalance.
__global__ __launch_bounds__(256) void q_emit_kernel(const uint32_t *qidx, const uint64_t *H, uint64_t n,
                                                     const uint64_t *O, const uint32_t *T, uint32_t *pt, uint32_t *pq) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t w0 = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) & ~63ull; w0 < n;
         w0 += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = w0 + lane;
        const uint32_t idx = i < n ? qidx[i] : NONE;
        const uint64_t o = idx == NONE ? 0 : O[idx], c = idx == NONE ? 0 : O[idx + 1] - o;
        const uint64_t h = i < n ? H[i] : ~0ull;                // (past the end: never an owner)
        uint64_t end = i < n ? h + c : 0;
        for (int d = 32; d >= 1; d >>= 1) {
            const uint64_t x = __shfl_xor(end, d);
            end = x > end ? x : end;
        }
        const uint64_t start = __shfl(h, 0);
        // (wave-uniform trip count: every lane takes part in the shuffles)
        for (uint64_t r = start; r < end; r += 64) {
            const uint64_t e = r + lane;
            int lo = 0, hi = 63;                                // the last lane with h <= e owns e
#pragma unroll
            for (int it = 0; it < 6; ++it) {
                const int mid = (lo + hi + 1) >> 1;
                if (__shfl(h, mid) <= e) lo = mid;
                else hi = mid - 1;
            }
            const uint64_t hl = __shfl(h, lo), ol = __shfl(o, lo);
            if (e < end) {
                pt[e] = T[ol + (e - hl)];
                pq[e] = (uint32_t)(w0 + (uint64_t)lo);
            }
        }
    }
}

// seg[t] = first sorted hit of template >= t (t = 0 .. nt)
__global__ void q_seg_kernel(const uint32_t *st, uint64_t hits, uint32_t nt, uint64_t *seg) {
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t <= nt; t += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t lo = 0, hi = hits;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (st[mid] < t) lo = mid + 1;
            else hi = mid;
        }
        seg[t] = lo;
    }
}

// one wave per template: round-1 scores and its first-hit sort key
__global__ __launch_bounds__(256) void q_score_kernel(const uint64_t *seg, const uint32_t *sq, const uint64_t *cnt,
                                                      uint32_t nt, uint32_t *u0, uint64_t *t0, uint32_t *cu,
                                                      uint64_t *ct, uint64_t *fkey, uint32_t *nh) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t t = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6; t < nt;
         t += ((uint64_t)gridDim.x * blockDim.x) >> 6) {
        const uint64_t a = seg[t], b = seg[t + 1];
        uint64_t s = 0;
        for (uint64_t e = a + lane; e < b; e += 64) s += cnt[sq[e]];
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
        if (lane == 0) {
            const uint32_t u = (uint32_t)(b - a);
            u0[t] = u;
            cu[t] = u;
            t0[t] = s;
            ct[t] = s;
            fkey[t] = u ? ((uint64_t)sq[a] << 32) | t : ~0ull;
            if (u) atomicAdd(nh, 1u);
        }
    }
}

__global__ void q_order_kernel(const uint64_t *skey, uint32_t nh, uint32_t *order, uint32_t *rank) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < nh; r += gridDim.x * blockDim.x) {
        const uint32_t t = (uint32_t)skey[r];
        order[r] = t;
        rank[t] = r;
    }
}

// scal: [0] hits left; winner written to *w
__global__ __launch_bounds__(1024) void winner_kernel(const uint32_t *order, uint32_t nh, const uint32_t *cu,
                                                      const uint64_t *ct, const uint32_t *u0, const uint64_t *t0,
                                                      const uint64_t *scal, kmer_winner *w) {
    __shared__ uint64_t part[16];
    uint64_t best = 0;
    for (uint32_t r = threadIdx.x; r < nh; r += blockDim.x) {
        const uint32_t u = cu[order[r]];
        const uint64_t key = u ? ((uint64_t)u << 32) | (0xFFFFFFFFu - r) : 0;
        best = key > best ? key : best;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o = __shfl_xor(best, d);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t i = 1; i < blockDim.x / 64; ++i) best = part[i] > best ? part[i] : best;
        kmer_winner o;
        memset(&o, 0, sizeof(o));
        o.tmpl = NONE;
        o.hits = scal[0];
        if (best) {
            const uint32_t t = order[0xFFFFFFFFu - (uint32_t)best];
            o.tmpl = t;
            o.uscore = cu[t];
            o.tscore = ct[t];
            o.first_uscore = u0[t];
            o.first_tscore = t0[t];
        }
        *w = o;
    }
}

// removeWinnerKmers: the winner's query k-mers still present leave the query
__global__ void remove_kernel(const uint64_t *seg, const uint32_t *sq, uint32_t w, uint32_t *present,
                              const uint32_t *qidx, const uint64_t *O, const uint32_t *T, const uint64_t *cnt,
                              uint32_t *cu, uint64_t *ct, uint64_t *scal) {
    const uint64_t a = seg[w], b = seg[w + 1];
    for (uint64_t e = a + blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < b;
         e += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t q = sq[e];
        if (atomicExch(&present[q], 0u) == 0u) continue;
        const uint32_t idx = qidx[q];
        const uint64_t o = O[idx], len = O[idx + 1] - o, c = cnt[q];
        for (uint64_t j = 0; j < len; ++j) {
            const uint32_t t = T[o + j];
            atomicSub(&cu[t], 1u);
            atomicAdd((unsigned long long *)&ct[t], (unsigned long long)(0ull - c));
        }
        atomicAdd((unsigned long long *)&scal[0], (unsigned long long)(0ull - len));
    }
}

__global__ void removed_kernel(const uint32_t *qidx, const uint32_t *present, uint64_t n, uint8_t *flags) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        flags[i] = qidx[i] != NONE && present[i] == 0u ? 1 : 0;
}

// U[first + i] -> its k bytes
__global__ void db_decode_kernel(const uint64_t *U, uint64_t first, uint64_t n, uint32_t k, uint8_t *keys) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t c = U[first + i];
        for (uint32_t j = 0; j < k; ++j) keys[i * k + j] = (uint8_t)"ACGT"[(c >> (2 * (k - 1 - j))) & 3u];
    }
}

// DB k-mer i has template t in its (ascending) list
struct HasTemplate {
    const uint64_t *O;
    const uint32_t *T;
    uint32_t t;
    __device__ bool operator()(uint32_t i) const {
        uint64_t lo = O[i], hi = O[i + 1];
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (T[mid] < t) lo = mid + 1;
            else hi = mid;
        }
        return lo < O[i + 1] && T[lo] == t;
    }
};

uint32_t grid_for(uint64_t n, uint32_t block = 256, uint32_t cap = 65536) {
    const uint64_t g = (n + block - 1) / block;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(g, cap));
}

}  // namespace

// Per-match arrays; a closed match hands them to its DB for the next one.
struct MatchBufs {
    DArr<uint64_t> cnt, H, seg, t0, ct, scal;
    DArr<uint32_t> qidx, present, sq, u0, cu, order, rank;
    DArr<kmer_winner> dw;
    kmer_winner *hw = nullptr;
    void release() {
        cnt.release(), H.release(), seg.release(), t0.release(), ct.release(), scal.release();
        qidx.release(), present.release(), sq.release(), u0.release(), cu.release(), order.release(), rank.release();
        dw.release();
        if (hw) (void)hipHostFree(hw);
        hw = nullptr;
    }
};

struct kmer_db {
    int device = 0;
    uint32_t k = 0, nt = 0;
    uint64_t m = 0, entries = 0;
    hipStream_t s = nullptr;
    uint64_t *U = nullptr, *O = nullptr;
    uint32_t *T = nullptr;
    uint32_t *dir = nullptr;                   // directory over the codes' high bits
    uint64_t dlo = ~0ull, dhi = 0;
    uint32_t dsh = 0;
    // scratch of a match build (matches of one DB are built one at a time)
    DArr<uint8_t> qkeys;
    DArr<uint64_t> qoffs, hc, fkey, fkey2;
    DArr<uint32_t> pt, pt2, pq2, nhd;
    DArr<uint32_t> pb_bkt, pb_bkt2, pb_idx, pb_idx2;   // table probe: (bucket, DB index) pairs, sorted
    Temp tmp;
    MatchBufs spare;                           // buffers of the last closed match
    bool has_spare = false;
    uint32_t live = 0;                         // open matches
    bool closing = false;                      // kmer_db_close called while matches were open
    // per template (host): keys handed in / FASTA window keys, entries after dedup, names (FASTA DBs)
    std::vector<uint64_t> lengths, ulengths, name_off;
    std::string names;
};

struct kmer_match {
    kmer_db *db = nullptr;
    uint64_t n = 0, hits0 = 0;
    uint32_t nh = 0;
    MatchBufs b;
    uint64_t *cnt = nullptr, *H = nullptr, *seg = nullptr, *t0 = nullptr, *ct = nullptr, *scal = nullptr;
    uint32_t *qidx = nullptr, *present = nullptr, *sq = nullptr, *u0 = nullptr, *cu = nullptr, *order = nullptr,
             *rank = nullptr;
    kmer_winner *dw = nullptr, *hw = nullptr;
    void release() {
        if (!db->has_spare) {                  // keep the buffers for the DB's next match
            db->spare = b;
            db->has_spare = true;
        } else {
            b.release();
        }
        b = MatchBufs();
    }
};

namespace {

void free_db(kmer_db *db) {
    if (!db) return;
    (void)hipSetDevice(db->device);
    if (db->U) (void)hipFree(db->U);
    if (db->O) (void)hipFree(db->O);
    if (db->T) (void)hipFree(db->T);
    if (db->dir) (void)hipFree(db->dir);
    db->qkeys.release(), db->qoffs.release(), db->hc.release(), db->fkey.release(), db->fkey2.release();
    db->pt.release(), db->pt2.release(), db->pq2.release(), db->nhd.release();
    db->pb_bkt.release(), db->pb_bkt2.release(), db->pb_idx.release(), db->pb_idx2.release();
    if (db->has_spare) db->spare.release();
    if (db->s) (void)hipStreamDestroy(db->s);
    delete db;
}

// The DB from n (code, template) pairs in device memory, duplicates included,
// a k-mer's templates in ascending order among its pairs (template-major input
// and the stable sort): sort, dedup, CSR, directory, entries per template.  c
// and t are sorted in place (they stay the caller's); queued on the DB's
// stream, which the caller's writers of c and t must have been waited for.
kmer_status build_from_pairs(kmer_db *db, uint64_t *c, uint32_t *t, uint64_t n) {
    hipStream_t s = db->s;
    Temp tmp;
    uint64_t *c2 = nullptr, *pos = nullptr, *seg = nullptr;
    uint32_t *t2 = nullptr, *e1 = nullptr, *e2 = nullptr;
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(s);
        for (void *p : {(void *)c2, (void *)pos, (void *)seg, (void *)t2, (void *)e1, (void *)e2})
            if (p) (void)hipFree(p);
    };
    struct Guard {
        decltype(cleanup) &f;
        ~Guard() { f(); }
    } guard{cleanup};
    db->ulengths.assign(db->nt, 0);
    if (n == 0) {
        MCHK(dalloc(&db->O, 1));
        MCHK(hipMemsetAsync(db->O, 0, 8, s));
        MCHK(hipStreamSynchronize(s));
        return KMER_OK;
    }
    MCHK(dalloc(&c2, n));
    MCHK(dalloc(&t2, n));
    MCHK(dalloc(&pos, n));
    rocprim::double_buffer<uint64_t> kb(c, c2);
    rocprim::double_buffer<uint32_t> vb(t, t2);
    MROC(tmp, rocprim::radix_sort_pairs(t, b, kb, vb, (size_t)n, 0, 2 * db->k, s));
    const uint64_t *sc = kb.current();
    const uint32_t *stt = vb.current();
    rocprim::counting_iterator<uint64_t> iota(0);
    auto flags = rocprim::make_transform_iterator(iota, KeepHead{sc, stt});
    MROC(tmp, rocprim::exclusive_scan(t, b, flags, pos, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), s));
    uint64_t last[2] = {0, 0};
    MCHK(hipMemcpyAsync(&last[0], pos + n - 1, 8, hipMemcpyDeviceToHost, s));
    MCHK(hipStreamSynchronize(s));
    // (the last entry's own flags: recomputed on the host from the two sorted tails)
    uint64_t tail_c[2] = {0, 0};
    uint32_t tail_t[2] = {0, 0};
    MCHK(hipMemcpy(tail_c, sc + (n >= 2 ? n - 2 : 0), 8 * std::min<uint64_t>(n, 2), hipMemcpyDeviceToHost));
    MCHK(hipMemcpy(tail_t, stt + (n >= 2 ? n - 2 : 0), 4 * std::min<uint64_t>(n, 2), hipMemcpyDeviceToHost));
    bool head = n == 1 || tail_c[1] != tail_c[0];
    bool keep = head || tail_t[1] != tail_t[0];
    db->entries = (last[0] & 0xFFFFFFFFull) + (keep ? 1 : 0);
    db->m = (last[0] >> 32) + (head ? 1 : 0);
    if (db->entries >= NONE || db->m >= NONE)
        return set_err(KMER_E_BAD_PARAM, "kmer_db_open: more than 2^32 - 2 DB entries");
    MCHK(dalloc(&db->U, db->m));
    MCHK(dalloc(&db->O, db->m + 1));
    MCHK(dalloc(&db->T, db->entries));
    hipLaunchKernelGGL(db_csr_kernel, dim3(grid_for(n)), dim3(256), 0, s, sc, stt, n, pos, db->U, db->O, db->T);
    MCHK(hipGetLastError());
    MCHK(hipMemcpyAsync(db->O + db->m, &db->entries, 8, hipMemcpyHostToDevice, s));
    // directory: up to 2^20 cells over the bits below the codes' common prefix
    MCHK(hipMemcpyAsync(&db->dlo, db->U, 8, hipMemcpyDeviceToHost, s));
    MCHK(hipMemcpyAsync(&db->dhi, db->U + db->m - 1, 8, hipMemcpyDeviceToHost, s));
    MCHK(hipStreamSynchronize(s));
    const int span = bit_width64(db->dlo ^ db->dhi);
    db->dsh = (uint32_t)std::max(0, span - 20);
    const uint64_t np = (db->dhi >> db->dsh) - (db->dlo >> db->dsh) + 1;
    MCHK(dalloc(&db->dir, np + 1));
    hipLaunchKernelGGL(db_dir_kernel, dim3(grid_for(np + 1)), dim3(256), 0, s, db->U, db->m, db->dlo, db->dsh, np,
                       db->dir);
    MCHK(hipGetLastError());
    // entries per template (kmer_db_template_stats): T sorted, a search per template
    if (db->nt) {
        MCHK(dalloc(&e1, db->entries));
        MCHK(dalloc(&e2, db->entries));
        MCHK(dalloc(&seg, (uint64_t)db->nt + 1));
        MCHK(hipMemcpyAsync(e1, db->T, db->entries * 4, hipMemcpyDeviceToDevice, s));
        rocprim::double_buffer<uint32_t> eb(e1, e2);
        MROC(tmp, rocprim::radix_sort_keys(t, b, eb, (size_t)db->entries, 0, std::max(1, bit_width64(db->nt)), s));
        hipLaunchKernelGGL(q_seg_kernel, dim3(grid_for((uint64_t)db->nt + 1)), dim3(256), 0, s, eb.current(),
                           db->entries, db->nt, seg);
        MCHK(hipGetLastError());
        std::vector<uint64_t> hseg((size_t)db->nt + 1);
        MCHK(hipMemcpyAsync(hseg.data(), seg, hseg.size() * 8, hipMemcpyDeviceToHost, s));
        MCHK(hipStreamSynchronize(s));
        for (uint32_t i = 0; i < db->nt; ++i) db->ulengths[i] = hseg[i + 1] - hseg[i];
    }
    MCHK(hipStreamSynchronize(s));
    return KMER_OK;
}

// kmer_db_open: the caller's strings uploaded and packed, template t owning [ts[t], ts[t + 1])
kmer_status build_db(kmer_db *db, const char *keys, uint64_t n, const uint64_t *ts) {
    hipStream_t s = db->s;
    uint8_t *dkeys = nullptr;
    uint64_t *c = nullptr, *dts = nullptr;
    uint32_t *t = nullptr, *bad = nullptr;
    auto cleanup = [&]() {
        for (void *p : {(void *)dkeys, (void *)c, (void *)dts, (void *)t, (void *)bad})
            if (p) (void)hipFree(p);
    };
    struct Guard {
        decltype(cleanup) &f;
        ~Guard() { f(); }
    } guard{cleanup};
    MCHK(dalloc(&dkeys, n * db->k));
    MCHK(dalloc(&c, n));
    MCHK(dalloc(&t, n));
    MCHK(dalloc(&dts, (uint64_t)db->nt + 1));
    MCHK(dalloc(&bad, 1));
    MCHK(hipMemsetAsync(bad, 0, 4, s));
    {
        // (the caller's arrays, read in place: waited for on every return path)
        struct SyncOnExit {
            hipStream_t s;
            ~SyncOnExit() { (void)hipStreamSynchronize(s); }
        } wait_uploads{s};
        MCHK(hipMemcpyAsync(dkeys, keys, n * db->k, hipMemcpyHostToDevice, s));
        MCHK(hipMemcpyAsync(dts, ts, ((uint64_t)db->nt + 1) * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(db_pack_kernel, dim3(grid_for(n)), dim3(256), 0, s, dkeys, n, db->k, c, bad);
        hipLaunchKernelGGL(db_tmpl_kernel, dim3(std::min<uint32_t>(std::max<uint32_t>(db->nt, 1), 65536)), dim3(256),
                           0, s, dts, db->nt, t);
        MCHK(hipGetLastError());
        uint32_t hbad = 0;
        MCHK(hipMemcpyAsync(&hbad, bad, 4, hipMemcpyDeviceToHost, s));
        MCHK(hipStreamSynchronize(s));
        if (hbad) return set_err(KMER_E_BAD_PARAM, "kmer_db_open: a template k-mer has a byte outside A/C/G/T");
    }
    return build_from_pairs(db, c, t, n);
}

// The arrays of a match build (every open): per query index and per template.
kmer_status match_alloc(kmer_match *m) {
    kmer_db *db = m->db;
    const uint64_t n = m->n;
    const uint32_t nt = db->nt;
    MatchBufs &b = m->b;
    MCHK(b.qidx.ensure(n));
    MCHK(b.present.ensure(n));
    MCHK(b.H.ensure(n));
    MCHK(b.seg.ensure((uint64_t)nt + 1));
    MCHK(b.u0.ensure(nt));
    MCHK(b.cu.ensure(nt));
    MCHK(b.t0.ensure(nt));
    MCHK(b.ct.ensure(nt));
    MCHK(b.order.ensure(nt));
    MCHK(b.rank.ensure(nt));
    MCHK(b.scal.ensure(2));
    MCHK(b.dw.ensure(1));
    if (!b.hw) MCHK(hipHostMalloc((void **)&b.hw, sizeof(kmer_winner), hipHostMallocDefault));
    MCHK(db->nhd.ensure(1));
    MCHK(db->fkey.ensure(nt));
    MCHK(db->fkey2.ensure(nt));
    MCHK(db->hc.ensure(n));
    m->qidx = b.qidx.p, m->present = b.present.p, m->H = b.H.p, m->seg = b.seg.p, m->u0 = b.u0.p;
    m->cu = b.cu.p, m->t0 = b.t0.p, m->ct = b.ct.p, m->order = b.order.p, m->rank = b.rank.p;
    m->scal = b.scal.p, m->dw = b.dw.p, m->hw = b.hw;
    return KMER_OK;
}

// Round 1 from the join's answers on (every open): qidx / present / cnt per
// query index and the hit counts db->hc, queued on the DB's stream -> their
// exclusive scan, the hits by template, the scores, the first-hit order.
kmer_status match_finish(kmer_match *m) {
    kmer_db *db = m->db;
    hipStream_t s = db->s;
    const uint64_t n = m->n;
    const uint32_t nt = db->nt;
    Temp &tmp = db->tmp;
    MatchBufs &b = m->b;
    uint32_t *nhd = db->nhd.p;
    uint64_t *fkey = db->fkey.p, *fkey2 = db->fkey2.p, *hc = db->hc.p;
    if (n) MROC(tmp, rocprim::exclusive_scan(t, b, hc, m->H, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), s));
    uint64_t tail[2] = {0, 0};
    if (n) MCHK(hipMemcpyAsync(&tail[0], m->H + n - 1, 8, hipMemcpyDeviceToHost, s));
    if (n) MCHK(hipMemcpyAsync(&tail[1], hc + n - 1, 8, hipMemcpyDeviceToHost, s));
    MCHK(hipStreamSynchronize(s));
    const uint64_t hits = tail[0] + tail[1];
    m->hits0 = hits;
    MCHK(hipMemcpyAsync(m->scal, &m->hits0, 8, hipMemcpyHostToDevice, s));
    MCHK(hipMemsetAsync(nhd, 0, 4, s));
    if (hits >= NONE) return set_err(KMER_E_BAD_PARAM, "kmer_match_open: more than 2^32 - 2 hits");
    MCHK(db->pt.ensure(hits));
    MCHK(db->pt2.ensure(hits));
    MCHK(db->pq2.ensure(hits));
    MCHK(b.sq.ensure(hits));
    m->sq = b.sq.p;
    if (hits) {
        hipLaunchKernelGGL(q_emit_kernel, dim3(grid_for(n)), dim3(256), 0, s, m->qidx, m->H, n, db->O, db->T,
                           db->pt.p, db->pq2.p);
        MCHK(hipGetLastError());
        rocprim::double_buffer<uint32_t> kb(db->pt.p, db->pt2.p);
        rocprim::double_buffer<uint32_t> vb(db->pq2.p, m->sq);
        MROC(tmp, rocprim::radix_sort_pairs(t, b, kb, vb, (size_t)hits, 0, std::max(1, bit_width64(nt)), s));
        if (vb.current() != m->sq) MCHK(hipMemcpyAsync(m->sq, vb.current(), hits * 4, hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(q_seg_kernel, dim3(grid_for((uint64_t)nt + 1)), dim3(256), 0, s, kb.current(), hits, nt,
                           m->seg);
    } else {
        MCHK(hipMemsetAsync(m->seg, 0, ((uint64_t)nt + 1) * 8, s));
    }
    hipLaunchKernelGGL(q_score_kernel, dim3(grid_for((uint64_t)nt * 64)), dim3(256), 0, s, m->seg, m->sq, m->cnt, nt,
                       m->u0, m->t0, m->cu, m->ct, fkey, nhd);
    MCHK(hipGetLastError());
    MROC(tmp, rocprim::radix_sort_keys(t, b, fkey, fkey2, (size_t)std::max<uint32_t>(nt, 1), 0, 64, s));
    MCHK(hipMemcpyAsync(&m->nh, nhd, 4, hipMemcpyDeviceToHost, s));
    MCHK(hipStreamSynchronize(s));
    hipLaunchKernelGGL(q_order_kernel, dim3(grid_for(std::max<uint32_t>(m->nh, 1))), dim3(256), 0, s, fkey2, m->nh,
                       m->order, m->rank);
    MCHK(hipGetLastError());
    MCHK(hipStreamSynchronize(s));
    return KMER_OK;
}

// the query's keys joined against U by binary search (host and device opens)
kmer_status match_build(kmer_match *m, const uint8_t *dkeys, const uint64_t *doffs, uint32_t klen) {
    kmer_db *db = m->db;
    const kmer_status st = match_alloc(m);
    if (st != KMER_OK) return st;
    // hit counts per query key
    hipLaunchKernelGGL(q_lookup_kernel, dim3(grid_for(m->n)), dim3(256), 0, db->s, dkeys, doffs, klen, m->n, db->k,
                       db->U, db->m, db->O, db->dir, db->dlo, db->dhi, db->dsh, m->qidx, db->hc.p, m->present);
    MCHK(hipGetLastError());
    return match_finish(m);
}

// the query is a finished table: every DB k-mer probed in it (kmer_probe.hip)
kmer_status match_build_table(kmer_match *m, kmerhip::TabProbe &a, const kmerhip::TabOwner &o) {
    kmer_db *db = m->db;
    hipStream_t s = db->s;
    const uint64_t n = m->n;
    kmer_status st = match_alloc(m);
    if (st != KMER_OK) return st;
    if (o.empty || o.k != db->k || n == 0) {         // no key of the DB is in the Map: no table memory touched
        if (n) MCHK(hipMemsetAsync(m->qidx, 0xFF, n * 4, s));
        if (n) MCHK(hipMemsetAsync(m->present, 0, n * 4, s));
        if (n) MCHK(hipMemsetAsync(db->hc.p, 0, n * 8, s));
        if (n) MCHK(hipMemsetAsync(m->cnt, 0, n * 8, s));
        return match_finish(m);
    }
    size_t bytes = 0;
    MCHK(kmerhip::bucket_sort_bytes(n, &bytes));
    MCHK(db->tmp.ensure(bytes + 16));
    MCHK(db->pb_bkt.ensure(n));
    MCHK(db->pb_bkt2.ensure(n));
    MCHK(db->pb_idx.ensure(n));
    MCHK(db->pb_idx2.ensure(n));
    a.U = db->U, a.O = db->O, a.m = n;
    a.bkt = db->pb_bkt.p, a.bkt2 = db->pb_bkt2.p, a.idx = db->pb_idx.p, a.idx2 = db->pb_idx2.p;
    a.tmp = db->tmp.p, a.tmp_bytes = bytes;
    a.qidx = m->qidx, a.hc = db->hc.p, a.present = m->present, a.cnt = m->cnt;
    MCHK(kmerhip::launch_tab_probe(a, o.n_cu, s));
    uint32_t e = 0, q = 0;                           // a refused bucket extent, as in the lookup
    MCHK(hipMemcpyAsync(&e, a.err, 4, hipMemcpyDeviceToHost, s));
    MCHK(hipMemcpyAsync(&q, a.badq, 4, hipMemcpyDeviceToHost, s));
    MCHK(hipStreamSynchronize(s));
    if (e & kmerhip::ERR_TAB_LOOKUP) {
        MCHK(hipMemsetD32Async((hipDeviceptr_t)a.err, (int)(e & ~kmerhip::ERR_TAB_LOOKUP), 1, s));
        MCHK(hipStreamSynchronize(s));
        return set_err(KMER_E_DEVICE,
                       "kmer_match_open_table: the extent of bucket " + std::to_string(q) + " lies past the table");
    }
    return match_finish(m);
}

kmer_status match_open_common(kmer_db *db, uint64_t n, kmer_match **out, kmer_match **mm) {
    if (!db || !out) return set_err(KMER_E_BAD_PARAM, "kmer_match_open: NULL argument");
    if (db->closing) return set_err(KMER_E_STATE, "kmer_match_open: the DB is closed");
    if (n >= NONE) return set_err(KMER_E_BAD_PARAM, "kmer_match_open: more than 2^32 - 2 query keys");
    *out = nullptr;
    MCHK(hipSetDevice(db->device));
    kmer_match *m = new kmer_match();
    m->db = db;
    m->n = n;
    ++db->live;
    if (db->has_spare) {                        // the last closed match's buffers
        m->b = db->spare;
        db->spare = MatchBufs();
        db->has_spare = false;
    }
    *mm = m;
    return KMER_OK;
}

}  // namespace

extern "C" {

kmer_status kmer_db_open(int32_t device, uint32_t k, const char *keys, uint64_t n_keys,
                         const uint64_t *template_start, uint32_t n_templates, kmer_db **out) {
    if (!out || (!keys && n_keys) || !template_start) return set_err(KMER_E_BAD_PARAM, "kmer_db_open: NULL argument");
    *out = nullptr;
    if (k == 0 || k > 32) return set_err(KMER_E_BAD_PARAM, "kmer_db_open: k must be 1..32");
    if (n_templates >= 0x7FFFFFFFu) return set_err(KMER_E_BAD_PARAM, "kmer_db_open: too many templates");
    if (template_start[0] != 0 || template_start[n_templates] != n_keys)
        return set_err(KMER_E_BAD_PARAM, "kmer_db_open: template_start must run from 0 to n_keys");
    for (uint32_t t = 0; t < n_templates; ++t)
        if (template_start[t + 1] < template_start[t])
            return set_err(KMER_E_BAD_PARAM, "kmer_db_open: template_start must not decrease");
    if (n_keys >= NONE) return set_err(KMER_E_BAD_PARAM, "kmer_db_open: more than 2^32 - 2 k-mers");
    MCHK(hipSetDevice(device));
    kmer_db *db = new kmer_db();
    db->device = device;
    db->k = k;
    db->nt = n_templates;
    hipError_t e = hipStreamCreateWithFlags(&db->s, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete db;
        MCHK(e);
    }
    db->lengths.resize(n_templates);
    for (uint32_t t = 0; t < n_templates; ++t) db->lengths[t] = template_start[t + 1] - template_start[t];
    db->name_off.assign((size_t)n_templates + 1, 0);
    const kmer_status st = n_keys ? build_db(db, keys, n_keys, template_start) : build_from_pairs(db, nullptr, nullptr, 0);
    if (st != KMER_OK) {
        free_db(db);
        return st;
    }
    *out = db;
    return KMER_OK;
}

}  // extern "C"

namespace {

// kmer_db_open_fasta*: the pairs gathered over the context (kmer_dbfasta.hip), then the shared build
kmer_status open_fasta(kmer_ctx *ctx, const uint8_t *bytes, size_t len, bool on_device, uint32_t flags, void *stream,
                       kmer_db **out) {
    if (out) *out = nullptr;
    if (!ctx || !out || (len && !bytes) || (flags & ~(uint32_t)KMER_DB_PIECE_TEST))
        return set_err(KMER_E_BAD_PARAM, "kmer_db_open_fasta: NULL argument or unknown flag");
    kmerhip::DbFastaPairs p;
    kmer_status st = (kmer_status)kmerhip::dbfasta_gather(ctx, bytes, len, on_device, flags, stream, &p);
    if (st != KMER_OK) return set_err(st, std::string("kmer_db_open_fasta: ") + kmer_last_error(ctx));
    struct Release {
        kmerhip::DbFastaPairs *p;
        ~Release() { kmerhip::dbfasta_release(p); }
    } release{&p};
    MCHK(hipSetDevice(p.device));
    kmer_db *db = new kmer_db();
    db->device = p.device;
    db->k = p.k;
    db->nt = p.nt;
    hipError_t e = hipStreamCreateWithFlags(&db->s, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete db;
        MCHK(e);
    }
    if (p.nt) {
        db->lengths.assign(p.lengths, p.lengths + p.nt);
        db->name_off.assign(p.name_off, p.name_off + p.nt + 1);
        db->names.assign(p.names, p.name_off[p.nt]);
    } else {
        db->name_off.assign(1, 0);
    }
    st = build_from_pairs(db, p.codes, p.tmpl, p.n);     // (the gather waited for the context's stream)
    if (st != KMER_OK) {
        free_db(db);
        return st;
    }
    *out = db;
    return KMER_OK;
}

}  // namespace

extern "C" {

kmer_status kmer_db_open_fasta_device(kmer_ctx *ctx, const void *d_bytes, size_t len, uint32_t flags, void *stream,
                                      kmer_db **out) {
    return open_fasta(ctx, (const uint8_t *)d_bytes, len, true, flags, stream, out);
}

kmer_status kmer_db_open_fasta(kmer_ctx *ctx, const uint8_t *bytes, size_t len, uint32_t flags, kmer_db **out) {
    return open_fasta(ctx, bytes, len, false, flags, nullptr, out);
}

kmer_status kmer_db_template_stats(kmer_db *db, uint32_t first, uint32_t n, uint64_t *lengths, uint64_t *ulengths) {
    if (!db || first > db->nt || n > db->nt - first)
        return set_err(KMER_E_BAD_PARAM, "kmer_db_template_stats: NULL db or a range past the DB's templates");
    for (uint32_t i = 0; i < n; ++i) {
        if (lengths) lengths[i] = db->lengths[first + i];
        if (ulengths) ulengths[i] = db->ulengths[first + i];
    }
    return KMER_OK;
}

kmer_status kmer_db_template_kmers(kmer_db *db, uint32_t tmpl, uint64_t cap, uint32_t *idx, uint64_t *n) {
    if (!db || !n || tmpl >= db->nt || (cap && !idx))
        return set_err(KMER_E_BAD_PARAM, "kmer_db_template_kmers: bad argument");
    const uint64_t ul = db->ulengths[tmpl];
    *n = ul;
    if (!ul || !cap) return KMER_OK;
    MCHK(hipSetDevice(db->device));
    hipStream_t s = db->s;
    // count + compact over the DB's distinct k-mers (ascending): those whose list holds the template
    uint32_t *d = nullptr;
    unsigned long long *dn = nullptr;
    auto body = [&]() -> kmer_status {
        MCHK(dalloc(&d, db->m));                     // (room for every candidate: the select writes what it finds)
        MCHK(dalloc(&dn, 1));
        rocprim::counting_iterator<uint32_t> iota(0);
        MROC(db->tmp, rocprim::select(t, b, iota, d, dn, (size_t)db->m, HasTemplate{db->O, db->T, tmpl}, s));
        unsigned long long got = 0;
        MCHK(hipMemcpyAsync(&got, dn, 8, hipMemcpyDeviceToHost, s));
        MCHK(hipStreamSynchronize(s));
        if (got != ul) return set_err(KMER_E_DEVICE, "kmer_db_template_kmers: the CSR and the template's entries differ");
        MCHK(hipMemcpyAsync(idx, d, std::min(cap, ul) * 4, hipMemcpyDeviceToHost, s));
        MCHK(hipStreamSynchronize(s));
        return KMER_OK;
    };
    const kmer_status st = body();
    if (d) (void)hipFree(d);
    if (dn) (void)hipFree(dn);
    return st;
}

kmer_status kmer_db_template_name(const kmer_db *db, uint32_t tmpl, const char **name, uint32_t *len) {
    if (!db || tmpl >= db->nt || !name || !len)
        return set_err(KMER_E_BAD_PARAM, "kmer_db_template_name: bad argument");
    *name = db->names.c_str() + db->name_off[tmpl];
    *len = (uint32_t)(db->name_off[tmpl + 1] - db->name_off[tmpl]);
    return KMER_OK;
}

kmer_status kmer_db_info(const kmer_db *db, uint32_t *k, uint32_t *n_templates, uint64_t *distinct,
                         uint64_t *entries) {
    if (!db) return set_err(KMER_E_BAD_PARAM, "kmer_db_info: NULL db");
    if (k) *k = db->k;
    if (n_templates) *n_templates = db->nt;
    if (distinct) *distinct = db->m;
    if (entries) *entries = db->entries;
    return KMER_OK;
}

kmer_status kmer_db_close(kmer_db *db) {
    if (db && db->live) {   // a match reads the DB's CSR and hands its buffers back at close:
        db->closing = true;  // the last kmer_match_close frees the DB
        return KMER_OK;
    }
    free_db(db);
    return KMER_OK;
}

kmer_status kmer_match_open(kmer_db *db, const char *keys, const uint64_t *offsets, const uint64_t *counts,
                            uint64_t n, kmer_match **out) {
    if (n && (!keys || !offsets || !counts)) return set_err(KMER_E_BAD_PARAM, "kmer_match_open: NULL argument");
    if (n && offsets[0] != 0) return set_err(KMER_E_BAD_PARAM, "kmer_match_open: offsets[0] must be 0");
    for (uint64_t i = 0; i < n; ++i)    // q_lookup_kernel packs keys + offsets[i] .. offsets[i + 1]
        if (offsets[i + 1] < offsets[i])
            return set_err(KMER_E_BAD_PARAM, "kmer_match_open: offsets must not decrease");
    kmer_match *m = nullptr;
    kmer_status st = match_open_common(db, n, out, &m);
    if (st != KMER_OK) return st;
    const uint64_t nbytes = n ? offsets[n] : 0;
    hipError_t e = db->qkeys.ensure(nbytes);
    if (e == hipSuccess) e = db->qoffs.ensure(n + 1);
    if (e == hipSuccess) e = m->b.cnt.ensure(n);
    m->cnt = m->b.cnt.p;
    if (e == hipSuccess && nbytes) e = hipMemcpyAsync(db->qkeys.p, keys, nbytes, hipMemcpyHostToDevice, db->s);
    if (e == hipSuccess && n) e = hipMemcpyAsync(db->qoffs.p, offsets, (n + 1) * 8, hipMemcpyHostToDevice, db->s);
    if (e == hipSuccess && n) e = hipMemcpyAsync(m->cnt, counts, n * 8, hipMemcpyHostToDevice, db->s);
    st = e == hipSuccess ? match_build(m, db->qkeys.p, db->qoffs.p, 0)
                         : set_err(KMER_E_DEVICE, std::string("HIP error: ") + hipGetErrorString(e));
    (void)hipStreamSynchronize(db->s);
    if (st != KMER_OK) {
        m->release();
        --m->db->live;
        delete m;
        return st;
    }
    *out = m;
    return KMER_OK;
}

kmer_status kmer_match_open_device(kmer_db *db, const void *d_keys, uint32_t klen, const void *d_counts, uint64_t n,
                                   void *stream, kmer_match **out) {
    if (n && (!d_keys || !d_counts || klen == 0))
        return set_err(KMER_E_BAD_PARAM, "kmer_match_open_device: NULL argument");
    kmer_match *m = nullptr;
    kmer_status st = match_open_common(db, n, out, &m);
    if (st != KMER_OK) return st;
    hipEvent_t ev = nullptr;
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(ev, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(db->s, ev, 0);
    if (e == hipSuccess) e = m->b.cnt.ensure(n);
    m->cnt = m->b.cnt.p;
    if (e == hipSuccess && n) e = hipMemcpyAsync(m->cnt, d_counts, n * 8, hipMemcpyDeviceToDevice, db->s);
    st = e == hipSuccess ? match_build(m, (const uint8_t *)d_keys, nullptr, klen)
                         : set_err(KMER_E_DEVICE, std::string("HIP error: ") + hipGetErrorString(e));
    if (ev) (void)hipEventDestroy(ev);
    if (st != KMER_OK) {
        m->release();
        --m->db->live;
        delete m;
        return st;
    }
    *out = m;
    return KMER_OK;
}

kmer_status kmer_match_open_table(kmer_db *db, kmer_ctx *ctx, kmer_match **out) {
    if (!db || !ctx || !out) return set_err(KMER_E_BAD_PARAM, "kmer_match_open_table: NULL argument");
    *out = nullptr;
    kmerhip::TabProbe a;
    memset(&a, 0, sizeof(a));
    kmerhip::TabOwner o;
    memset(&o, 0, sizeof(o));
    kmer_status st = (kmer_status)kmerhip::table_view(ctx, &a, &o);   // (settles an in-flight chunk)
    if (st != KMER_OK) return set_err(st, std::string("kmer_match_open_table: ") + kmer_last_error(ctx));
    if (o.device != db->device)
        return set_err(KMER_E_BAD_PARAM, "kmer_match_open_table: the context and the DB are on different devices");
    kmer_match *m = nullptr;
    st = match_open_common(db, db->m, out, &m);
    if (st != KMER_OK) return st;
    // the table's writers are queued on the context's stream
    hipEvent_t ev = nullptr;
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(ev, o.stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(db->s, ev, 0);
    if (e == hipSuccess) e = m->b.cnt.ensure(m->n);
    m->cnt = m->b.cnt.p;
    st = e == hipSuccess ? match_build_table(m, a, o)
                         : set_err(KMER_E_DEVICE, std::string("HIP error: ") + hipGetErrorString(e));
    (void)hipStreamSynchronize(db->s);               // the table is not read after the call
    if (ev) (void)hipEventDestroy(ev);
    if (st != KMER_OK) {
        m->release();
        --m->db->live;
        delete m;
        return st;
    }
    *out = m;
    return KMER_OK;
}

kmer_status kmer_db_kmers(const kmer_db *db, uint64_t first, uint64_t n, char *keys) {
    if (!db || first > db->m || n > db->m - first || (n && !keys))
        return set_err(KMER_E_BAD_PARAM, "kmer_db_kmers: NULL argument or a range past the DB's distinct k-mers");
    if (n == 0) return KMER_OK;
    MCHK(hipSetDevice(db->device));
    uint8_t *d = nullptr;
    MCHK(dalloc(&d, n * db->k));
    hipLaunchKernelGGL(db_decode_kernel, dim3(grid_for(n)), dim3(256), 0, db->s, db->U, first, n, db->k, d);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(keys, d, n * db->k, hipMemcpyDeviceToHost, db->s);
    if (e == hipSuccess) e = hipStreamSynchronize(db->s);
    (void)hipFree(d);
    MCHK(e);
    return KMER_OK;
}

kmer_status kmer_match_info(kmer_match *m, uint64_t *hits, uint32_t *n_templates) {
    if (!m) return set_err(KMER_E_BAD_PARAM, "kmer_match_info: NULL match");
    MCHK(hipSetDevice(m->db->device));
    kmer_winner w;
    kmer_status st = kmer_match_winner(m, &w);
    if (st != KMER_OK) return st;
    if (hits) *hits = w.hits;
    if (n_templates) {
        uint32_t n = 0;
        st = kmer_match_templates(m, KMER_ORDER_DB, 0, nullptr, nullptr, nullptr, &n);
        if (st != KMER_OK) return st;
        *n_templates = n;
    }
    return KMER_OK;
}

kmer_status kmer_match_templates(kmer_match *m, uint32_t order, uint32_t cap, uint32_t *tmpl, uint64_t *uscore,
                                 uint64_t *tscore, uint32_t *n) {
    if (!m || !n || (cap && (!tmpl || !uscore || !tscore)) || order > KMER_ORDER_DB)
        return set_err(KMER_E_BAD_PARAM, "kmer_match_templates: bad argument");
    MCHK(hipSetDevice(m->db->device));
    const uint32_t nt = m->db->nt, nh = m->nh;
    std::vector<uint32_t> ord(nh), cu(nt);
    std::vector<uint64_t> ct(nt);
    hipStream_t s = m->db->s;
    if (nh) MCHK(hipMemcpyAsync(ord.data(), m->order, nh * 4ull, hipMemcpyDeviceToHost, s));
    if (nt) MCHK(hipMemcpyAsync(cu.data(), m->cu, nt * 4ull, hipMemcpyDeviceToHost, s));
    if (nt) MCHK(hipMemcpyAsync(ct.data(), m->ct, nt * 8ull, hipMemcpyDeviceToHost, s));
    MCHK(hipStreamSynchronize(s));
    uint32_t c = 0;
    auto put = [&](uint32_t t) {
        if (!cu[t]) return;
        if (c < cap) {
            tmpl[c] = t;
            uscore[c] = cu[t];
            tscore[c] = ct[t];
        }
        ++c;
    };
    if (order == KMER_ORDER_FIRST_HIT) {
        for (uint32_t r = 0; r < nh; ++r) put(ord[r]);
    } else {
        for (uint32_t t = 0; t < nt; ++t) put(t);
    }
    *n = c;
    return KMER_OK;
}

kmer_status kmer_match_template_kmers(kmer_match *m, uint32_t tmpl, uint64_t cap, uint32_t *qidx, uint64_t *n) {
    if (!m || !n || tmpl >= m->db->nt || (cap && !qidx))
        return set_err(KMER_E_BAD_PARAM, "kmer_match_template_kmers: bad argument");
    MCHK(hipSetDevice(m->db->device));
    hipStream_t s = m->db->s;
    uint64_t ab[2];
    MCHK(hipMemcpyAsync(ab, m->seg + tmpl, 16, hipMemcpyDeviceToHost, s));
    MCHK(hipStreamSynchronize(s));
    const uint64_t len = ab[1] - ab[0];
    if (cap && len) {
        MCHK(hipMemcpyAsync(qidx, m->sq + ab[0], std::min(cap, len) * 4, hipMemcpyDeviceToHost, s));
        MCHK(hipStreamSynchronize(s));
    }
    *n = len;
    return KMER_OK;
}

kmer_status kmer_match_winner(kmer_match *m, kmer_winner *w) {
    if (!m || !w) return set_err(KMER_E_BAD_PARAM, "kmer_match_winner: NULL argument");
    MCHK(hipSetDevice(m->db->device));
    hipStream_t s = m->db->s;
    hipLaunchKernelGGL(winner_kernel, dim3(1), dim3(1024), 0, s, m->order, m->nh, m->cu, m->ct, m->u0, m->t0,
                       m->scal, m->dw);
    MCHK(hipGetLastError());
    MCHK(hipMemcpyAsync(m->hw, m->dw, sizeof(kmer_winner), hipMemcpyDeviceToHost, s));
    MCHK(hipStreamSynchronize(s));
    *w = *m->hw;
    return KMER_OK;
}

kmer_status kmer_match_remove(kmer_match *m, uint32_t tmpl, uint64_t *hits) {
    if (!m || tmpl >= m->db->nt) return set_err(KMER_E_BAD_PARAM, "kmer_match_remove: bad template");
    MCHK(hipSetDevice(m->db->device));
    hipStream_t s = m->db->s;
    uint64_t ab[2];
    MCHK(hipMemcpyAsync(ab, m->seg + tmpl, 16, hipMemcpyDeviceToHost, s));
    MCHK(hipStreamSynchronize(s));
    const uint64_t len = ab[1] - ab[0];
    if (len) {
        hipLaunchKernelGGL(remove_kernel, dim3(grid_for(len)), dim3(256), 0, s, m->seg, m->sq, tmpl, m->present,
                           m->qidx, m->db->O, m->db->T, m->cnt, m->cu, m->ct, m->scal);
        MCHK(hipGetLastError());
    }
    uint64_t h = 0;
    MCHK(hipMemcpyAsync(&h, m->scal, 8, hipMemcpyDeviceToHost, s));
    MCHK(hipStreamSynchronize(s));
    if (hits) *hits = h;
    return KMER_OK;
}

kmer_status kmer_match_removed(kmer_match *m, uint8_t *flags) {
    if (!m || (m->n && !flags)) return set_err(KMER_E_BAD_PARAM, "kmer_match_removed: NULL argument");
    if (!m->n) return KMER_OK;
    MCHK(hipSetDevice(m->db->device));
    hipStream_t s = m->db->s;
    uint8_t *d = nullptr;
    MCHK(dalloc(&d, m->n));
    hipLaunchKernelGGL(removed_kernel, dim3(grid_for(m->n)), dim3(256), 0, s, m->qidx, m->present, m->n, d);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(flags, d, m->n, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d);
    MCHK(e);
    return KMER_OK;
}

kmer_status kmer_match_close(kmer_match *m) {
    if (!m) return KMER_OK;
    (void)hipSetDevice(m->db->device);
    (void)hipStreamSynchronize(m->db->s);
    kmer_db *db = m->db;
    m->release();
    delete m;
    if (--db->live == 0 && db->closing) free_db(db);
    return KMER_OK;
}

const char *kmer_match_last_error(void) { return g_err.c_str(); }

}  // extern "C"
