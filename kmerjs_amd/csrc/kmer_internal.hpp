// kmer_internal.hpp — shared definitions between the gfx950 kernels (the
// kmer_*.hip kernel files; their common device helpers are in kmer_device.hpp)
// and the host orchestration (kmer_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kmerhip {

// The library reads no environment variable.

// ---- tile geometry (tile kernel) -------------------------------------------
// One workgroup owns one 16 KiB tile of the input.  The tile plus a front halo
// (rc windows whose start lies in the previous tile) and a back halo (forward
// windows that run into the next tile) is staged in LDS.
constexpr int TPB = 256;                 // threads per workgroup (4 waves)
constexpr int BPT = 64;                  // bytes scanned per thread
constexpr int TILE = TPB * BPT;          // 16384
constexpr int FH = 64;                   // front halo bytes
constexpr int BH = 80;                   // back halo bytes (>= KMAX_TILE - 1 + 3, x16)
constexpr int KMAX_PACKED = 32;          // longest k of a 2-bit packed (u64) key
constexpr int KMAX_TILE = 64;            // longest k handled by the tile kernel
constexpr int KMAX_DENSE = 32;           // longest k packed into 2-bit codes
constexpr uint32_t MAXREL = (1u << 23) - 1;  // longest sequence line (bytes - 1), default order-key layout
// Order key = line << (pbits + 1) | strand << pbits | position field (pbits
// bits).  Default 23 (lines up to 8 MiB, 2^40 lines); long-line mode 40
// (lines up to 1 TiB, 2^23 lines) -- KMER_FLAG_LONG_LINES, or the automatic
// retry of kmer_count_file / kmer_count_buffer.
constexpr uint32_t PBITS_DEFAULT = 23, PBITS_LONG = 40;
// newline positions kept per 16 KiB tile by the one-pass line split (lines of
// >= 16 bytes on average; denser tiles take the two-pass route)
constexpr uint32_t NL_SLOTS = 1024;

// error bits (device-side, OR-ed into ctx->d_err)
enum : uint32_t {
    ERR_NONASCII = 1u << 0,
    ERR_LINE_TOO_LONG = 1u << 1,
    ERR_LOOKBACK_TIMEOUT = 1u << 2,
    ERR_REC_OVERFLOW = 1u << 3,
    ERR_LINE_OVERFLOW = 1u << 4,
    ERR_OVF_OVERFLOW = 1u << 5,
    ERR_CROSS_OVERFLOW = 1u << 6,
    ERR_COUNT_OVERFLOW = 1u << 7,    // table mode: one key counted 2^32 times in one bucket
    ERR_BIG_OVERFLOW = 1u << 8,      // table mode: big-count list full
    ERR_TAB_SPLIT = 1u << 9,         // table mode: bucket range could not be split further
    ERR_DENSE_RANK = 1u << 10,       // dense-hit path: a rank slot past the counted hits (count / write disagree)
    ERR_TAB_CAP = 1u << 11,          // table mode: a bucket past its fixed pass-2 capacity (counted route redoes it)
    ERR_BKT_CAP = 1u << 12,          // bucket finish: a run past its bucket's fixed region (counted route redoes it)
    ERR_BKT_RANK = 1u << 13,         // bucket finish: a partitioned rank past the hits (a defect)
    ERR_TAB_LOOKUP = 1u << 14,       // table lookup: a bucket extent past the table (not read; a defect)
    ERR_TAB_EXTRACT = 1u << 15,      // table extract: a slot past the counted keys (not written; a defect)
    // not an error: a tile without '\n' had hits, or a tile overflowed its hit
    // slots -- cross segments may be long (finish sorts the whole cross list)
    INFO_LONGSEG = 1u << 16,
};
// With any of these in the error word at the chunk tail a chunk's cross
// entries wait for the host (finish sorts the whole list, or the chunk is
// redone); without, the device places them right behind the chunk
// (cross_segsort_chunk_kernel).
constexpr uint32_t CROSS_HOST_BITS = INFO_LONGSEG | ERR_OVF_OVERFLOW | ERR_REC_OVERFLOW | ERR_CROSS_OVERFLOW;

// look-back word: [63:62] status, [61:0] value
constexpr uint64_t LB_AGG = 1ull << 62;
constexpr uint64_t LB_INC = 2ull << 62;
constexpr uint64_t LB_VAL = (1ull << 62) - 1;

// Running position of the stream, kept in device memory so consecutive
// launches chain without host round trips.
struct StreamPos {
    uint64_t lines;        // newlines consumed before the next chunk (= its first line index)
    uint64_t unused;
    uint64_t ends_open;    // 1 if the last chunk did not end with '\n'
    uint64_t pad;
};

// A window that cannot take the dense path (non-ACGT byte, long key, or a
// non-dense configuration).  Its key bytes are gathered later:
// key = strand ? rc(data[pos, pos+len)) : data[pos, pos+len)   (pos is chunk-relative)
struct Record {
    uint64_t order;
    uint64_t pos;
    uint32_t len;
    uint32_t strand;
};

// A sequence line for the general (any k / any step) kernel.
struct SeqLine {
    uint64_t start;        // chunk-relative byte offset
    uint64_t len;
    uint64_t line_index;   // global line index
};

// A verified prefix hit from the tile scan with its tile-local line context.
struct HitRec {
    uint64_t code;         // 2-bit codes of the k-byte forward window (its last 32 bases when k > 32;
                           // the first k - 32 are in ScanArgs::hits_hi / ovf_hi at the same index)
    uint32_t tile;
    uint32_t qm;           // [13:0] pattern position q, [14] strand, [15] exotic, [16] line start in tile,
                           // [31:17] ordinal of the hit in its tile
    uint32_t c_local;      // '\n' count in the tile before the window start
    uint32_t lstart;       // tile-relative line start (when [16] is set)
};
constexpr int HMAX = 64;   // hit slots per tile (more go to the overflow list)

// Tile-local line context of the tile position base + qrel (qrel 0..63) from
// what the thread that scanned the 64 bytes at `base` knows: mask = its '\n'
// bytes (bit i: byte base + i), pre = the tile's '\n' count before base,
// prevnl = the tile position of the last '\n' before base (-1: none).
// *c_local = '\n' count of the tile before the position, *lstart = one past
// the last '\n' before it (-1: none in this tile).  A window that becomes a hit
// record holds no '\n' and holds the position, so this is the context of the
// window's start as well (HitRec::c_local / lstart).
__host__ __device__ inline void region_line_context(uint32_t pre, int32_t prevnl, uint64_t mask, uint32_t qrel,
                                                    int32_t base, uint32_t *c_local, int32_t *lstart) {
    const uint64_t below = mask & ((1ull << qrel) - 1ull);
    const uint32_t lo = (uint32_t)below, hi = (uint32_t)(below >> 32);
    *c_local = pre + (uint32_t)__builtin_popcount(lo) + (uint32_t)__builtin_popcount(hi);
    const int32_t own = hi ? 64 - __builtin_clz(hi) : 32 - __builtin_clz(lo | 1u);   // (below != 0: top bit + 1)
    const int32_t ls = below ? base + own : prevnl + 1;
    *lstart = ls > 0 ? ls : -1;
}

// Per-tile aggregates of the scan kernel, scanned (exclusive) across tiles
// with TileSumOp: lines before the tile, start of the line open at the tile
// start, hits before the tile.
struct TileSum {
    uint64_t cnt;                  // real '\n' count
    uint32_t nh;                   // prefix hits (stored + overflow)
    uint32_t nx;                   // ... of which cross hits (line crosses a tile edge; all if overflowed)
    uint64_t lnl;                  // absolute start of the line after its last '\n' (0 = none; scan: max)
};

__host__ __device__ inline TileSum tile_sum_op(const TileSum &x, const TileSum &y) {
    TileSum r;
    r.cnt = x.cnt + y.cnt;
    r.nh = x.nh + y.nh;
    r.nx = x.nx + y.nx;
    r.lnl = x.lnl > y.lnl ? x.lnl : y.lnl;
    return r;
}
constexpr uint32_t TSCAN_BLOCK = 1024;     // tiles per block of the tile scan
constexpr uint32_t TSCAN_INLINE_MAX = 2048; // block-sum prefixes computed in-kernel up to this many blocks

struct ScanArgs {
    const uint8_t *data;
    uint64_t len;
    uint64_t abs_offset;
    uint32_t n_tiles, k, plen;
    uint32_t p4, r4, pmask;
    const uint8_t *PR;
    TileSum *tsum;                 // per tile
    HitRec *hits;                  // n_tiles * HMAX slots
    HitRec *ovf;
    unsigned long long *ovf_count;
    uint64_t ovf_cap;
    unsigned int *err;
    uint64_t *hits_hi, *ovf_hi;    // k > 32: code of the window's first k - 32 bases, per hit slot
};

// Bit-plane prefix test (ACGT prefixes): per prefix base i, xor masks that
// turn the plane bits into "code bit equals P_i's bit" (~0 where P_i's bit is 0).
struct PlaneArgs {
    uint32_t kl[5], kh[5];         // P (forward strand)
    uint32_t rl[5], rh[5];         // rc(P), as a forward-strand string
    uint32_t pb;                   // bases tested on the planes: min(|P|, 5); the rest byte-exact
};

// value of a unique packed key: first-occurrence order and count
struct Agg {
    uint64_t first;
    uint64_t count;
};

// Hit resolution.  Packed mode places every hit of the session at its RANK
// (position in first-occurrence order of all hits): a hit whose line lies
// inside one tile gets hits-before-tile + its rank among the tile's hits;
// hits of lines that cross a tile edge (or of overflowed tiles) go to the
// cross list with their natural slot and are placed by a sort at finish.
struct HitArgs {
    const HitRec *hits;
    const TileSum *tsum;
    const TileSum *tscan;          // exclusive scan of tsum (cnt: sum, lnl: max from abs_offset, nh: sum)
    const HitRec *ovf;
    const unsigned long long *ovf_count;
    uint64_t ovf_cap;
    uint32_t n_tiles, k, plen;
    uint64_t abs_offset;
    const StreamPos *pos;
    uint32_t packed;               // ACGT windows are ranked packed keys
    uint32_t pbits;                // order-key position bits (PBITS_*)
    uint64_t smask;                // suffix mask: 2*(k - |P|) bits (its low 64 when wide)
    uint64_t invalid_key;          // 2^(2*(k-|P|)): sorts after every real key (wide: in rkeyh)
    // k > 32: 128-bit window codes (hits_hi / ovf_hi); wide (2(k - |P|) >= 64):
    // keys of two words, the high one in rkeyh (cross list: xkeyh, and xkey
    // holds the entry's own index until apply_cross has moved it)
    const uint64_t *hits_hi, *ovf_hi;
    uint32_t wide;
    uint64_t smask_hi;             // wide: mask of the high word (2(k - |P|) - 64 bits)
    uint64_t *rkeyh;
    uint64_t *xkeyh, *xkeyl;
    uint64_t out_base;             // session hits before this chunk
    uint64_t rcap;                 // capacity of the rank arrays (a slot past it: the chunk overflowed and is redone)
    uint64_t *rkey;                // by rank: suffix code (invalid_key: filtered / record)
    uint32_t *rkey32;              // ... as u32 when 2(k-|P|) + 1 <= 32 (then rkey is unused)
    uint64_t *rord;                // by rank: first-occurrence order key
    uint64_t *xord, *xkey;         // cross list in natural-slot order (order, key, natural slot)
    uint32_t *xslot;
    uint64_t xbase, xcap;          // session cross entries before this chunk, capacity
    Record *recs;
    unsigned long long *rec_count;
    uint64_t rec_cap;
    unsigned int *err;
    // chunk tail (hit_overflow_kernel's last block): stream position update and
    // the chunk's counters published to host memory
    const uint8_t *data;
    uint64_t len;
    uint64_t *scal;                // device scalars [0..7] (see kmer_ctx::d_scal)
    unsigned int *ticket;          // last-block ticket (returned to 0 by the last block)
    unsigned long long *chunk_hits, *chunk_cross, *ends_open;
    unsigned int *cross_go;        // 1: the error word at the tail has none of CROSS_HOST_BITS
    uint64_t *host_out;            // mapped host memory: copy of scal[0..7], then [9] = seq
    uint64_t seq;                  // chunk sequence number (the host waits for it in host_out[9])
    uint64_t *stamp;               // device clock stamps (STAMP_*): the tail writes FEED_END and copies
                                   // [SCAN_START .. FEED_END] to host_out[TAIL_STAMP ..]; or null
};

// Device clock stamps (wall_clock64, a constant-rate counter) of the packed
// path's phases: written by lane 0 of workgroup 0 of the kernels that delimit
// them, so that no timing event sits between the launches of a step.
enum : uint32_t { STAMP_SCAN_START = 0, STAMP_SCAN_END = 1, STAMP_FEED_END = 2, STAMP_FINISH_START = 3, STAMP_WORDS = 4 };
// the mapped host words (kmer_ctx::h_tail): [0..7] device scalars, [8] unique
// keys, [9] chunk sequence, [10] error word at the emit, [11..13] the chunk's
// stamps, [14] finish start, [15] finish end
enum : uint32_t { TAIL_NUNIQ = 8, TAIL_SEQ = 9, TAIL_ERR = 10, TAIL_STAMP = 11, TAIL_FIN_START = 14, TAIL_FIN_END = 15,
                  TAIL_WORDS = 16 };
__device__ __forceinline__ void stamp_now(uint64_t *stamp, uint32_t which) {
    if (stamp && blockIdx.x == 0 && threadIdx.x == 0) stamp[which] = wall_clock64();
}

// By rank, after the key sort: the key and its total count if this rank is
// the key's first occurrence, count 0 otherwise.
struct HeadRec {
    uint64_t key;
    uint64_t count;
};

// Ordered output from the rank arrays after the key sort.
struct EmitArgs {
    const uint32_t *hcnt;          // by rank: the key's count at its first occurrence, else 0
    const uint8_t *hmark;          // bucket routes: min(that count, 255) by rank, hcnt valid only where it is 255; or null
    const HeadRec *hrec;           // merged finish (summed counts): by rank, key and u64 count of heads; else null
    const uint32_t *rkey32;        // hrec == null: key by rank (narrow keys) ...
    const uint64_t *rkey64;        // ... or (wider keys)
    const uint64_t *rkeyh;         // ... with, for keys of >= 64 bits, their high words
    const uint32_t *ecnt;          // heads per EMIT_RPB ranks (head_count_kernel)
    const uint64_t *epre;          // ... their exclusive scan, or null: each workgroup sums the earlier counts
    const uint64_t *rord;          // by rank: order key
    uint64_t n;
    uint64_t invalid_key;
    uint64_t *nuniq;
    uint64_t *nuniq_host;          // mapped host copy of *nuniq (or null)
    uint64_t *host_out;            // mapped host words (TAIL_*): error word, finish stamps (or null)
    const unsigned int *err;       // ... the device error word copied there
    const uint64_t *stamp;         // ... the device stamps (STAMP_FINISH_START), or null
    uint32_t k, plen, partial;
    uint8_t P[KMAX_TILE];          // the prefix (|P| <= k <= 64 on the packed paths)
    uint8_t *keys_out;             // decode: n * k bytes
    uint64_t *cnt_out, *first_out;
    uint64_t *ukey;                // partial: suffix codes
    Agg *uval;                     // partial: {first, count}
};

struct TileArgs {
    const uint8_t *data;
    uint64_t len;
    uint32_t n_tiles;
    uint32_t k;
    uint32_t plen;
    uint32_t p4, r4, pmask;        // first min(4,|P|) bytes of P and rc(P) (little-endian), byte mask
    uint32_t dense;                // 1: ACGT windows go to the dense table
    uint32_t dense_update;         // 0: skip dense atomics (record-overflow redo of a chunk)
    uint64_t abs_offset;           // absolute byte offset of data[0] in the whole input
    uint32_t emit_lines;           // 1: emit sequence-line descriptors instead of windows
    const uint8_t *PR;             // device: P[0..KMAX_TILE) then rc(P)[0..KMAX_TILE)
    // dense table
    unsigned long long *counts;
    unsigned long long *first;
    // records
    Record *recs;
    unsigned long long *rec_count;
    uint64_t rec_cap;
    // line list
    SeqLine *lines_out;
    unsigned long long *line_count;
    uint64_t line_cap;
    // look-back / positions
    unsigned long long *lb_cnt;
    unsigned long long *lb_lnl;
    unsigned int *ticket;
    StreamPos *pos;
    const uint64_t *tp_cnt;        // two-pass mode: exclusive newline count per tile (absolute line index)
    const uint64_t *tp_lnl;        // two-pass mode: line start before tile (absolute)
    unsigned int *err;
};

// General path with the device merge (step 1): sequence lines from
// chunk_lines, their windows flattened (wbase: exclusive scan of 2W per line)
struct GenWinArgs {
    const uint8_t *data;
    uint64_t len;
    const SeqLine *lines;
    const uint64_t *wbase;
    const uint64_t *tbase;         // newlines before each TILE of the chunk (chunk_lines)
    uint64_t first;                // line index (from the chunk start) of the first sequence line
    uint64_t n_lines, total;       // lines, windows of both strands
    uint32_t k, plen, pbits;
    const uint8_t *P, *RP;         // the prefix and its reverse complement (device)
    Record *recs;
    unsigned long long *rec_count;
    uint64_t rec_cap;
    unsigned int *err;
};
hipError_t launch_gen_windows(const GenWinArgs &a, hipStream_t s);
hipError_t launch_gen_cand(const GenWinArgs &a, const PlaneArgs &pa, hipStream_t s);   // A/C/G/T prefix
hipError_t launch_gen_fix(const Record *cand, uint64_t n, const SeqLine *lines, uint32_t k, uint32_t plen,
                          uint32_t pbits, Record *recs, unsigned long long *rec_count, uint64_t rec_cap,
                          unsigned int *err, hipStream_t s);

struct WindowArgs {
    const uint8_t *data;
    const SeqLine *lines;
    const unsigned long long *n_lines;
    uint32_t k, step, plen;
    uint32_t pbits;                // order-key position bits (PBITS_*)
    const uint8_t *P;              // device copy of the prefix
    Record *recs;
    unsigned long long *rec_count;
    uint64_t rec_cap;
    unsigned int *err;
};

// Dense-hit path (empty or 1-2 base ACGT prefix, step 1, k <= 32): every
// window of every sequence line gets a rank slot -- its position in the
// first-occurrence order: line base (scan of 2W per sequence line) + s for
// the forward window at s, + W + (W-1-s) for the reverse strand's.
struct WinArgs {
    const uint8_t *data;
    uint64_t len;
    const SeqLine *lines;          // by sequence ordinal (len 0: no windows)
    uint64_t n_lines;
    uint64_t li0;                  // line index of the chunk's first line
    const uint64_t *wbase;         // by sequence ordinal: rank of the line's first window (chunk-relative)
    uint32_t k, plen;
    uint32_t pbits;                // order-key position bits (PBITS_*)
    uint32_t step;                 // windows at 0, step, 2 step, ... of the line and of its complement
    unsigned long long *empty;     // step > 1, no prefix: [0] empty keys "" counted, [1] min order key of one
    const uint8_t *P;              // device copy of the prefix (cut-short windows of step > 1)
    uint64_t pcode, rcode;         // P and rc(P) as 2-bit codes (first base most significant)
    uint64_t smask, invalid_key;
    uint64_t out_base;
    uint32_t block_lines;          // lines of many windows (contigs): a workgroup per line, else a wave
    uint64_t *rkey;
    uint32_t *rkey32;
    uint64_t *rord;
    Record *recs;
    unsigned long long *rec_count;
    uint64_t rec_cap;
    unsigned int *err;
};

// dense-hit path, step 1, k <= 64 (kmer_dense.hip): only accepted windows,
// ranked by two passes over the lines
struct DenseArgs {
    const uint8_t *data;
    uint64_t len;
    const SeqLine *lines;          // by sequence ordinal (len 0: no windows)
    uint64_t n_lines;
    uint64_t lpw;                  // lines per wave
    uint32_t k, plen;
    uint32_t pbits;                // order-key position bits (PBITS_*)
    uint64_t pcode;                // P as 2-bit codes (first base most significant)
    uint64_t smask, smask_hi;      // the key: the low 2 (k - |P|) bits of the window code (hi: above bit 64)
    uint64_t *cnt;                 // count pass: per line accepted forward | reverse << 32
    uint32_t *tot;                 // count pass: per line forward + reverse
    const uint64_t *hbase;         // write pass: per line first slot (chunk-relative, exclusive scan of tot)
    uint64_t out_base;
    uint64_t out_end;              // write pass: out_base + the counted hits (slots past it are refused)
    unsigned long long *dbg;       // write pass: the first refused slot's context (8 words, [0] = taken)
    uint32_t *rkey32;              // narrow keys (2 (k - |P|) <= 31 bits), else rkey
    uint64_t *rkey;
    uint64_t *rkeyh;               // wide keys (2 (k - |P|) >= 64 bits): the bits above 64
    uint64_t *rord;
    const uint8_t *P, *RP;         // device: P and rc(P) (exotic windows' prefix bytes)
    Record *recs;
    unsigned long long *rec_count;
    uint64_t rec_cap;
    unsigned int *err;
};
hipError_t launch_dense_windows(const DenseArgs &a, bool write, hipStream_t s);

// ---- launchers (kmer_kernels.hip) ------------------------------------------
hipError_t launch_lines(const TileArgs &a, bool lookback, hipStream_t s);
hipError_t launch_scan_tiles(const ScanArgs &a, hipStream_t s);
hipError_t launch_scan_planes(const ScanArgs &a, const PlaneArgs &pa, hipStream_t s);
hipError_t launch_hits(const HitArgs &a, hipStream_t s);
// exclusive scan of the per-tile sums (init folded in); bsum / bscan: n_blocks scratch
hipError_t launch_tile_reduce(const TileSum *in, uint32_t n, TileSum *bsum, uint64_t *stamp, hipStream_t s);
hipError_t launch_tile_scan(const TileSum *in, uint32_t n, const TileSum *bsum, bool bsum_scanned, TileSum init,
                            TileSum *out, hipStream_t s);
enum : uint32_t { PREP_RESET = 1, PREP_SETPOS = 2, PREP_SAVE = 4, PREP_ZERO = 8 };
hipError_t launch_prep(StreamPos *pos, StreamPos *saved, unsigned int *err, uint64_t *scal, uint32_t flags,
                       uint64_t lines, uint64_t *stamp, hipStream_t s);
hipError_t launch_tile_aggregate(const uint8_t *data, uint64_t len, uint32_t n_tiles, uint64_t *agg_cnt,
                                 uint64_t *agg_lnl, unsigned int *err, hipStream_t s);
hipError_t launch_windows(const WindowArgs &a, uint32_t grid, hipStream_t s);
// rkey32 != NULL: keys are written as u32 (narrow mode), else to rkey
hipError_t launch_cross_scatter(const uint32_t *slot, const uint64_t *ord, const uint64_t *key, uint64_t n,
                                uint64_t *rkey, uint32_t *rkey32, uint64_t *rord, hipStream_t s);
hipError_t launch_cross_sort_small(const uint32_t *slot, const uint64_t *ord, const uint64_t *key, uint64_t n,
                                   uint64_t *rkey, uint32_t *rkey32, uint64_t *rord, hipStream_t s);
constexpr uint64_t XSMALL_MAX = 16384;   // cross lists up to this size: one-workgroup sort
hipError_t launch_cross_segsort(uint64_t *ord, uint64_t *key, const uint32_t *slot, uint64_t n, uint64_t *rkey,
                                uint32_t *rkey32, uint64_t *rord, uint32_t pbits, uint64_t *stamp, hipStream_t s);
// the chunk's cross entries [xbase, xbase + *count), placed on the device if the chunk tail set *go
hipError_t launch_cross_segsort_chunk(uint64_t *ord, uint64_t *key, const uint32_t *slot, uint64_t xbase, uint64_t xcap,
                                      const unsigned long long *count, const unsigned int *go, uint64_t *rkey,
                                      uint32_t *rkey32, uint64_t *rord, uint32_t pbits, hipStream_t s);
hipError_t launch_heads(const uint64_t *skey, const uint32_t *srank, uint64_t n, uint64_t invalid_key,
                        const uint64_t *rcnt, HeadRec *hrec, uint32_t *hcnt, hipStream_t s);
// sort finish without per-entry counts: hcnt prefilled with 1, only groups of >= 2 and invalid keys written
hipError_t launch_heads_sparse(const uint64_t *skey64, const uint32_t *skey32, const uint32_t *srank, uint64_t n,
                               uint64_t invalid_key, uint32_t *hcnt, hipStream_t s);
hipError_t launch_heads32(const uint32_t *skey, const uint32_t *srank, uint64_t n, uint32_t invalid_key,
                          const uint64_t *rcnt, HeadRec *hrec, uint32_t *hcnt, hipStream_t s);
hipError_t launch_emit(const EmitArgs &a, hipStream_t s);
hipError_t launch_head_count(const uint32_t *hcnt, const uint8_t *hmark, uint64_t n, uint32_t *ecnt, hipStream_t s);
uint64_t emit_blocks(uint64_t n);
constexpr uint64_t EMIT_DIRECT_MAX = 4096;   // emit workgroups that sum the earlier counts themselves (O(n^2) reads)
// wide keys (2(k - |P|) >= 64 bits, k <= 64): dst[i] = src[idx[i]]; the cross
// entries' keys after apply_cross; heads over (hi, lo) sorted ranks (hcnt
// prefilled with 1, as launch_heads_sparse)
hipError_t launch_gather_u64(const uint64_t *src, const uint32_t *idx, uint64_t n, uint64_t *dst, hipStream_t s);
constexpr uint64_t CP_BLOCK = 4096;   // ranks per compaction workgroup (compact_count / compact_write)
hipError_t launch_compact_count(const uint32_t *k32, const uint64_t *k64, uint64_t n, uint64_t invalid, uint32_t *bcnt,
                                hipStream_t s);
hipError_t launch_compact_write(const uint32_t *k32, const uint64_t *k64, const uint64_t *ord, uint64_t n,
                                uint64_t invalid, const uint64_t *boff, uint32_t *o32, uint64_t *o64, uint64_t *oord,
                                hipStream_t s);
hipError_t launch_cross_wide_fix(const uint32_t *xslot, uint64_t n, const uint64_t *xkeyl, const uint64_t *xkeyh,
                                 uint64_t *rkey, uint64_t *rkeyh, hipStream_t s);
hipError_t launch_heads_wide(const uint64_t *shi, const uint64_t *slo, const uint32_t *srank, uint64_t n,
                             uint64_t invalid_hi, uint32_t *hcnt, hipStream_t s);
// bucket finish (u32 keys of <= BKT_LOW + 11 bits)
constexpr uint32_t BKT_LOW = 14;             // keys per bucket table: 2^14 (128 KiB of LDS: min rank, count)
constexpr uint32_t BKT_MAX = 2048;           // buckets (keys of <= BKT_LOW + 11 bits)
constexpr uint32_t BKT_EPB_HOST = 4096;      // elements per partition block of the counted route (= BKT_EPB)
constexpr uint32_t BKT_OP_EPB_HOST = 8192;   // ... of the one-pass route (= BKT_OP_EPB)
constexpr uint32_t BKT_CUR_STRIDE = 32;      // one-pass partition: one bucket cursor per 128-byte line
// the fixed region of a bucket on the one-pass route: 1.5 x the mean bucket
// size + one block of that route, so that a finish of up to one block fits
// whatever its keys are (a bucket past it sets ERR_BKT_CAP: the counted route
// redoes the finish)
inline uint64_t bucket_cap(uint64_t n, uint32_t nb) { return (n + nb - 1) / nb * 3 / 2 + BKT_OP_EPB_HOST; }
hipError_t launch_bucket_onepass(const uint32_t *key, uint64_t n, uint32_t invalid, uint32_t shift, uint32_t nb,
                                 uint32_t cap, uint32_t *cur, uint16_t *pkey, uint32_t *prank, uint8_t *hmark,
                                 unsigned int *err, uint64_t *stamp, hipStream_t s);
hipError_t launch_bucket_hist(const uint32_t *key, uint64_t n, uint32_t invalid, uint32_t shift, uint32_t nb,
                              uint32_t nblk, uint32_t *H, uint8_t *hmark, uint64_t *stamp, hipStream_t s);
hipError_t launch_bucket_offsets(const uint32_t *H, uint32_t nb, uint32_t nblk, uint32_t *Hs, uint32_t *btot,
                                 uint32_t *bbase, unsigned int *ticket, hipStream_t s);
hipError_t launch_bucket_scatter(const uint32_t *key, uint64_t n, uint32_t invalid, uint32_t shift, uint32_t nb,
                                 uint32_t nblk, const uint32_t *Hs, const uint32_t *bbase, uint16_t *pkey,
                                 uint32_t *prank, hipStream_t s);
// (cur != null: the one-pass route's regions of `cap` entries, totals in the cursors, which it returns to 0)
hipError_t launch_bucket_heads(const uint16_t *pkey, const uint32_t *prank, const uint32_t *bbase, uint32_t nb,
                               uint32_t shift, uint8_t *hmark, uint32_t *hcnt, uint32_t *cur, uint32_t cap, uint64_t n,
                               unsigned int *err, hipStream_t s);
// multi-GPU hit exchange (kmer_exchange_prepare / kmer_finish_exchanged)
struct XHit {
    uint64_t ord;                  // first-occurrence order key
    uint64_t key;                  // packed suffix code
};
constexpr uint32_t XP_MAXW = 256;            // most ranks of one exchange
constexpr uint32_t XP_EPB_HOST = 4096;       // rank slots per partition block (= XP_EPB)
hipError_t launch_xpart_hist(const uint64_t *rkey, const uint32_t *rkey32, uint64_t n, uint64_t invalid,
                             uint32_t kbits, uint32_t world, uint32_t nblk, uint32_t *H, hipStream_t s);
hipError_t launch_xpart_scatter(const uint64_t *rkey, const uint32_t *rkey32, const uint64_t *rord, uint64_t n,
                                uint64_t invalid, uint32_t kbits, uint32_t world, uint32_t nblk, const uint32_t *H,
                                const uint32_t *Hs, XHit *out, uint64_t *counts, hipStream_t s);
hipError_t launch_xprep(const XHit *x, uint64_t n, uint64_t *rkey, uint32_t *rkey32, uint64_t *rord, uint32_t *ridx,
                        hipStream_t s);
hipError_t launch_merge_prep(const uint64_t *keys, const Agg *vals, uint64_t n, uint64_t *rkey, uint32_t *rkey32,
                             uint64_t *rord, uint64_t *rcnt, uint32_t *ridx, hipStream_t s);
hipError_t launch_gather_records(const Record *recs, uint64_t stride, uint64_t n,
                                 const uint8_t *data, uint8_t *out, hipStream_t s);
hipError_t launch_nl_write(const uint8_t *data, uint64_t len, uint32_t n_tiles, const uint64_t *tbase, uint64_t *nl,
                           hipStream_t s);
// one pass: per-tile '\n' counts + tile-relative positions in `cap` u16 slots per
// tile (ERR_LINE_OVERFLOW: a tile had more; fall back to nl_write)
hipError_t launch_nl_slots(const uint8_t *data, uint64_t len, uint32_t n_tiles, uint32_t cap, uint16_t *slots,
                          uint32_t *tcount, unsigned int *err, hipStream_t s);
// sequence lines from the slots (tbase: exclusive scan of tcount)
hipError_t launch_seq_lines_slots(const uint16_t *slots, const uint32_t *tcount, const uint64_t *tbase,
                                  uint32_t n_tiles, uint32_t cap, uint64_t len, uint64_t li0, uint64_t first,
                                  uint64_t n_nl, uint64_t n_seq, uint32_t k, uint32_t step, SeqLine *lines,
                                  uint64_t *wcount, unsigned int *err, uint64_t maxrel, hipStream_t s);
// wcount = windows of both strands per sequence line: 2 ceil(W / step)
hipError_t launch_seq_lines(const uint64_t *nl, uint64_t n_nl, uint64_t len, uint64_t li0, uint64_t n_seq, uint32_t k,
                            uint32_t step, SeqLine *lines, uint64_t *wcount, unsigned int *err, uint64_t maxrel,
                            hipStream_t s);
hipError_t launch_pos_after(StreamPos *pos, uint64_t lines, const uint8_t *data, uint64_t len,
                            unsigned long long *ends_open, hipStream_t s);
hipError_t launch_windows_packed(const WinArgs &a, hipStream_t s);

// ---- table mode (kmer_table.hip): unordered canonical counts ---------------
// Every counted forward window w contributes its canonical planar code
// c = min(code(w), code(rc w)) (planar code: low plane bits of the k bases,
// then the high plane bits, base 0 least significant; A=00 C=01 G=10 T=11 as
// (hi, lo)); h = tab_mix(c) is a bijection.  h's top 10 bits pick the pass-1
// partition, the next 10 the bucket (2^20 buckets), the low 44 bits are the
// remainder kept in the table.  count(x) = C[c] for x in {c, rc c} when x
// starts with P (palindromes: 2 C[c]) -- SURVEY.md App. A.6.
constexpr uint32_t TAB_L1 = 10, TAB_L2 = 10;           // bits per partition level
constexpr uint32_t TAB_NB = 1u << 10;                  // bins per level
constexpr uint32_t TAB_NQ = 1u << (TAB_L1 + TAB_L2);   // buckets
constexpr uint32_t TAB_RBITS = 64 - TAB_L1 - TAB_L2;   // remainder bits (44)
constexpr uint64_t TAB_CMAX = 0xFFFFFull;              // entry count field (20 bits); larger -> big list
constexpr uint64_t TAB_UNIT = 1ull << 18;              // pass-2 keys per workgroup
constexpr uint32_t TAB_FWG = 1024;                     // final workgroup (16 waves, one per CU)
constexpr uint32_t TAB_SLOTS = 8192;                   // final LDS table slots (96 KiB)
constexpr uint32_t TAB_CAP = 7000;                     // distinct keys per range before it is split (+1024 in flight)

// multiplicative hash: a bijection of the 64-bit code (odd multiplier) whose
// top bits -- partition and bucket -- depend on every bit of the code
constexpr uint64_t TAB_MUL = 0x9E3779B97F4A7C15ull;
__host__ __device__ inline uint64_t tab_mix(uint64_t x) { return x * TAB_MUL; }
constexpr uint64_t tab_inv_odd(uint64_t a) {   // inverse of an odd number mod 2^64 (Newton: 3 -> 96 bits)
    uint64_t x = a;
    for (int i = 0; i < 5; ++i) x *= 2 - a * x;
    return x;
}
constexpr uint64_t TAB_INV = tab_inv_odd(TAB_MUL);
static_assert(TAB_INV * TAB_MUL == 1, "TAB_INV");
// NARROW keys (k <= 21).  The key code c' has 41 bits: odd k -- the
// orientation (w or rc w) whose middle base is A or C, with that base's zero
// high-plane bit taken out (exactly one orientation qualifies: complementing a
// base flips both its bits, and the middle base is its own mirror); even k --
// min(code(w), code(rc w)) (< 2^40).  h = f(c') << 23 with f(x) = (x ^ (x >>
// 21)) TAB_MUL mod 2^41, a bijection of [0, 2^41) (the xor-shift lets the
// bucket bits see every bit).  The remainder's low 23 bits are then 0, and a
// key below its partition fits 31 bits: (uint32_t)(h >> 23) = bucket offset
// << 21 | the remainder's top 21 bits -- the 32-bit keys of pass 1's runs
// (B1) and of pass 2's regions (B2), with TAB_SENT32 free for filler slots.
constexpr uint32_t TAB_NSH = 23;
constexpr uint32_t TAB_NARROW_K = 21;
constexpr uint32_t TAB_SENT32 = 0xFFFFFFFFu;
__host__ __device__ inline uint64_t tab_mix_n(uint64_t x) { return ((x ^ (x >> 21)) * TAB_MUL) << TAB_NSH; }
// pass 1: the narrow key code of a window from its two orientations' codes
__host__ __device__ inline uint64_t tab_canon_n(uint64_t cf, uint64_t cr, uint32_t k) {
    if (!(k & 1)) return cf < cr ? cf : cr;
    const uint32_t pos = k + (k - 1) / 2;             // the middle base's high-plane bit
    const uint64_t c = ((cf >> pos) & 1) ? cr : cf;
    return ((c >> (pos + 1)) << pos) | (c & ((1ull << pos) - 1));
}
// the planar code of h: the canonical code (wide keys) or an orientation of
// the window (narrow keys); inv = TAB_MUL^-1 mod 2^64
__host__ __device__ inline uint64_t tab_code(uint64_t h, uint32_t k, bool narrow, uint64_t inv) {
    if (!narrow) return h * inv;
    const uint64_t z = ((h >> TAB_NSH) * inv) & ((1ull << 41) - 1);
    const uint64_t x = z ^ (z >> 21);
    if (!(k & 1)) return x;
    const uint32_t pos = k + (k - 1) / 2;
    return ((x >> pos) << (pos + 1)) | (x & ((1ull << pos) - 1));
}
// reverse complement of a planar code (k <= 32)
__host__ __device__ inline uint64_t tab_rc_code(uint64_t code, uint32_t k) {
    const uint32_t km = k >= 32 ? ~0u : ((1u << k) - 1u);
    const uint32_t lo = (uint32_t)code & km, hi = (uint32_t)(code >> k) & km;
    const uint32_t rlo = __builtin_bitreverse32(~lo & km) >> (32 - k);
    const uint32_t rhi = __builtin_bitreverse32(~hi & km) >> (32 - k);
    return ((uint64_t)rhi << k) | rlo;
}
// Key arithmetic of a lookup (kmer_lookup.hip, kmer_table_lookup): from the
// k bytes of a query key to the h its class has in the table.
// the planar code of k A/C/G/T bytes (base i at bit i of each plane); false
// when a byte is none of the four
__host__ __device__ inline bool tab_bytes_code(const uint8_t *x, uint32_t k, uint64_t *code) {
    uint32_t lo = 0, hi = 0, ok = 1;
    for (uint32_t i = 0; i < k; ++i) {
        const uint32_t ch = x[i];
        ok &= (uint32_t)(ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T');
        lo |= (((ch >> 1) ^ (ch >> 2)) & 1u) << i;
        hi |= ((ch >> 2) & 1u) << i;
    }
    *code = ((uint64_t)hi << k) | lo;
    return ok != 0;
}
// h of the class {w, rc w} from its two orientations' planar codes: wide keys
// (k >= 22) tab_mix of the smaller code, narrow keys tab_mix_n of the key code
__host__ __device__ inline uint64_t tab_key_h(uint64_t cf, uint64_t cr, uint32_t k) {
    return k <= TAB_NARROW_K ? tab_mix_n(tab_canon_n(cf, cr, k)) : tab_mix(cf < cr ? cf : cr);
}
// key bytes -> h (and the codes of the key and of its reverse complement)
__host__ __device__ inline bool tab_bytes_h(const uint8_t *x, uint32_t k, uint64_t *cf, uint64_t *cr, uint64_t *h) {
    const bool ok = tab_bytes_code(x, k, cf);
    *cr = tab_rc_code(*cf, k);
    *h = tab_key_h(*cf, *cr, k);
    return ok;
}
// x <= y as strings (A < C < G < T, base 0 first), x and y planar codes: the
// order in which the host result names a class (build_table_result)
__host__ __device__ inline bool tab_str_le(uint64_t x, uint64_t y, uint32_t k) {
    const uint32_t km = k >= 32 ? ~0u : ((1u << k) - 1u);
    const uint32_t xl = (uint32_t)x & km, xh = (uint32_t)(x >> k) & km;
    const uint32_t yl = (uint32_t)y & km, yh = (uint32_t)(y >> k) & km;
    const uint32_t d = (xl ^ yl) | (xh ^ yh);
    if (!d) return true;
    const uint32_t j = (uint32_t)__builtin_ctz(d);
    return (((xh >> j) & 1u) * 2 + ((xl >> j) & 1u)) < (((yh >> j) & 1u) * 2 + ((yl >> j) & 1u));
}
// Key arithmetic of the matcher's probe (kmer_probe.hip): from a 2-bit code
// (base j at bits 2 (k - 1 - j) + 1 .. 2 (k - 1 - j), A C G T = 0 1 2 3: the
// matcher's pack_key) to the planar codes of the k-mer and of its reverse
// complement
__host__ __device__ inline uint32_t tab_even_bits(uint64_t x) {   // bits 0, 2, 4 .. 62 of x, packed
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
    return (uint32_t)x;
}
__host__ __device__ inline void tab_code2_planar(uint64_t code2, uint32_t k, uint64_t *cf, uint64_t *cr) {
    // (packed bit m belongs to base k - 1 - m: reversed into base order)
    const uint32_t lo = __builtin_bitreverse32(tab_even_bits(code2)) >> (32 - k);
    const uint32_t hi = __builtin_bitreverse32(tab_even_bits(code2 >> 1)) >> (32 - k);
    *cf = ((uint64_t)hi << k) | lo;
    *cr = tab_rc_code(*cf, k);
}
// Key arithmetic of the table's by-value readers (kmer_abundance.hip): from a
// table entry to the Map keys it stands for, and from a planar code back to
// the matcher's 2-bit code.
__host__ __device__ inline uint64_t tab_spread_bits(uint32_t x) {   // bit m of x at bit 2 m (tab_even_bits' inverse)
    uint64_t v = x;
    v = (v | (v << 16)) & 0x0000FFFF0000FFFFull;
    v = (v | (v << 8)) & 0x00FF00FF00FF00FFull;
    v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
    v = (v | (v << 2)) & 0x3333333333333333ull;
    v = (v | (v << 1)) & 0x5555555555555555ull;
    return v;
}
// planar code -> 2-bit code, first base most significant (tab_code2_planar's
// inverse): 2-bit codes compare as the key bytes do (A < C < G < T)
__host__ __device__ inline uint64_t tab_planar_code2(uint64_t code, uint32_t k) {
    const uint32_t km = k >= 32 ? ~0u : ((1u << k) - 1u);
    const uint32_t lo = (uint32_t)code & km, hi = (uint32_t)(code >> k) & km;
    const uint32_t rlo = __builtin_bitreverse32(lo) >> (32 - k), rhi = __builtin_bitreverse32(hi) >> (32 - k);
    return tab_spread_bits(rlo) | (tab_spread_bits(rhi) << 1);
}
// The Map keys of the table entry h (the loop body of build_table_result):
// their planar codes in keys[0 .. n), n = 0, 1 or 2 the return value; *dbl:
// the value is twice the entry's count (table mode, x == rc x).  Table mode:
// x and rc x, each if it starts with the prefix (one key when x == rc x);
// canonical mode: the smaller string of the class, if it starts with the prefix.
__host__ __device__ inline uint32_t tab_entry_keys(uint64_t h, uint32_t k, uint32_t plo, uint32_t phi, uint32_t pmask,
                                                   bool canonical, uint64_t keys[2], bool *dbl) {
    const uint32_t km = k >= 32 ? ~0u : ((1u << k) - 1u);
    const uint64_t x = tab_code(h, k, k <= TAB_NARROW_K, TAB_INV), r = tab_rc_code(x, k);
    const bool okx = (((((uint32_t)x & km) ^ plo) | (((uint32_t)(x >> k) & km) ^ phi)) & pmask) == 0;
    const bool okr = (((((uint32_t)r & km) ^ plo) | (((uint32_t)(r >> k) & km) ^ phi)) & pmask) == 0;
    *dbl = false;
    if (canonical) {
        const bool fx = tab_str_le(x, r, k);
        keys[0] = fx ? x : r;
        return (fx ? okx : okr) ? 1u : 0u;
    }
    const bool pal = x == r;
    *dbl = pal;
    uint32_t n = 0;
    if (okx) keys[n++] = x;
    if (!pal && okr) keys[n++] = r;
    return n;
}
// the hash the table digest weighs: tab_mix(min(code(w), code(rc w))) for every k
__host__ __device__ inline uint64_t tab_digest_key(uint64_t h, uint32_t k, bool narrow) {
    if (!narrow) return h;
    const uint64_t c = tab_code(h, k, true, TAB_INV), r = tab_rc_code(c, k);
    return tab_mix(c < r ? c : r);
}
// Table digest weight of a key h: the splitmix64 finalizer (kmer_table_digest)
__host__ __device__ inline uint64_t tab_digest_mix(uint64_t h) {
    h ^= h >> 30;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 27;
    h *= 0x94D049BB133111EBull;
    return h ^ (h >> 31);
}

struct TabArgs {
    const uint8_t *data;
    uint64_t len;
    const SeqLine *lines;          // by sequence ordinal (len 0: no windows)
    uint64_t n_lines;
    uint64_t lpw;                  // sequence lines per pass-1 workgroup
    uint32_t nwg;                  // pass-1 workgroups
    uint32_t k;
    uint32_t plo, phi, pmask;      // prefix planes (base i at bit i), mask of |P| bits
    uint32_t canonical;            // non-ACGT windows: forward-strand records, unfiltered (KMER_FLAG_CANONICAL)
    uint32_t narrow;               // k <= 21: h = tab_mix_n(tab_canon_n(..)), and B1 holds 32-bit keys (h >> 23)
    uint32_t *H1;                  // hist: [p * nwg + g]
    const uint64_t *H1s;           // scatter: exclusive scan of H1 (chunk-relative)
    uint64_t base;                 // scatter: session keys before this chunk
    uint64_t *B1;                  // scatter: hashed keys, partition-major
    Record *recs;                  // non-ACGT windows
    unsigned long long *rec_count;
    uint64_t rec_cap;
    unsigned int *err;
    // pass 1 without the counting pass (tab_scatter1f): partition p owns
    // [base + p * PS, base + (p + 1) * PS), PS = R + S: workgroup w's run at
    // p * PS + pcw[w] (pcw[w + 1] - pcw[w] keys), then S spill slots for the
    // keys past their run (cursor pcur[p]; a full spill area counts in
    // pcur[TAB_NB] and the chunk is redone by the counted pass)
    const uint64_t *pcw;
    uint64_t R, S, PS;
    unsigned long long *pcur;
};

// Pass-1 filler of a run's unused tail (tab_scatter1f), skipped by pass 2:
// tab_mix(2^64 - 1), whose code is no k-mer of k <= 31 (codes < 2^62).
constexpr uint64_t TAB_SENT = 0ull - TAB_MUL;

struct TabUnit {                   // pass 2: a run of one pass-1 partition's keys
    uint64_t start;                // first key in B1
    uint64_t hbase;                // H2 index of (bin 0, unit 0) of the partition
    uint32_t len, u, nunits, part; // keys, unit index within the partition, units of the partition, the partition
};

struct TabBig {                    // entries whose count does not fit the 20-bit field
    uint64_t h, count;
};

struct TabFinal {
    const uint64_t *B2;            // keys by bucket
    const uint64_t *start;         // TAB_NQ + 1 bucket starts in B2 (and in out)
    uint64_t *out;                 // per bucket: nd[q] entries (rem << 20 | min(count, TAB_CMAX))
    uint32_t *nd;
    uint32_t sub_bits;             // (unused: ranges are sized per unit from range_keys)
    uint32_t range_keys;           // target keys per LDS range (small buckets are grouped up to it)
    uint32_t cap;                  // claims per range before it is split (<= TAB_CAP)
    TabBig *big;
    unsigned long long *big_count;
    uint64_t big_cap;
    unsigned int *err;
    uint32_t k, plo, phi, pmask;
    uint32_t canonical;            // statistics of the canonical-k-mer view (KMER_FLAG_CANONICAL)
    uint64_t inv;                  // inverse of TAB_MUL mod 2^64 (tab_code)
    uint32_t narrow;               // keys h = tab_mix_n(c) (k <= 21)
    uint32_t b2n;                  // (narrow, capq) B2 holds 32-bit keys: (uint32_t)(h >> 23) (bucket offset, remainder)
    unsigned long long *stats;     // [0] canonical entries [1] Map keys [2] sum of Map counts
    uint32_t qlo, qhi;             // buckets [qlo, qhi) of this table (multi-GPU: the rank's partitions)
    // units the sort kernel (tab_sort_final) leaves to the general kernel: pairs
    // [q, qe) of buckets; the general kernel walks this list instead of
    // [qlo, qhi) when `left` is set
    uint32_t *left;
    unsigned int *left_n;
    // fixed-capacity pass 2 (tab_scatter2f): REGION r = tab_region(q) holds
    // the keys of qg consecutive buckets of one partition (1: one bucket) at
    // B2[r capq .. r capq + inlen[r]), in no order; rstart = the scan of inlen
    // (the compact OUTPUT layout: entries of region r from rstart[r]).  qg 1:
    // rstart is `start`; qg > 1: `start` holds rstart[tab_region(q)] (from
    // tab_region_starts) and the sort final writes each bucket's exact start
    // (wstart) from its counting sort.  capq 0: contiguous buckets, start for
    // both.
    uint64_t capq;
    const uint32_t *inlen;
    uint32_t qg, rpp, gmag;        // buckets per region, regions per partition, ceil(2^20 / qg)
    const uint64_t *rstart;
    uint64_t *wstart;
};

// fixed pass-2 region of bucket q (qg buckets per region, rpp regions per partition)
__host__ __device__ inline uint32_t tab_region(uint32_t q, uint32_t rpp, uint32_t gmag) {
    return (q >> TAB_L2) * rpp + (((q & (TAB_NB - 1)) * gmag) >> 20);
}

constexpr uint64_t TAB_PIECE = 4096;                   // windows per piece of a long line (pass 1)
hipError_t launch_tab_piece_count(const uint64_t *wcount, uint64_t n, uint32_t *pc, uint32_t *split, hipStream_t s);
hipError_t launch_tab_piece_write(const SeqLine *lines, const uint64_t *wcount, const uint64_t *pbase, uint64_t n,
                                  uint32_t k, SeqLine *out, hipStream_t s);
hipError_t launch_tab_hist1(const TabArgs &a, hipStream_t s);
hipError_t launch_tab_scatter1(const TabArgs &a, hipStream_t s);
hipError_t launch_tab_p1_offsets(const uint64_t *H1s, uint32_t nwg, uint64_t *out, hipStream_t s);
hipError_t launch_tab_hist2(const uint64_t *B1, const TabUnit *units, uint32_t n_units, uint32_t *H2, hipStream_t s);
hipError_t launch_tab_scatter2(const uint64_t *B1, const TabUnit *units, uint32_t n_units, const uint64_t *H2s,
                               uint64_t *B2, hipStream_t s);
hipError_t launch_tab_starts(const uint64_t *H2s, const uint32_t *H2, uint64_t nh, const TabUnit *pfirst,
                             uint64_t *start, hipStream_t s);
// pass 2 without its histogram: one workgroup per partition p in [p0, p0 +
// np), bucket q's keys at B2[q cap ..) (capacity cap, a multiple of 8);
// blen[q] = its keys; a bucket past its capacity sets ERR_TAB_CAP (the caller
// redoes pass 2 with the counted route)
hipError_t launch_tab_scatter2f(const uint64_t *B1, const TabUnit *units, const uint32_t *ufirst, uint32_t p0,
                                uint32_t np, uint64_t cap, uint32_t rpp, uint32_t gmag, bool narrow, bool b1n,
                                void *B2, uint32_t *blen, unsigned int *err, hipStream_t s);
// start[q] = rstart[tab_region(q)] for every bucket, start[TAB_NQ] = the total
hipError_t launch_tab_region_starts(const uint64_t *rstart, uint32_t rpp, uint32_t gmag, uint64_t *start,
                                    hipStream_t s);
hipError_t launch_tab_scatter1f(const TabArgs &a, hipStream_t s);
hipError_t launch_tab_wg_windows(const SeqLine *lines, uint64_t n, uint64_t lpw, uint32_t k, uint32_t nwg,
                                 uint64_t *W, hipStream_t s);
// pass-1 spill areas (tab_scatter1f): the unused slots of each partition's
// spill area filled with TAB_SENT
hipError_t launch_tab_spill_fill(bool narrow, uint64_t *B1, uint64_t base, uint64_t R, uint64_t S, uint64_t PS,
                                 const unsigned long long *pcur, hipStream_t s);
hipError_t launch_tab_final(const TabFinal &a, uint32_t grid, hipStream_t s);
hipError_t launch_tab_sort_final(const TabFinal &a, uint32_t grid, hipStream_t s);
// sort-final workgroup (8 waves, two per CU)
constexpr uint32_t TAB_SWG = 512;
constexpr uint64_t TAB_SORT_KEYS = 12288;               // sort final: keys of a unit (one bucket, or narrow keys: TS_CAP1)
constexpr uint64_t TAB_SORT_KEYS_BIG = 12160;           // ... with 16,384 bins (fixed regions: tab_sort_final_kernel<14>)
constexpr uint64_t TAB_SORT_GROUP_KEYS = 6144;          // sort final: keys of a unit of several buckets (TS_CAPG)
hipError_t launch_tab_digest(const uint64_t *ent, const uint64_t *start, const uint32_t *nd, uint32_t k,
                            uint32_t narrow, unsigned long long *out,
                             hipStream_t s);
// A finished table as its readers see it (kmer_lookup.hip, kmer_probe.hip, kmer_screen.hip ...);
// filled in one place, table_view (kmer_api.hip)
struct TabView {
    const uint64_t *ent;           // the table: entries, TAB_NQ + 1 bucket starts, entries per bucket
    const uint64_t *start;
    const uint32_t *nd;
    uint64_t cap;                  // entries the table's buffer holds (start[TAB_NQ] is at most this)
    const TabBig *big;
    uint64_t n_big;
    uint32_t k, plo, phi, pmask;   // prefix planes (base i at bit i), mask of |P| bits
    uint32_t canonical;            // KMER_FLAG_CANONICAL: only the class's smaller string is a key, never doubled
    unsigned int *err;             // ERR_TAB_LOOKUP ...
    uint32_t *badq;                // ... and a bucket it was raised for
};
// Batched lookup against a finished table (kmer_lookup.hip): counts[i] = the
// Map value of the k bytes at keys + i k (0: absent, filtered, or not A/C/G/T)
struct TabLookup : TabView {
    const uint8_t *keys;
    uint64_t n;
    uint64_t *counts;
};
hipError_t launch_tab_lookup(const TabLookup &a, uint32_t n_cu, hipStream_t s);
// The matcher's probe of a finished table (kmer_probe.hip): the m distinct
// k-mers of a template DB, U[i] their 2-bit codes (first base most
// significant, ascending), O the CSR offsets of their template lists.  DB
// k-mer i is in the query iff its Map value is > 0: qidx[i] = i or 0xFFFFFFFF,
// hc[i] = its list length or 0, present[i] = 1 or 0, cnt[i] = the value.
struct TabProbe : TabView {
    const uint64_t *U, *O;
    uint64_t m;
    uint32_t *bkt, *bkt2, *idx, *idx2;   // scratch, m each: the probes' buckets and DB indices, sorted by bucket
    void *tmp;                           // scratch of the sort (bucket_sort_bytes)
    size_t tmp_bytes;
    uint32_t *qidx;
    uint64_t *hc;
    uint32_t *present;
    uint64_t *cnt;
};
hipError_t launch_tab_probe(const TabProbe &a, uint32_t n_cu, hipStream_t s);
// The sort of m (bucket or TAB_NQ: no probe, index) pairs by bucket that the
// probe and the screen's sorted route share (kmer_probe.hip): one radix sort
// over TAB_QBITS bits; *sb / *si: where the sorted pairs are
constexpr uint32_t TAB_QBITS = TAB_L1 + TAB_L2 + 1;
hipError_t bucket_sort_bytes(uint64_t m, size_t *bytes);
hipError_t launch_bucket_sort(uint32_t *bkt, uint32_t *bkt2, uint32_t *idx, uint32_t *idx2, uint64_t m, void *tmp,
                              size_t tmp_bytes, const uint32_t **sb, const uint32_t **si, hipStream_t s);
// The windows of all lines (reads, records) of an input numbered in input
// order and worked in pieces of consecutive windows, WALK_NS per lane
// (kmer_device.hpp: walk_windows); a piece may end inside a line
constexpr uint32_t WALK_NS = 16;                       // consecutive windows per lane
struct WinWalk {
    const uint8_t *data;           // the input: nothing outside [data, data + len) is loaded
    uint64_t len;
    const SeqLine *lines;          // by line (len 0: no windows)
    const uint64_t *wbase2;        // by line: twice the index of its first window (scan of 2W)
    uint64_t n, total;             // lines, windows of all lines
    uint64_t p0, m;                // the piece: windows [p0, p0 + m)
};
// Read screen against a finished table (kmer_screen.hip, kmer_table_screen):
// every forward window w of every read is one probe, by its class {w, rc w}.
// The weight of a window is the value its read's own Map gives the class's
// keys: table mode -- the orientations that start with the prefix (a
// self-complementary window counts for both strands: 2 if it starts with it);
// canonical mode -- 1 if the class's smaller string starts with it.  cf / cr:
// the planar codes of w and rc w.  *dbl: the table's count is doubled (table
// mode, w == rc w), as tab_entry_keys doubles it.
__host__ __device__ inline uint32_t screen_weight(uint64_t cf, uint64_t cr, uint32_t k, uint32_t plo, uint32_t phi,
                                                  uint32_t pmask, bool canonical, bool *dbl) {
    const uint32_t km = k >= 32 ? ~0u : ((1u << k) - 1u);
    const uint32_t f = (((((uint32_t)cf & km) ^ plo) | (((uint32_t)(cf >> k) & km) ^ phi)) & pmask) == 0 ? 1u : 0u;
    const uint32_t r = (((((uint32_t)cr & km) ^ plo) | (((uint32_t)(cr >> k) & km) ^ phi)) & pmask) == 0 ? 1u : 0u;
    *dbl = false;
    if (canonical) return tab_str_le(cf, cr, k) ? f : r;
    if (cf == cr) {
        *dbl = true;
        return 2u * f;
    }
    return f + r;
}
// Window m of a line's bit planes (bit j of LO / HI: the low / high code bit
// of byte j, as pass 1 forms them; m + k <= 64): the planar codes of w and rc w
__host__ __device__ inline void screen_window_codes(uint64_t LO, uint64_t HI, uint32_t m, uint32_t k, uint64_t *cf,
                                                    uint64_t *cr) {
    const uint32_t km = k >= 32 ? ~0u : ((1u << k) - 1u);
    const uint32_t flo = (uint32_t)(LO >> m) & km, fhi = (uint32_t)(HI >> m) & km;
    const uint32_t rlo = __builtin_bitreverse32(~flo & km) >> (32 - k);
    const uint32_t rhi = __builtin_bitreverse32(~fhi & km) >> (32 - k);
    *cf = ((uint64_t)fhi << k) | flo;
    *cr = ((uint64_t)rhi << k) | rlo;
}
// the one-byte code of a window: its weight (0, 1, 2), SC_DBL when the table's
// count is doubled, or SC_SKIP (a byte outside A/C/G/T: a record key, not matched)
constexpr uint8_t SC_WMASK = 3, SC_DBL = 4, SC_SKIP = 0x80;
constexpr uint64_t SC_PIECE = 1ull << 26;              // windows per piece
constexpr uint64_t SC_PIECE_TEST = 4096;               // ... with KMER_SCREEN_PIECE_TEST
struct ScreenRow {                                     // (kmer_read_screen)
    uint64_t windows, hits, skipped, sum;
};
struct TabScreen : TabView, WinWalk {                  // (the lines are the reads)
    uint64_t *h;                   // by window of the piece: tab_key_h of its class
    uint8_t *code;                 // ... its code (SC_*)
    uint64_t *val;                 // ... the Map value of its class (0: absent or no probe)
    uint32_t *bkt, *idx;           // sorted route: (bucket or TAB_NQ, window of the piece), or null
    uint64_t min_count;            // >= 1
    ScreenRow *rows;
};
hipError_t launch_screen_keys(const TabScreen &a, uint32_t n_cu, hipStream_t s);
// sb / si: the piece's probes sorted by bucket (sorted route), or null: window order
hipError_t launch_screen_probe(const TabScreen &a, const uint32_t *sb, const uint32_t *si, uint32_t n_cu,
                               hipStream_t s);
hipError_t launch_screen_reduce(const TabScreen &a, hipStream_t s);
// Read filter (kmer_filter.hip, kmer_table_filter): the records of the screened
// reads that pass the predicate, compacted on the device.
// a * b as a 96-bit number (hi: bits 64.., lo: bits 0..63), exact
__host__ __device__ inline void filter_mul96(uint64_t a, uint32_t b, uint64_t *hi, uint64_t *lo) {
    const uint64_t l = (a & 0xFFFFFFFFull) * b;
    const uint64_t h = (a >> 32) * b + (l >> 32);
    *lo = (h << 32) | (l & 0xFFFFFFFFull);
    *hi = h >> 32;
}
// match(r): hits >= min_hits AND hits * frac_den >= frac_num * windows, the
// products in exact arithmetic (kmer_api.h, kmer_filter_params)
__host__ __device__ inline bool filter_match(uint64_t hits, uint64_t windows, uint64_t min_hits, uint32_t frac_num,
                                             uint32_t frac_den) {
    if (hits < min_hits) return false;
    uint64_t lh, ll, rh, rl;
    filter_mul96(hits, frac_den, &lh, &ll);
    filter_mul96(windows, frac_num, &rh, &rl);
    return lh > rh || (lh == rh && ll >= rl);
}
constexpr uint32_t FILTER_DROP = 1u, FILTER_PAIRED = 2u;   // (KMER_FILTER_*)
constexpr uint32_t FL_TILE = 4096;                     // output bytes per workgroup tile of the copy: 256 lanes x 16
constexpr uint32_t FL_SEGS = FL_TILE / 4 + 2;          // segment bounds a tile can hold (a record is >= 4 bytes), + the end
struct FilterScan {                                    // per record, then its inclusive scan
    uint64_t kept, bytes, segs;                        // kept records, their bytes, kept runs begun
};
struct FilterScanPlus {
    __host__ __device__ FilterScan operator()(const FilterScan &x, const FilterScan &y) const {
        return FilterScan{x.kept + y.kept, x.bytes + y.bytes, x.segs + y.segs};
    }
};
struct FilterArgs {
    const uint8_t *data;           // the input: nothing outside [data, data + len) is loaded
    uint64_t len;
    uint64_t n_nl, n_reads;        // '\n' of the input, records
    // the '\n' positions as chunk_lines left them: per-tile slots, or nl (flat) when slots is null
    const uint16_t *slots;
    const uint32_t *tcount;
    const uint64_t *tbase;
    uint32_t n_tiles, cap;
    const uint64_t *nl;
    const ScreenRow *rows;         // by read
    uint64_t min_hits;
    uint32_t frac_num, frac_den, flags;
    uint64_t *rend;                // by record: its end (the start of the next one)
    uint8_t *keep;                 // by record: 0 / 1
    FilterScan *scan;              // by record
    uint64_t *seg_src, *seg_out;   // by kept run: where it begins in the input / in the output; seg_out[n_segs] = out_len
    uint64_t n_segs, out_len;      // (the copy)
    uint8_t *out;                  // 16-byte aligned, room for out_len rounded up to 16
};
hipError_t launch_filter_ends(const FilterArgs &a, hipStream_t s);
hipError_t launch_filter_mark(const FilterArgs &a, hipStream_t s);
hipError_t launch_filter_segments(const FilterArgs &a, hipStream_t s);
hipError_t launch_filter_copy(const FilterArgs &a, uint32_t n_cu, hipStream_t s);
// Template DB from FASTA (kmer_dbfasta.hip, kmer_db_open_fasta): every forward
// window w of every record's joined sequence gives the A/C/G/T keys of "the
// record's own Map" as the matcher's 2-bit codes.  The keys of a window, from
// the planar codes of w and rc w: their number is the window's weight
// (screen_weight: the value the record's Map gains by it), so a
// self-complementary window of a non-canonical configuration gives its one key
// twice (the DB's dedup drops the repeat; `lengths` counts both).
__host__ __device__ inline uint32_t dbf_window_keys(uint64_t cf, uint64_t cr, uint32_t k, uint32_t plo, uint32_t phi,
                                                    uint32_t pmask, bool canonical, uint64_t keys[2]) {
    bool dbl;
    const uint32_t wt = screen_weight(cf, cr, k, plo, phi, pmask, canonical, &dbl);
    if (wt == 0) return 0;
    if (canonical) {
        keys[0] = tab_planar_code2(tab_str_le(cf, cr, k) ? cf : cr, k);
    } else if (wt == 2) {                               // (both orientations start with the prefix, or w == rc w)
        keys[0] = tab_planar_code2(cf, k);
        keys[1] = tab_planar_code2(cr, k);
    } else {                                            // the one orientation that starts with the prefix
        const uint32_t km = k >= 32 ? ~0u : ((1u << k) - 1u);
        const bool f = (((((uint32_t)cf & km) ^ plo) | (((uint32_t)(cf >> k) & km) ^ phi)) & pmask) == 0;
        keys[0] = tab_planar_code2(f ? cf : cr, k);
    }
    return wt;
}
constexpr uint64_t DBF_PIECE = 1ull << 26;             // windows per piece
constexpr uint64_t DBF_PIECE_TEST = 4096;              // ... with KMER_DB_PIECE_TEST
struct DbFasta : WinWalk {                             // (the input is the rewritten FASTA, the lines its records)
    uint32_t k, plo, phi, pmask, canonical;
    uint32_t t0;                   // template index of record 0
    uint32_t *cnt;                 // count pass: keys of each lane's windows (one per WALK_NS windows of the piece)
    const uint64_t *off;           // write pass: their exclusive scan
    uint64_t *codes;               // write pass: the piece's pairs, in window order
    uint32_t *tmpl;
    uint64_t n_pairs;              // pairs of the piece (the scan's total)
    uint64_t *lengths;             // by record: pairs so far (a record cut by a piece edge adds up over the pieces)
};
hipError_t launch_dbf_keys(const DbFasta &a, bool write, uint32_t n_cu, hipStream_t s);
hipError_t launch_dbf_lengths(const DbFasta &a, hipStream_t s);
// the records' header lines in the rewritten FASTA: nlen[r] = bytes of record
// r's name (the header without '>'), then gathered back to back at noff[r]
hipError_t launch_dbf_name_lens(const uint8_t *data, uint64_t len, const SeqLine *lines, uint64_t n_rec,
                                uint64_t *nlen, hipStream_t s);
hipError_t launch_dbf_names(const uint8_t *data, const SeqLine *lines, uint64_t n_rec, const uint64_t *noff,
                            const uint64_t *nlen, uint8_t *out, hipStream_t s);
// The by-value readers of a finished table (kmer_abundance.hip).  Spectrum:
// hist[v] += the Map keys with value v, over the entries whose count is in
// the 20-bit field (the host adds the big list and the record keys); counts
// 1 .. AB_REGS are kept in registers, counts below AB_LDS_BINS in LDS.
// Extract: the Map keys with lo <= value <= hi as (2-bit code, value) pairs,
// first counted (n_out = their number), then written at codes / vals in no
// order (n_out = the cursor, cap_out = the counted number), sorted by code
// and decoded to key bytes.
constexpr uint32_t AB_REGS = 4;
constexpr uint32_t AB_LDS_BINS = 4096;
constexpr uint32_t AB_HIST_BINS = 1u << 21;            // every value of a 20-bit count, doubled
struct TabAbund : TabView {
    unsigned long long *hist;      // spectrum: AB_HIST_BINS bins, zeroed by the caller
    uint64_t lo, hi;               // extract: the range, both ends included
    unsigned long long *n_out;
    uint64_t cap_out;
    uint64_t *codes, *vals;
};
hipError_t launch_tab_spectrum(const TabAbund &a, hipStream_t s);
// out[0] = sum of hist[from ..), out[1] = sum of v hist[v] over the same bins (out zeroed by the caller)
hipError_t launch_tab_spectrum_tail(const unsigned long long *hist, uint32_t from, unsigned long long *out,
                                    hipStream_t s);
hipError_t launch_tab_extract_count(const TabAbund &a, hipStream_t s);
hipError_t launch_tab_extract_write(const TabAbund &a, hipStream_t s);
hipError_t tab_extract_sort_bytes(uint64_t n, uint32_t k, size_t *bytes);
hipError_t launch_tab_extract_sort(uint64_t *codes, uint64_t *codes2, uint64_t *vals, uint64_t *vals2, uint64_t n,
                                   uint32_t k, void *tmp, size_t tmp_bytes, const uint64_t **sorted_codes,
                                   const uint64_t **sorted_vals, hipStream_t s);
hipError_t launch_tab_extract_decode(const uint64_t *codes, uint64_t n, uint32_t k, uint8_t *keys, uint32_t n_cu,
                                     hipStream_t s);
// Set operations of two finished tables (kmer_setops.hip): bucket q of A can
// only meet bucket q of B (same k, hash and 2^20 buckets), so the tables are
// joined bucket by bucket, on the class (the remainder); the Map keys and the
// doubling of a class (tab_entry_keys) are the same on both sides and are
// applied afterwards.  A pair of long buckets is joined by one wave in its LDS
// slice: the staged side S as an open-addressing table of at most JOIN_SLOTS
// slots keyed by remainder (at most JOIN_TILE entries in join_slots(entries)
// slots, load <= 1/2; slot value 0 = empty: a staged entry has a count field
// > 0), the probing side P streamed.
// A side of more than JOIN_TILE entries is split by leading bits of the
// remainder's significant part (narrow keys: the low TAB_NSH bits are 0) into
// ranges (depth s, index t): a range that still holds more than JOIN_TILE
// entries of S is halved, (s, t) -> (s + 1, 2 t) and (s + 1, 2 t + 1).
// Remainders within a bucket are distinct, so a range of width 1 holds one
// entry and the halving ends at s <= join_width.  The helpers below are the
// whole arithmetic (checked on the CPU by tests/native/setops_keys_check.hip).
constexpr uint32_t JOIN_TILE = 1024;                   // staged entries per wave (16 KiB of LDS at load 1/2)
constexpr uint32_t JOIN_SLOTS = 2 * JOIN_TILE;
constexpr uint32_t JOIN_LANE_MAX = 16;                 // both buckets up to this long: the pair's own lane joins them
// the significant bits of a remainder and their number
__host__ __device__ inline uint32_t join_width(bool narrow) { return narrow ? TAB_RBITS - TAB_NSH : TAB_RBITS; }
__host__ __device__ inline uint64_t join_sig(uint64_t rem, bool narrow) { return narrow ? rem >> TAB_NSH : rem; }
// the first split depth tried for a staged side of len entries: 0 when it fits
// the tile, else the depth at which the mean range is at most 3/4 of a tile
__host__ __device__ inline uint32_t join_depth0(uint64_t len) {
    uint32_t s = 0;
    if (len <= JOIN_TILE) return 0;
    while ((len >> s) > JOIN_TILE * 3 / 4) ++s;
    return s;
}
// the range of depth s (<= width) that holds sig: its leading s bits
__host__ __device__ inline uint64_t join_sub(uint64_t sig, uint32_t width, uint32_t s) {
    return s ? sig >> (width - s) : 0;
}
// the range after (s, t) is done, ranges above depth s0 in depth-first order;
// false after the last one
__host__ __device__ inline bool join_next(uint32_t s0, uint32_t *s, uint64_t *t) {
    while (*s > s0 && (*t & 1)) {
        *t >>= 1;
        --*s;
    }
    ++*t;
    return !(*s == s0 && *t == (1ull << s0));
}
// the slots of a table of n <= JOIN_TILE staged entries: a power of two >= 2 n, at least a wave's 64
__host__ __device__ inline uint32_t join_slots(uint32_t n) {
    uint32_t m = 64;
    while (m < 2 * n && m < JOIN_SLOTS) m <<= 1;
    return m;
}
// first slot probed for sig in a table of nslots slots (then linear, wrapping)
__host__ __device__ inline uint32_t join_slot(uint64_t sig, uint32_t nslots) {
    return (uint32_t)((sig * TAB_MUL) >> 40) & (nslots - 1);
}
enum { JOIN_INTERSECT = 0, JOIN_SUBTRACT = 1, JOIN_UNION = 2 };   // (KMER_SETOP_*)
// The result as a table (kmer_table_setop_into): the arithmetic of one class.
// The Map value one walk gives a class with the values va / vb on the two
// sides (0: not there); `second`: JOIN_UNION's second walk.  0: no result.
__host__ __device__ inline uint64_t join_result(uint32_t op, bool second, uint64_t va, uint64_t vb, uint64_t min_a,
                                                uint64_t min_b) {
    const bool in_a = va >= min_a, in_b = vb >= min_b;
    if (op == JOIN_INTERSECT) return in_a && in_b ? (va < vb ? va : vb) : 0;
    if (op == JOIN_SUBTRACT) return in_a && !in_b ? va : 0;
    if (!second) return in_a ? va + (in_b ? vb : 0) : 0;
    return in_b && !in_a ? vb : 0;
}
// the class count C behind a result value: both sides double a
// self-complementary class alike, so its value is even
__host__ __device__ inline uint64_t join_class_count(uint64_t v, bool dbl) { return dbl ? v >> 1 : v; }
// the result's entry of a class: rem << 20 | min(C, TAB_CMAX); *big: C goes to the big list as well
__host__ __device__ inline uint64_t join_entry(uint64_t rem, uint64_t C, bool *big) {
    *big = C >= TAB_CMAX;
    return (rem << 20) | (C < TAB_CMAX ? C : TAB_CMAX);
}
// slot `off` of a result bucket of nd entries that begins at `start` in a table of cap entries: may it be written?
__host__ __device__ inline bool join_slot_ok(uint64_t start, uint32_t off, uint32_t nd, uint64_t cap) {
    return off < nd && start <= cap && off < cap - start;
}
struct TabJoin {
    TabView a, b;                  // nd == nullptr: an empty table; the key parameters (k, prefix, mode) are a's
    uint64_t min_a, min_b;         // a key is in a side iff its value there is >= this (>= 1)
    uint32_t op;                   // setop: JOIN_*
    uint32_t second;               // JOIN_UNION's second walk: B's keys that are not in A
    unsigned long long *sums;      // compare: the 8 words of kmer_table_overlap
    unsigned long long *n_out;     // setop: counted keys, then the write cursor
    uint64_t cap_out;
    uint64_t *codes, *vals;        // setop: (2-bit code, value) pairs, as the extract's
    unsigned int *err;             // ERR_TAB_LOOKUP / ERR_TAB_EXTRACT ...
    uint32_t *badq;                // ... [0] the bucket, [1] the side (0 a, 1 b)
    // the result as a table (launch_tab_join_tcount / twrite).  n_out: the
    // result entries with a count >= TAB_CMAX (count), the big list's cursor (write)
    uint32_t *nd_dst;              // count: result entries of bucket q (stored; JOIN_UNION's second walk adds)
    const uint64_t *start_dst;     // write: their exclusive scan (TAB_NQ + 1)
    uint32_t *cur_dst;             // write, JOIN_UNION: the offset the first walk reached in bucket q
    uint64_t *ent_dst;             // write: the result's entries ...
    uint64_t cap_dst;              // ... as many as the scan's total
    TabBig *big_dst;
    uint64_t big_cap;
    unsigned long long *stats;     // write: [0] classes [1] Map keys [2] sum of Map values
};
hipError_t launch_tab_join_compare(const TabJoin &j, hipStream_t s);
hipError_t launch_tab_join_count(const TabJoin &j, hipStream_t s);
hipError_t launch_tab_join_write(const TabJoin &j, hipStream_t s);
hipError_t launch_tab_join_tcount(const TabJoin &j, hipStream_t s);
hipError_t launch_tab_join_twrite(const TabJoin &j, hipStream_t s);
// multi-GPU table exchange: copy n segments {src offset, dst offset, length}
// of u64 keys (one workgroup per segment, grid-strided)
struct TabSeg {
    uint64_t src, dst, len;
    uint64_t part;                 // (tab_widen) the segment's pass-1 partition
};
hipError_t launch_tab_segcopy(const uint64_t *src, const TabSeg *segs, uint32_t n, uint64_t *dst, hipStream_t s);
// 32-bit pass-1 keys (narrow) -> 64-bit h (segment src/dst in keys; filler -> TAB_SENT)
hipError_t launch_tab_widen(const uint32_t *src, const TabSeg *segs, uint32_t n, uint64_t *dst, hipStream_t s);
// FASTA input (kmer_fasta.hip, KMER_FLAG_FASTA): a chunk of FASTA rewritten
// as FASTQ-shaped lines (header, joined sequence, "", "" per record).  A tile
// of 16 KiB is a function of the header state it inherits: kind 0 passes the
// state through, 1 / 2 leave it 0 / 1; c0 / c1 = output bytes for an incoming
// state 0 / 1; nl = input '\n' bytes.  Composed by an exclusive scan.
struct FaTile {
    uint32_t kind, pad;
    uint64_t c0, c1, nl;
};
__host__ __device__ inline FaTile fa_tile_compose(const FaTile &a, const FaTile &b) {
    FaTile r;
    const uint32_t s0 = a.kind ? a.kind - 1 : 0u, s1 = a.kind ? a.kind - 1 : 1u;
    r.kind = b.kind ? b.kind : a.kind;
    r.pad = 0;
    r.c0 = a.c0 + (s0 ? b.c1 : b.c0);
    r.c1 = a.c1 + (s1 ? b.c1 : b.c0);
    r.nl = a.nl + b.nl;
    return r;
}
hipError_t launch_fa_tiles(const uint8_t *data, uint64_t len, uint32_t n_tiles, FaTile *tiles, hipStream_t s);
hipError_t launch_fa_write(const uint8_t *data, uint64_t len, uint32_t n_tiles, const FaTile *tiles_x, uint8_t *out,
                           hipStream_t s);
hipError_t launch_synth_fastq(uint8_t *out, uint64_t seed, uint64_t first_read, uint64_t n_reads,
                              hipStream_t s);
hipError_t launch_gen_append(const Record *recs, uint64_t n, const uint8_t *data, uint32_t k, uint8_t *keys,
                             uint64_t *cnt, uint64_t *first, hipStream_t s);
hipError_t launch_gen_hash(const uint8_t *keys, uint64_t n, uint32_t k, uint64_t seed, uint64_t *h1, uint64_t *h2,
                           uint32_t *idx, hipStream_t s);
hipError_t launch_gen_heads(const uint64_t *h1, const uint64_t *h2, const uint32_t *idx, uint64_t n, const uint8_t *keys,
                            uint32_t k, uint32_t *head, unsigned int *collide, hipStream_t s);
hipError_t launch_gen_starts(const uint32_t *head, const uint32_t *gid, uint64_t n, uint32_t *start, hipStream_t s);
hipError_t launch_gen_reduce(const uint32_t *start, uint64_t ng, const uint32_t *idx, const uint8_t *keys,
                             const uint64_t *cnt, const uint64_t *first, uint32_t k, uint8_t *okeys, uint64_t *ocnt,
                             uint64_t *ofirst, hipStream_t s);
hipError_t launch_permute_rows(const uint8_t *keys, const uint64_t *cnt, const uint64_t *first, const uint32_t *idx,
                               uint64_t n, uint32_t k, uint8_t *okeys, uint64_t *ocnt, uint64_t *ofirst,
                               hipStream_t s);


}  // namespace kmerhip

struct kmer_ctx;

namespace kmerhip {

// The finished table of a single-device table-mode context for the matcher
// (kmer_api.hip; kmer_match_open_table): the context settled and its state
// checked as for a lookup, the view filled.  Returns a kmer_status; on a
// failure the message is the context's last error.
struct TabOwner {
    hipStream_t stream;            // the context's stream (the table's writers are queued on it)
    int device;
    uint32_t k, n_cu;
    bool empty;                    // a finish with no keys: the view is not filled
};
int table_view(kmer_ctx *c, TabView *v, TabOwner *o);

// The (2-bit code, template) pairs of FASTA genomes for the matcher
// (kmer_dbfasta.hip; kmer_db_open_fasta*): gathered with the context's FASTA
// rewrite, line finder, stream and scratch, template-major, duplicates
// included, complete (the context's stream waited for) on return.  The arrays
// are the caller's: dbfasta_release.  Returns a kmer_status; on a failure
// nothing is held and the message is the context's last error.
struct DbFastaPairs {
    int device;
    uint32_t k;
    uint64_t *codes;               // device, n
    uint32_t *tmpl;
    uint64_t n, cap;
    uint32_t nt;                   // records = templates
    uint64_t *lengths;             // host (malloc), nt: pairs per template
    char *names;                   // host (malloc): the names back to back
    uint64_t *name_off;            // host (malloc), nt + 1
};
// the state checks that need the context (k, step, group, open session): before any device call
int dbfasta_check(kmer_ctx *c);
int dbfasta_gather(kmer_ctx *c, const uint8_t *bytes, uint64_t len, bool on_device, uint32_t flags, void *stream,
                   DbFastaPairs *out);
void dbfasta_release(DbFastaPairs *p);

}  // namespace kmerhip
