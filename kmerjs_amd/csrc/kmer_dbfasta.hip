// kmer_dbfasta.hip — the template DB's (k-mer, template) pairs straight from
// FASTA genomes (gfx950): kmer_db_open_fasta / kmer_db_open_fasta_device
// (include/kmer_match.h).  The replacement of the reference's offline ETL
// (src/kmerPyToMongo.py): record r of the input is template r, its k-mers are
// the A/C/G/T keys of the record's own Map under the context's configuration.
//
// Per piece of input (the whole device buffer, or one upload of the host call):
//   rewrite  fasta_rewrite (kmer_fasta.hip): each record's joined sequence is
//            one line, line 4 r + 1 of the rewritten buffer
//   lines    chunk_lines from line phase 0 without a length limit: one SeqLine
//            and window count per record; their exclusive scan numbers the
//            windows of all records in input order
//   keys     dbf_keys_kernel: a lane takes WALK_NS consecutive windows
//            (kmer_device.hpp: walk_windows, as the screen's keys kernel does)
//            and evaluates each (dbf_window_keys).  Two passes over the same
//            code: COUNT the keys of each lane -> exclusive scan -> WRITE the
//            (2-bit code, template) pairs at the scanned offsets.  The pairs
//            come out in window order, so template-major: what the stable
//            sort of the DB build (kmer_match.hip) needs for ascending
//            templates inside a k-mer's list.  One writer per slot, no atomics.
//   lengths  per record, the pairs that carry its template: two binary
//            searches in the piece's (ascending) template column
//   names    the header lines of the rewritten buffer, gathered back to back
// The pairs of all pieces are appended to one pair of arrays that the DB build
// then sorts; device memory is the piece plus the pairs gathered so far.
#include "kmer_device.hpp"
#include "kmer_host.hpp"

namespace kmerhip {

namespace {

template <bool WRITE>
__global__ __launch_bounds__(256) void dbf_keys_kernel(const DbFasta a) {
    const uint32_t k = a.k;
    const uint64_t ngroups = (a.m + WALK_NS - 1) / WALK_NS;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t n = 0;                                          // keys of this lane's windows so far
        uint64_t o = 0;
        if (WRITE) o = a.off[g];
        walk_windows(a, k, g, [&](uint64_t, uint64_t r, uint64_t LO, uint64_t HI, uint32_t m, bool acgt) {
            if (!acgt) return;                                   // a byte outside A/C/G/T: a record key, not in the DB
            uint64_t cf, cr, keys[2];
            screen_window_codes(LO, HI, m, k, &cf, &cr);
            if (!WRITE) {
                bool dbl;
                n += screen_weight(cf, cr, k, a.plo, a.phi, a.pmask, a.canonical != 0, &dbl);
            } else {
                const uint32_t c = dbf_window_keys(cf, cr, k, a.plo, a.phi, a.pmask, a.canonical != 0, keys);
                for (uint32_t j = 0; j < c; ++j) {
                    if (o + n < a.n_pairs) {                     // (the counted slots: the two passes agree)
                        a.codes[o + n] = keys[j];
                        a.tmpl[o + n] = a.t0 + (uint32_t)r;
                    }
                    ++n;
                }
            }
        });
        if (!WRITE) a.cnt[g] = n;
    }
}

// lengths[r] += the pairs of the piece whose template is t0 + r
__global__ __launch_bounds__(256) void dbf_lengths_kernel(const DbFasta a) {
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.n; r += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t t = a.t0 + (uint32_t)r;
        uint64_t lo = 0, hi = a.n_pairs;
        while (lo < hi) {                                        // first pair of a template >= t
            const uint64_t mid = (lo + hi) >> 1;
            if (a.tmpl[mid] < t) lo = mid + 1;
            else hi = mid;
        }
        const uint64_t first = lo;
        hi = a.n_pairs;
        while (lo < hi) {                                        // ... of a template > t
            const uint64_t mid = (lo + hi) >> 1;
            if (a.tmpl[mid] <= t) lo = mid + 1;
            else hi = mid;
        }
        a.lengths[r] += lo - first;
    }
}

// record r's header line ends right before its sequence line and starts after
// the '\n' before it (or at the buffer's start); without '>' (the headerless
// first record's line is empty) there is no name
__device__ __forceinline__ uint64_t dbf_name(const uint8_t *data, uint64_t len, const SeqLine *lines, uint64_t r,
                                             uint64_t *start) {
    const uint64_t st = lines[r].start;
    if (st == 0 || st > len) return 0;                           // (no line before it; never past the buffer)
    const uint64_t he = st - 1;                                  // the header's '\n'
    uint64_t b = he;
    while (b > 0 && data[b - 1] != '\n') --b;
    if (b == he || data[b] != '>') return 0;
    *start = b + 1;
    return he - (b + 1);
}

__global__ __launch_bounds__(256) void dbf_name_lens_kernel(const uint8_t *data, uint64_t len, const SeqLine *lines,
                                                            uint64_t n_rec, uint64_t *nlen) {
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t s = 0;
        nlen[r] = dbf_name(data, len, lines, r, &s);
    }
}

__global__ __launch_bounds__(256) void dbf_names_kernel(const uint8_t *data, const SeqLine *lines, uint64_t n_rec,
                                                        const uint64_t *noff, const uint64_t *nlen, uint8_t *out) {
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t n = nlen[r];
        if (!n) continue;
        const uint64_t s = lines[r].start - 1 - n;               // (dbf_name's start)
        for (uint64_t j = 0; j < n; ++j) out[noff[r] + j] = data[s + j];
    }
}

uint32_t dbf_grid(uint64_t n) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 65536)); }

}  // namespace

hipError_t launch_dbf_keys(const DbFasta &a, bool write, uint32_t n_cu, hipStream_t s) {
    if (a.m == 0) return hipSuccess;
    const uint64_t groups = (a.m + WALK_NS - 1) / WALK_NS;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((groups + 255) / 256, (uint64_t)std::max(n_cu, 1u) * 16);
    if (write) hipLaunchKernelGGL(dbf_keys_kernel<true>, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(dbf_keys_kernel<false>, dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_dbf_lengths(const DbFasta &a, hipStream_t s) {
    if (a.n == 0 || a.n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(dbf_lengths_kernel, dim3(dbf_grid(a.n)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_dbf_name_lens(const uint8_t *data, uint64_t len, const SeqLine *lines, uint64_t n_rec,
                                uint64_t *nlen, hipStream_t s) {
    if (n_rec == 0) return hipSuccess;
    hipLaunchKernelGGL(dbf_name_lens_kernel, dim3(dbf_grid(n_rec)), dim3(256), 0, s, data, len, lines, n_rec, nlen);
    return hipGetLastError();
}

hipError_t launch_dbf_names(const uint8_t *data, const SeqLine *lines, uint64_t n_rec, const uint64_t *noff,
                            const uint64_t *nlen, uint8_t *out, hipStream_t s) {
    if (n_rec == 0) return hipSuccess;
    hipLaunchKernelGGL(dbf_names_kernel, dim3(dbf_grid(n_rec)), dim3(256), 0, s, data, lines, n_rec, noff, nlen, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// host side: the gather over a context (kmer_db_open_fasta*, kmer_match.hip)
// ---------------------------------------------------------------------------
namespace {

constexpr uint64_t DBF_BATCH = 64ull << 20;      // bytes per upload of the host call (batch_bytes overrides)

// the call's own device arrays (the context lends the rewrite, the line finder and the sort scratch)
struct DbfBufs {
    hipStream_t s = nullptr;
    DBuf<uint8_t> in, nblob;
    DBuf<uint32_t> cnt, tmpl;
    DBuf<uint64_t> off, codes, lengths, nlen, noff;
    ~DbfBufs() {
        (void)hipStreamSynchronize(s);
        in.release(), nblob.release(), cnt.release(), tmpl.release();
        off.release(), codes.release(), lengths.release(), nlen.release(), noff.release();
    }
};

struct DbfHost {                                 // what the gather hands over, grown piece by piece
    std::vector<uint64_t> lengths, name_off{0};
    std::vector<char> names;
    uint64_t n = 0;                              // pairs gathered
    uint32_t nt = 0;                             // records so far
};

#define DBF_ENSURE(c, buf, n, ...)                                                                   \
    do {                                                                                             \
        if ((buf).ensure((n), (c)->stream, ##__VA_ARGS__) != hipSuccess) {                           \
            (void)hipGetLastError();                                                                 \
            return fail(c, KMER_E_OOM, "device allocation failed (DB from FASTA: " #buf ")");        \
        }                                                                                            \
    } while (0)

// One piece: len device-resident bytes of FASTA that start at a record start.
kmer_status dbf_piece(kmer_ctx *c, const uint8_t *d, uint64_t len, uint32_t flags, DbfBufs &B, DbfHost &H) {
    hipStream_t s = c->stream;
    const uint8_t *rd = nullptr;
    uint64_t rlen = 0;
    {
        const uint64_t nt64 = (len + TILE - 1) / TILE;
        DBF_ENSURE(c, c->fa_t, nt64 + 1);
        DBF_ENSURE(c, c->fa_x, nt64 + 1);
    }
    kmer_status st = fasta_rewrite(c, d, len, s, &rd, &rlen);
    if (st) return st;
    const uint64_t n_tiles64 = (rlen + TILE - 1) / TILE;
    if (n_tiles64 > 0x7FFFFFFFull) return fail(c, KMER_E_BAD_PARAM, "DB from FASTA: input too large for one piece");
    const uint32_t n_tiles = (uint32_t)n_tiles64;
    DBF_ENSURE(c, c->tcount, n_tiles);
    DBF_ENSURE(c, c->tbase, n_tiles);
    DBF_ENSURE(c, c->nlslots, (uint64_t)n_tiles * NL_SLOTS);
    c->host_lines = 0;                               // the line finder from line phase 0 (restored by the caller)
    uint64_t n_nl = 0, n_seq = 0;
    st = chunk_lines(c, rd, rlen, n_tiles, s, false, &n_nl, &n_seq);
    if (st == KMER_E_NONASCII) {                     // (reported, not kept: the context stays usable)
        const std::string msg = c->err;
        HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)c->d_err, (int)((uint32_t)c->h_small[5] & ~ERR_NONASCII), 1, s));
        HIPCHK(c, hipStreamSynchronize(s));
        return fail(c, st, msg);
    }
    if (st) return st;
    if (!n_seq) return KMER_OK;
    if ((uint64_t)H.nt + n_seq >= 0x7FFFFFFFull) return fail(c, KMER_E_BAD_PARAM, "kmer_db_open: too many templates");
    // names
    DBF_ENSURE(c, B.nlen, n_seq);
    DBF_ENSURE(c, B.noff, n_seq);
    HIPCHK(c, launch_dbf_name_lens(rd, rlen, c->lines.p, n_seq, B.nlen.p, s));
    ROCPRIM_RUN(c, rocprim::exclusive_scan(t, b, B.nlen.p, B.noff.p, (uint64_t)0, (size_t)n_seq,
                                           rocprim::plus<uint64_t>(), s));
    // windows of all records
    DBF_ENSURE(c, c->wbase, n_seq);
    ROCPRIM_RUN(c, rocprim::exclusive_scan(t, b, c->wcount.p, c->wbase.p, (uint64_t)0, (size_t)n_seq,
                                           rocprim::plus<uint64_t>(), s));
    uint64_t tail[4] = {0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(&tail[0], c->wbase.p + n_seq - 1, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&tail[1], c->wcount.p + n_seq - 1, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&tail[2], B.noff.p + n_seq - 1, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&tail[3], B.nlen.p + n_seq - 1, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const uint64_t total = (tail[0] + tail[1]) / 2;  // (wcount: both strands' windows)
    const uint64_t nbytes = tail[2] + tail[3];
    {
        std::vector<uint64_t> off(n_seq);
        const size_t nb0 = H.names.size();
        H.names.resize(nb0 + nbytes);
        if (nbytes) {
            DBF_ENSURE(c, B.nblob, nbytes);
            HIPCHK(c, launch_dbf_names(rd, c->lines.p, n_seq, B.noff.p, B.nlen.p, B.nblob.p, s));
            HIPCHK(c, hipMemcpyAsync(H.names.data() + nb0, B.nblob.p, nbytes, hipMemcpyDeviceToHost, s));
        }
        HIPCHK(c, hipMemcpyAsync(off.data(), B.noff.p, n_seq * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        for (uint64_t r = 1; r < n_seq; ++r) H.name_off.push_back(nb0 + off[r]);
        H.name_off.push_back(nb0 + nbytes);
    }
    DBF_ENSURE(c, B.lengths, n_seq);
    HIPCHK(c, hipMemsetAsync(B.lengths.p, 0, n_seq * 8, s));
    DbFasta a;
    memset(&a, 0, sizeof(a));
    a.data = rd;
    a.len = rlen;
    a.lines = c->lines.p;
    a.wbase2 = c->wbase.p;
    a.n = n_seq;
    a.total = total;
    a.k = c->p.k;
    for (size_t i = 0; i < c->prefix.size(); ++i) {  // (the planes of view_key_params, kmer_api.hip)
        const uint8_t ch = (uint8_t)c->prefix[i];
        a.plo |= ((((uint32_t)ch >> 1) ^ ((uint32_t)ch >> 2)) & 1u) << i;
        a.phi |= (((uint32_t)ch >> 2) & 1u) << i;
    }
    a.pmask = c->prefix.size() >= 32 ? ~0u : ((1u << c->prefix.size()) - 1u);
    a.canonical = (c->p.flags & KMER_FLAG_CANONICAL) ? 1u : 0u;
    a.t0 = H.nt;
    a.lengths = B.lengths.p;
    // a prefix that no A/C/G/T window can start with: no keys (its planes would stand for other bytes)
    bool possible = c->prefix.size() <= c->p.k;
    for (char ch : c->prefix) possible = possible && (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T');
    const uint32_t cus = (uint32_t)std::max(c->n_cu, 1);
    const uint64_t piece = (flags & 1u) ? DBF_PIECE_TEST : DBF_PIECE;
    for (uint64_t p0 = 0; possible && p0 < total; p0 += piece) {
        a.p0 = p0;
        a.m = std::min(piece, total - p0);
        const uint64_t groups = (a.m + WALK_NS - 1) / WALK_NS;
        DBF_ENSURE(c, B.cnt, groups);
        DBF_ENSURE(c, B.off, groups);
        a.cnt = B.cnt.p;
        a.off = B.off.p;
        HIPCHK(c, launch_dbf_keys(a, false, cus, s));
        ROCPRIM_RUN(c, rocprim::exclusive_scan(t, b, B.cnt.p, B.off.p, (uint64_t)0, (size_t)groups,
                                               rocprim::plus<uint64_t>(), s));
        uint64_t lo = 0;
        uint32_t lc = 0;
        HIPCHK(c, hipMemcpyAsync(&lo, B.off.p + groups - 1, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(&lc, B.cnt.p + groups - 1, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        a.n_pairs = lo + lc;
        if (!a.n_pairs) continue;
        if (H.n + a.n_pairs >= 0xFFFFFFFFull) return fail(c, KMER_E_BAD_PARAM, "kmer_db_open: more than 2^32 - 2 k-mers");
        DBF_ENSURE(c, B.codes, H.n + a.n_pairs, true, H.n);
        DBF_ENSURE(c, B.tmpl, H.n + a.n_pairs, true, H.n);
        a.codes = B.codes.p + H.n;
        a.tmpl = B.tmpl.p + H.n;
        HIPCHK(c, launch_dbf_keys(a, true, cus, s));
        HIPCHK(c, launch_dbf_lengths(a, s));
        H.n += a.n_pairs;
    }
    const size_t l0 = H.lengths.size();
    H.lengths.resize(l0 + n_seq);
    HIPCHK(c, hipMemcpyAsync(H.lengths.data() + l0, B.lengths.p, n_seq * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    H.nt += (uint32_t)n_seq;
    return KMER_OK;
}

kmer_status dbf_run(kmer_ctx *c, const uint8_t *bytes, uint64_t len, bool on_device, uint32_t flags, void *stream,
                    DbfBufs &B, DbfHost &H) {
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, KMER_E_DEVICE, "hipSetDevice failed");
    hipStream_t s = c->stream;
    if (on_device) {
        HIPCHK(c, hipEventRecord(c->evw, (hipStream_t)stream));
        HIPCHK(c, hipStreamWaitEvent(s, c->evw, 0));
        return dbf_piece(c, bytes, len, flags, B, H);
    }
    const uint64_t batch = c->p.batch_bytes ? c->p.batch_bytes : DBF_BATCH;
    for (uint64_t pos = 0; pos < len;) {
        // the piece: whole records (cut before a header line), as many as fit the batch, at least one
        uint64_t end = std::min(len, pos + batch);
        if (end < len) {
            const uint64_t cut = batch_cut(bytes + pos, end - pos, true);
            end = cut ? pos + cut : batch_extend(bytes, end, len, true);
        }
        const uint64_t m = end - pos;
        DBF_ENSURE(c, B.in, m);
        kmer_status st = upload(c, B.in.p, bytes + pos, m, s);
        if (st) return st;
        st = dbf_piece(c, B.in.p, m, flags, B, H);
        if (st) return st;
        pos = end;
    }
    return KMER_OK;
}

}  // namespace

int dbfasta_check(kmer_ctx *c) {
    if (c->p.k == 0 || c->p.k > 32) return (int)fail(c, KMER_E_BAD_PARAM, "DB from FASTA: k must be 1..32");
    if (c->p.step != 1) return (int)fail(c, KMER_E_BAD_PARAM, "DB from FASTA: step must be 1");
    if (!c->group.empty()) return (int)fail(c, KMER_E_STATE, "single-device call on a group context");
    if (c->open_stream && c->session_fed)
        return (int)fail(c, KMER_E_STATE, "DB from FASTA: the session has fed chunks and is not finished");
    return KMER_OK;
}

int dbfasta_gather(kmer_ctx *c, const uint8_t *bytes, uint64_t len, bool on_device, uint32_t flags, void *stream,
                   DbFastaPairs *out) {
    memset(out, 0, sizeof(*out));
    kmer_status st = (kmer_status)dbfasta_check(c);
    if (st) return (int)st;
    out->device = c->device;
    out->k = c->p.k;
    if (len == 0) return KMER_OK;
    st = settle(c);                                  // a chunk in flight
    if (st) return (int)st;
    // what the rewrite and the line finder count for a session stays the session's
    const uint64_t saved_lines = c->host_lines, saved_fa = c->fa_lines;
    const double saved_ms = c->t_ms[6];
    DbfHost H;
    {
        DbfBufs B;
        B.s = c->stream;
        st = dbf_run(c, bytes, len, on_device, flags, stream, B, H);
        c->host_lines = saved_lines;
        c->fa_lines = saved_fa;
        c->t_ms[6] = saved_ms;
        if (st == KMER_OK && hipStreamSynchronize(c->stream) != hipSuccess)
            st = fail(c, KMER_E_DEVICE, "DB from FASTA: the stream failed");
        if (st) return (int)st;                      // (B frees everything)
        out->codes = B.codes.p;                      // handed over: the caller frees them
        out->tmpl = B.tmpl.p;
        out->cap = B.codes.cap;
        B.codes.p = nullptr, B.codes.cap = 0;
        B.tmpl.p = nullptr, B.tmpl.cap = 0;
    }
    out->n = H.n;
    out->nt = H.nt;
    out->lengths = (uint64_t *)malloc(std::max<size_t>(H.lengths.size(), 1) * 8);
    out->name_off = (uint64_t *)malloc(H.name_off.size() * 8);
    out->names = (char *)malloc(std::max<size_t>(H.names.size(), 1));
    if (!out->lengths || !out->name_off || !out->names) {
        dbfasta_release(out);
        return (int)fail(c, KMER_E_OOM, "DB from FASTA: host allocation failed");
    }
    if (!H.lengths.empty()) memcpy(out->lengths, H.lengths.data(), H.lengths.size() * 8);
    memcpy(out->name_off, H.name_off.data(), H.name_off.size() * 8);
    if (!H.names.empty()) memcpy(out->names, H.names.data(), H.names.size());
    return KMER_OK;
}

void dbfasta_release(DbFastaPairs *p) {
    if (p->codes) (void)hipFree(p->codes);
    if (p->tmpl) (void)hipFree(p->tmpl);
    free(p->lengths);
    free(p->names);
    free(p->name_off);
    memset(p, 0, sizeof(*p));
}

}  // namespace kmerhip
