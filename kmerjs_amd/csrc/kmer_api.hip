// kmer_api.hip — the C-ABI entry points (include/kmer_api.h): context
// lifecycle, device-resident feeds, multi-GPU exchange, results, table queries.
// The machinery behind them: kmer_host.hpp.
#include "kmer_host.hpp"

using namespace kmerhip;

extern "C" {

const char *kmer_version(void) { return "kmerhip 0.2 (gfx950)"; }

const char *kmer_status_string(kmer_status s) {
    switch (s) {
    case KMER_OK: return "ok";
    case KMER_E_IO: return "i/o error";
    case KMER_E_BAD_PARAM: return "bad parameter";
    case KMER_E_OOM: return "out of memory";
    case KMER_E_DEVICE: return "device error";
    case KMER_E_TOO_MANY_KEYS: return "too many keys";
    case KMER_E_NONASCII: return "non-ASCII input";
    case KMER_E_LINE_TOO_LONG: return "line too long";
    case KMER_E_STATE: return "bad call sequence";
    }
    return "unknown";
}

const char *kmer_last_error(const kmer_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

kmer_status kmer_open(const kmer_params *pp, kmer_ctx **out) {
    if (!pp || !out) return KMER_E_BAD_PARAM;
    if (pp->k == 0 || pp->step == 0 || (pp->prefix_len && !pp->prefix)) return KMER_E_BAD_PARAM;
    if (pp->flags & ~KMER_FLAGS_PUBLIC) return KMER_E_BAD_PARAM;   // reserved flag bits
    *out = nullptr;
    if (pp->ndev > 1) {
        if (pp->ndev > 64) return KMER_E_BAD_PARAM;
        kmer_ctx *g = new (std::nothrow) kmer_ctx();
        if (!g) return KMER_E_OOM;
        g->p = *pp;
        g->p.prefix = nullptr;
        g->p.devices = nullptr;
        g->prefix.assign((const char *)pp->prefix, pp->prefix_len);
        for (uint32_t i = 0; i < pp->ndev; ++i) {
            kmer_params cp = *pp;
            cp.ndev = 1;
            cp.devices = nullptr;
            cp.device = pp->devices ? pp->devices[i] : (int32_t)i;
            kmer_ctx *c = nullptr;
            const kmer_status st = kmer_open(&cp, &c);
            if (st) {
                kmer_close(g);
                return st;
            }
            g->group.push_back(c);
        }
        // peer access between every pair of distinct devices, so the group's
        // partial / key copies (hipMemcpyPeerAsync, kmer_group.hip) go device to
        // device over xGMI.  A pair the platform refuses (no P2P path) keeps
        // working: the runtime stages such peer copies through host memory.
        for (kmer_ctx *a : g->group)
            for (kmer_ctx *b : g->group) {
                if (a->device == b->device) continue;
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, a->device, b->device) != hipSuccess) can = 0;
                hipError_t e = hipErrorPeerAccessUnsupported;
                if (can && hipSetDevice(a->device) == hipSuccess) {
                    e = hipDeviceEnablePeerAccess(b->device, 0);
                    if (e == hipErrorPeerAccessAlreadyEnabled) {
                        (void)hipGetLastError();   // (enabled by an earlier group: fine)
                        e = hipSuccess;
                    }
                }
                if (e != hipSuccess) (void)hipGetLastError();
            }
        g->device = g->group[0]->device;
        g->mode = g->group[0]->mode;
        (void)hipSetDevice(g->device);
        *out = g;
        return KMER_OK;
    }
    kmer_ctx *c = new (std::nothrow) kmer_ctx();
    if (!c) return KMER_E_OOM;
    c->p = *pp;
    c->fasta = (pp->flags & KMER_FLAG_FASTA) != 0;
    c->prefix.assign((const char *)pp->prefix, pp->prefix_len);
    c->rprefix.resize(c->prefix.size());
    for (size_t i = 0; i < c->prefix.size(); ++i)
        c->rprefix[c->prefix.size() - 1 - i] = (char)comp((uint8_t)c->prefix[i]);
    c->p.prefix = nullptr;
    for (unsigned char ch : c->prefix)
        if (ch >= 0x80) {
            delete c;
            return KMER_E_NONASCII;
        }
    c->device = pp->device;
    auto cleanup = [&](kmer_status s) {
        kmer_close(c);
        return s;
    };
    if (hipSetDevice(c->device) != hipSuccess) return cleanup(KMER_E_DEVICE);
    if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess) c->n_cu = 256;
    {
        // the session's one stream, at the device's highest priority
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = hi = 0;
        if (hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, hi) != hipSuccess)
            return cleanup(KMER_E_DEVICE);
    }

    c->pbits = (pp->flags & KMER_FLAG_LONG_LINES) ? PBITS_LONG : PBITS_DEFAULT;
    const uint32_t k = pp->k, plen = (uint32_t)c->prefix.size();
    bool acgt = plen > 0;
    for (char ch : c->prefix) acgt &= ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T';
    const bool dense_ok = !(pp->flags & KMER_FLAG_NO_DENSE) && pp->step == 1 && plen <= k;
    const bool win_step = !(pp->flags & KMER_FLAG_NO_DENSE) && pp->step > 1 && plen <= k &&
                          (plen == 0 ? k <= 31 : (acgt && k <= (uint32_t)KMAX_DENSE));
    if ((pp->flags & KMER_FLAG_CANONICAL) &&
        !(pp->step == 1 && plen <= k && k <= (uint32_t)KMAX_PACKED && (plen == 0 || acgt))) {
        delete c;                               // (canonical counts exist in table mode only)
        return KMER_E_BAD_PARAM;
    }
    if ((pp->flags & (KMER_FLAG_UNORDERED | KMER_FLAG_CANONICAL)) && pp->step == 1 && plen <= k &&
        k <= (uint32_t)KMAX_PACKED && (plen == 0 || acgt))
        c->mode = MODE_TABLE;
    else if (dense_ok && (plen == 0 ? k <= 31 : (acgt && plen <= 3 && k <= (uint32_t)KMAX_TILE)))
        c->mode = MODE_WINDOWS;                 // (a 1-3-base prefix hits densely: kmer_dense.hip, k <= 64)
    else if (win_step)
        c->mode = MODE_WINDOWS;                 // step > 1: every stepped window ranked (the tile scan has no line ends)
    else if (dense_ok && plen > 0 && k <= (uint32_t)KMAX_TILE)
        c->mode = MODE_PACKED;                  // (k > 32: 128-bit window codes; any prefix bytes: key = P + suffix code)
    else if (pp->step == 1 && plen > 0 && k <= (uint32_t)KMAX_TILE)
        c->mode = MODE_TILE_REC;
    else
        c->mode = MODE_GENERAL;
    // general path with step 1: every record is a k-byte key, merged on the
    // device (KMER_FLAG_NO_DENSE keeps the host record merge, for the tests)
    c->gm_on = c->mode == MODE_GENERAL && pp->step == 1 && !(pp->flags & KMER_FLAG_NO_DENSE);
    const bool packed_keys = c->mode == MODE_PACKED || c->mode == MODE_WINDOWS;
    c->kbits = packed_keys ? 2 * (k - plen) : 0;
    c->narrow = packed_keys && c->kbits <= 31;
    c->wide = packed_keys && c->kbits >= 64;
    c->planes = (c->mode == MODE_PACKED || c->mode == MODE_TILE_REC) && acgt && !(pp->flags & KMER_FLAG_BYTE_SCAN);
    c->gen_planes = c->gm_on && acgt && !(pp->flags & KMER_FLAG_BYTE_SCAN);
    if (c->planes || c->gen_planes) {
        // plane bits of a base: bit 1 (plane L) and bit 2 (plane H) of its ASCII byte
        auto code = [](char ch) -> uint32_t { return (((uint8_t)ch >> 1) & 1u) | ((((uint8_t)ch >> 2) & 1u) << 1); };
        c->pargs.pb = std::min<uint32_t>(plen, 5);
        for (uint32_t i = 0; i < 5; ++i) {
            const uint32_t cp = i < plen ? code(c->prefix[i]) : 0u, cr = i < plen ? code(c->rprefix[i]) : 0u;
            c->pargs.kl[i] = (cp & 1u) ? 0u : ~0u;
            c->pargs.kh[i] = (cp & 2u) ? 0u : ~0u;
            c->pargs.rl[i] = (cr & 1u) ? 0u : ~0u;
            c->pargs.rh[i] = (cr & 2u) ? 0u : ~0u;
        }
    }

    bool ok = true;
    ok &= dalloc(&c->d_P, std::max<uint32_t>(plen, 1)) == hipSuccess;
    if (ok && plen) ok &= hipMemcpy(c->d_P, c->prefix.data(), plen, hipMemcpyHostToDevice) == hipSuccess;
    {
        // [0,64) P and [64,128) rc(P) (tile kernel, truncated), [128, 128+|P|) full P,
        // [128+|P|, 128+2|P|) full rc(P) (general kernels)
        std::vector<uint8_t> pr(2 * KMAX_TILE + 2 * c->prefix.size(), 0);
        memcpy(pr.data(), c->prefix.data(), std::min<size_t>(c->prefix.size(), KMAX_TILE));
        memcpy(pr.data() + KMAX_TILE, c->rprefix.data(), std::min<size_t>(c->rprefix.size(), KMAX_TILE));
        memcpy(pr.data() + 2 * KMAX_TILE, c->prefix.data(), c->prefix.size());
        memcpy(pr.data() + 2 * KMAX_TILE + c->prefix.size(), c->rprefix.data(), c->rprefix.size());
        ok &= dalloc(&c->d_PR, pr.size()) == hipSuccess;
        if (ok) ok &= hipMemcpy(c->d_PR, pr.data(), pr.size(), hipMemcpyHostToDevice) == hipSuccess;
    }
    ok &= dalloc(&c->d_ticket, 4) == hipSuccess;
    ok &= dalloc(&c->d_bticket, 1) == hipSuccess;
    if (ok) ok &= hipMemset(c->d_bticket, 0, sizeof(unsigned int)) == hipSuccess;
    ok &= dalloc(&c->d_scal, 16) == hipSuccess;
    if (ok) {
        ok &= hipMemset(c->d_scal, 0, 128) == hipSuccess;
        c->d_hticket = (unsigned int *)(c->d_scal + 8);
        c->d_cross_go = (unsigned int *)(c->d_scal + 9);
        c->d_rec_count = (unsigned long long *)(c->d_scal + 0);
        c->d_ovf_count = (unsigned long long *)(c->d_scal + 1);
        c->d_xcount = (unsigned long long *)(c->d_scal + 2);
        c->d_chunk_hits = (unsigned long long *)(c->d_scal + 3);
        c->d_nuniq = c->d_scal + 4;
        c->d_err = (unsigned int *)(c->d_scal + 5);
        c->d_line_count = (unsigned long long *)(c->d_scal + 6);
        c->d_ends_open = (unsigned long long *)(c->d_scal + 7);
    }
    ok &= dalloc(&c->d_stamp, STAMP_WORDS) == hipSuccess;
    if (ok) ok &= hipMemset(c->d_stamp, 0, STAMP_WORDS * sizeof(uint64_t)) == hipSuccess;
    {
        int khz = 0;
        ok &= hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) == hipSuccess && khz > 0;
        c->clock_khz = khz;
    }
    ok &= dalloc(&c->d_pos, 1) == hipSuccess;
    ok &= dalloc(&c->d_pos_saved, 1) == hipSuccess;
    ok &= hipHostMalloc((void **)&c->h_small, 24 * sizeof(uint64_t), hipHostMallocDefault) == hipSuccess;
    ok &= hipHostMalloc((void **)&c->h_tail, TAIL_WORDS * sizeof(uint64_t), hipHostMallocMapped | hipHostMallocCoherent) ==
          hipSuccess;
    ok &= c->h_tail && hipHostGetDevicePointer((void **)&c->d_tail, c->h_tail, 0) == hipSuccess;
    if (c->h_tail) memset(c->h_tail, 0, TAIL_WORDS * sizeof(uint64_t));
    for (hipEvent_t &e : c->tev) ok &= hipEventCreate(&e) == hipSuccess;
    for (hipEvent_t &e : c->fa_ev) ok &= hipEventCreate(&e) == hipSuccess;
    ok &= hipEventCreate(&c->ev0) == hipSuccess && hipEventCreate(&c->ev1) == hipSuccess &&
          hipEventCreate(&c->ev2) == hipSuccess && hipEventCreate(&c->ev3) == hipSuccess &&
          hipEventCreateWithFlags(&c->evw, hipEventDisableTiming) == hipSuccess;
    if (!ok) return cleanup(KMER_E_OOM);
    if (ensure_records(c, 1 << 16) || ensure_tiles(c, 1 << 12)) return cleanup(KMER_E_OOM);
    if (ensure_ovf(c, 1 << 16, c->stream) != KMER_OK) return cleanup(KMER_E_OOM);
    if (hipMemset(c->d_err, 0, 4) != hipSuccess) return cleanup(KMER_E_DEVICE);
    if (reset(c) != KMER_OK) return cleanup(KMER_E_DEVICE);
    c->open_stream = false;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return cleanup(KMER_E_DEVICE);
    *out = c;
    return KMER_OK;
}

kmer_status kmer_close(kmer_ctx *c) {
    if (!c) return KMER_E_BAD_PARAM;
    if (!c->group.empty()) {
        if (hipSetDevice(c->group[0]->device) == hipSuccess) {
            c->gkeys.release();
            c->gvals.release();
            c->gkeys2.release();
            c->gvals2.release();
        }
        for (kmer_ctx *x : c->group) kmer_close(x);
        delete c;
        return KMER_OK;
    }
    (void)hipSetDevice(c->device);
    (void)settle(c);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->tcount.release();
    c->nlslots.release();
    c->fa_t.release();
    c->fa_x.release();
    c->fa_out[0].release();
    c->fa_out[1].release();
    for (auto *b : {&c->tbase, &c->nlpos, &c->wcount, &c->wbase, &c->tp_cnt, &c->tp_lnl, &c->rkey, &c->rkey2, &c->rord, &c->rord2, &c->csel, &c->rcnt, &c->xord, &c->xord2,
                    &c->xkey, &c->xkey2, &c->ukey, &c->first, &c->cnt_out})
        b->release();
    for (auto *b : {&c->ridx, &c->ridx2, &c->ecnt, &c->bbase, &c->xslot, &c->rkey32, &c->rkey32b, &c->bH, &c->bHs}) b->release();
    c->pkey16.release();
    c->bcur.release();
    c->xsend.release();
    c->xH.release();
    c->xHs.release();
    c->xcnt.release();
    if (c->h_xcnt) (void)hipHostFree(c->h_xcnt);
    c->bsum.release();
    c->bscan.release();
    c->hrec.release();
    c->hcnt.release();
    c->hmark.release();
    c->tsum.release();
    c->tscan.release();
    c->hits.release();
    c->ovf.release();
    c->lb_cnt.release();
    c->lb_lnl.release();
    c->uval.release();
    c->keys_out.release();
    c->recs.release();
    c->gcand.release();
    c->cpcnt.release();
    c->cpoff.release();
    c->lines.release();
    c->rec_keys.release();
    c->tmp.release();
    c->batch.release();
    for (auto *b : {&c->tb1, &c->tb2, &c->tHs, &c->tstart, &c->tp1, &c->tpb, &c->tsend}) b->release();
    c->tspc.release();
    c->tseg.release();
    c->tpc.release();
    c->tpieces.release();
    c->tH.release();
    c->tnd.release();
    c->epre.release();
    c->tunits.release();
    c->tbig.release();
    c->tstats.release();
    c->tleft.release();
    c->trecv.release();
    c->tlk_keys.release();
    c->tlk_cnt.release();
    c->tlk_bad.release();
    c->tab_hist.release();
    for (auto *b : {&c->tex_code, &c->tex_code2, &c->tex_val, &c->tex_val2}) b->release();
    c->tex_keys.release();
    c->tjoin.release();
    for (auto *b : {&c->tsc_h, &c->tsc_val}) b->release();
    for (auto *b : {&c->tsc_bkt, &c->tsc_bkt2, &c->tsc_idx, &c->tsc_idx2}) b->release();
    c->tsc_code.release();
    c->tsc_rows.release();
    c->tsc_in.release();
    for (auto *b : {&c->tfl_rend, &c->tfl_seg_src, &c->tfl_seg_out}) b->release();
    c->tfl_keep.release();
    c->tfl_scan.release();
    c->tfl_out.release();
    c->gm_keys.release();
    c->gm_keys2.release();
    for (auto *b : {&c->gm_cnt, &c->gm_cnt2, &c->gm_first, &c->gm_first2, &c->gm_h1, &c->gm_h2, &c->gm_h1b, &c->gm_h2b})
        b->release();
    for (auto *b : {&c->gm_idx, &c->gm_idx2, &c->gm_head, &c->gm_gid, &c->gm_start}) b->release();
    c->gm_flag.release();
    dfree(c->d_ticket); dfree(c->d_bticket); dfree(c->d_scal); dfree(c->d_pos); dfree(c->d_pos_saved);
    dfree(c->d_P); dfree(c->d_PR); dfree(c->d_stamp);
    if (c->h_small) (void)hipHostFree(c->h_small);
    if (c->h_tail) (void)hipHostFree(c->h_tail);
    for (hipStream_t us : c->up_streams) (void)hipStreamSynchronize(us);
    if (c->up_p) (void)hipHostFree(c->up_p);
    for (hipEvent_t e : {c->ev0, c->ev1, c->ev2, c->ev3, c->evw})
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->tev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->fa_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return KMER_OK;
}

kmer_status kmer_sync(kmer_ctx *c) {
    if (!c) return KMER_E_BAD_PARAM;
    if (!c->group.empty()) return fail(c, KMER_E_STATE, "single-device call on a group context");
    if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
    return settle(c);
}

kmer_status kmer_reset(kmer_ctx *c) {
    if (!c) return KMER_E_BAD_PARAM;
    if (!c->group.empty()) return fail(c, KMER_E_STATE, "single-device call on a group context");
    if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
    return reset(c);
}

kmer_status kmer_feed_device(kmer_ctx *c, const void *d_bytes, size_t len, void *stream) {
    if (!c || (!d_bytes && len)) return KMER_E_BAD_PARAM;
    SETTLE(c);
    if (!c->open_stream) return fail(c, KMER_E_STATE, "feed without reset");
    if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    if (s != c->stream) {
        // order the context's own (non-blocking) stream after the caller's
        // work; NULL is the legacy default stream, which a non-blocking stream
        // does not otherwise wait for
        HIPCHK(c, hipEventRecord(c->evw, s));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->evw, 0));
    }
    return feed(c, (const uint8_t *)d_bytes, len, c->stream);
}

kmer_status kmer_finish_device(kmer_ctx *c, kmer_result **out) {
    if (!c) return KMER_E_BAD_PARAM;
    SETTLE(c);
    if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
    if (out) *out = nullptr;
    return finish(c, out);
}


kmer_status kmer_partial_device(kmer_ctx *c, const void **d_keys, const void **d_vals, uint64_t *n) {
    if (!c || !d_keys || !d_vals || !n) return KMER_E_BAD_PARAM;
    SETTLE(c);
    if (c->mode != MODE_PACKED && c->mode != MODE_WINDOWS)
        return fail(c, KMER_E_STATE, "configuration has no packed keys");
    if (c->wide) return fail(c, KMER_E_STATE, "keys of 64 bits or more (k - |P| >= 32) have no packed partials");
    if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
    kmer_status st = apply_cross(c);
    if (st) return st;
    uint64_t nu = 0;
    st = rank_finish(c, c->n_hits, true, false, &nu);
    if (st) return st;
    c->n_hits = 0;           // the rank arrays were consumed by the sort
    *d_keys = c->ukey.p;
    *d_vals = c->uval.p;
    *n = nu;
    return KMER_OK;
}

kmer_status kmer_finish_merged(kmer_ctx *c, const void *d_keys, const void *d_vals, uint64_t n,
                               uint64_t total_lines, kmer_result **out) {
    if (!c || (n && (!d_keys || !d_vals))) return KMER_E_BAD_PARAM;
    SETTLE(c);
    if (c->mode != MODE_PACKED && c->mode != MODE_WINDOWS)
        return fail(c, KMER_E_STATE, "configuration has no packed keys");
    if (c->wide) return fail(c, KMER_E_STATE, "keys of 64 bits or more (k - |P| >= 32) have no packed partials");
    if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
    if (out) *out = nullptr;
    hipStream_t s = c->stream;
    HIPCHK(c, hipEventRecord(c->ev2, s));
    // the partials, concatenated in shard order, are already in first-occurrence
    // order: their index is their rank
    kmer_status st = ensure_rank_arrays(c, n, 0, s);
    if (st) return st;
    HIPCHK(c, c->rcnt.ensure(n, s));
    HIPCHK(c, launch_merge_prep((const uint64_t *)d_keys, (const Agg *)d_vals, n, c->rkey.p,
                                c->narrow ? c->rkey32.p : nullptr, c->rord.p, c->rcnt.p, c->ridx.p, s));
    uint64_t nu = 0;
    const bool sync = out || c->p.max_keys;
    st = rank_finish(c, n, false, true, &nu, sync);
    if (st) return st;
    c->n_out = nu;
    HIPCHK(c, hipEventRecord(c->ev3, s));
    c->timing_pending = true;
    c->n_hits = 0;
    c->n_cross = 0;
    c->open_stream = false;
    if (!sync) return KMER_OK;
    st = resolve_out(c);
    if (st) return st;
    const uint64_t total = c->n_out + c->exotic.size();
    if (c->p.max_keys && total > c->p.max_keys)
        return fail(c, KMER_E_TOO_MANY_KEYS, "more distinct keys than max_keys (reference Map limit)");
    if (!out) return KMER_OK;
    return build_result(c, total_lines, out);
}

// One ordered result from the ranks' ordered key ranges (after
// kmer_finish_exchanged), gathered to one device: a stable radix sort of the
// first-occurrence keys (each list is sorted; their union is re-ordered),
// then keys / counts / firsts permuted into the context's result arrays.
kmer_status kmer_merge_ordered(kmer_ctx *c, const void *d_keys, const void *d_counts, const void *d_firsts,
                               uint64_t n, uint64_t total_lines, kmer_result **out) {
    if (!c || (n && (!d_keys || !d_counts || !d_firsts))) return KMER_E_BAD_PARAM;
    SETTLE(c);
    if (c->mode != MODE_PACKED && c->mode != MODE_WINDOWS)
        return fail(c, KMER_E_STATE, "configuration has no packed keys");
    if (n >= (1ull << 32)) return fail(c, KMER_E_TOO_MANY_KEYS, "more than 2^32 entries to merge");
    if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
    if (out) *out = nullptr;
    hipStream_t s = c->stream;
    HIPCHK(c, hipEventRecord(c->ev2, s));
    const uint64_t k = c->p.k;
    if (n) {
        HIPCHK(c, c->xord.ensure(n, s));
        HIPCHK(c, c->xord2.ensure(n, s));
        HIPCHK(c, c->ridx.ensure(n, s));
        HIPCHK(c, c->ridx2.ensure(n, s));
        HIPCHK(c, c->keys_out.ensure(n * k, s));
        HIPCHK(c, c->cnt_out.ensure(n, s));
        HIPCHK(c, c->first.ensure(n, s));
        HIPCHK(c, hipMemcpyAsync(c->xord.p, d_firsts, n * 8, hipMemcpyDeviceToDevice, s));
        rocprim::counting_iterator<uint32_t> iota(0u);
        ROCPRIM_RUN(c, rocprim::radix_sort_pairs(t, b, c->xord.p, c->xord2.p, iota, c->ridx2.p, (size_t)n, 0, 64, s));
        HIPCHK(c, launch_permute_rows((const uint8_t *)d_keys, (const uint64_t *)d_counts, (const uint64_t *)d_firsts,
                                      c->ridx2.p, n, (uint32_t)k, c->keys_out.p, c->cnt_out.p, c->first.p, s));
    }
    c->n_out = n;
    c->out_pending = false;
    HIPCHK(c, hipEventRecord(c->ev3, s));
    c->timing_pending = true;
    c->open_stream = false;
    const bool sync = out || c->p.max_keys;
    if (!sync) return KMER_OK;
    kmer_status st = resolve_out(c);
    if (st) return st;
    const uint64_t total = c->n_out + c->exotic.size();
    if (c->p.max_keys && total > c->p.max_keys)
        return fail(c, KMER_E_TOO_MANY_KEYS, "more distinct keys than max_keys (reference Map limit)");
    if (!out) return KMER_OK;
    return build_result(c, total_lines, out);
}

kmer_status kmer_exchange_prepare(kmer_ctx *c, uint32_t world, const void **d_send, uint64_t *counts) {
    if (!c || !d_send || !counts || world == 0 || world > XP_MAXW) return KMER_E_BAD_PARAM;
    SETTLE(c);
    if (c->mode != MODE_PACKED && c->mode != MODE_WINDOWS)
        return fail(c, KMER_E_STATE, "configuration has no packed keys");
    if (c->wide) return fail(c, KMER_E_STATE, "keys of 64 bits or more (k - |P| >= 32) have no packed partials");
    if (!c->open_stream) return fail(c, KMER_E_STATE, "exchange without reset/feed");
    if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
    hipStream_t s = c->stream;
    kmer_status st = apply_cross(c);
    if (st) return st;
    const uint64_t n = c->n_hits;
    *d_send = nullptr;
    for (uint32_t o = 0; o < world; ++o) counts[o] = 0;
    c->n_hits = 0;           // the rank arrays are handed over (finish_exchanged refills them)
    if (n == 0) return KMER_OK;
    const uint64_t nblk64 = (n + XP_EPB_HOST - 1) / XP_EPB_HOST;
    if ((uint64_t)world * nblk64 >= (1ull << 31)) return fail(c, KMER_E_BAD_PARAM, "too many hits to partition");
    const uint32_t nblk = (uint32_t)nblk64;
    const uint64_t invalid = c->kbits >= 63 ? ~0ull : (1ull << c->kbits);
    HIPCHK(c, c->xsend.ensure(n, s));
    HIPCHK(c, c->xH.ensure((uint64_t)world * nblk, s));
    HIPCHK(c, c->xHs.ensure((uint64_t)world * nblk, s));
    HIPCHK(c, c->xcnt.ensure(world, s));
    if (!c->h_xcnt) HIPCHK(c, hipHostMalloc((void **)&c->h_xcnt, XP_MAXW * sizeof(uint64_t), hipHostMallocDefault));
    const uint64_t *rk = c->narrow ? nullptr : c->rkey.p;
    const uint32_t *rk32 = c->narrow ? c->rkey32.p : nullptr;
    HIPCHK(c, launch_xpart_hist(rk, rk32, n, invalid, c->kbits, world, nblk, c->xH.p, s));
    ROCPRIM_RUN(c, rocprim::exclusive_scan(t, b, c->xH.p, c->xHs.p, 0u, (size_t)world * nblk,
                                           rocprim::plus<uint32_t>(), s));
    HIPCHK(c, launch_xpart_scatter(rk, rk32, c->rord.p, n, invalid, c->kbits, world, nblk, c->xH.p, c->xHs.p,
                                   c->xsend.p, c->xcnt.p, s));
    HIPCHK(c, hipMemcpyAsync(c->h_xcnt, c->xcnt.p, world * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    for (uint32_t o = 0; o < world; ++o) counts[o] = c->h_xcnt[o];
    *d_send = c->xsend.p;
    return KMER_OK;
}

kmer_status kmer_finish_exchanged(kmer_ctx *c, const void *d_recv, uint64_t n, uint64_t total_lines,
                                  void *wait_stream, kmer_result **out) {
    if (!c || (n && !d_recv)) return KMER_E_BAD_PARAM;
    SETTLE(c);
    if (c->mode != MODE_PACKED && c->mode != MODE_WINDOWS)
        return fail(c, KMER_E_STATE, "configuration has no packed keys");
    if (c->wide) return fail(c, KMER_E_STATE, "keys of 64 bits or more (k - |P| >= 32) have no packed partials");
    if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
    if (out) *out = nullptr;
    hipStream_t s = c->stream;
    // the received buffer was written on the caller's stream (the collective);
    // NULL is the legacy default stream, which the context's non-blocking
    // stream does not otherwise wait for
    HIPCHK(c, hipEventRecord(c->evw, (hipStream_t)wait_stream));
    HIPCHK(c, hipStreamWaitEvent(s, c->evw, 0));
    HIPCHK(c, hipEventRecord(c->ev2, s));
    // the received hits, concatenated by source rank, are in rank order
    kmer_status st = ensure_rank_arrays(c, n, 0, s);
    if (st) return st;
    HIPCHK(c, launch_xprep((const XHit *)d_recv, n, c->rkey.p, c->narrow ? c->rkey32.p : nullptr, c->rord.p,
                           c->ridx.p, s));
    uint64_t nu = 0;
    const bool sync = out || c->p.max_keys;
    st = rank_finish(c, n, false, false, &nu, sync);
    if (st) return st;
    c->n_out = nu;
    HIPCHK(c, hipEventRecord(c->ev3, s));
    c->timing_pending = true;
    c->n_hits = 0;
    c->n_cross = 0;
    c->open_stream = false;
    if (!sync) return KMER_OK;
    st = resolve_out(c);
    if (st) return st;
    const uint64_t total = c->n_out + c->exotic.size();
    if (c->p.max_keys && total > c->p.max_keys)
        return fail(c, KMER_E_TOO_MANY_KEYS, "more distinct keys than max_keys (reference Map limit)");
    if (!out) return KMER_OK;
    return build_result(c, total_lines, out);
}

// Table mode across ranks: rank o owns the pass-1 partitions [o * TAB_NB /
// world, (o + 1) * TAB_NB / world), i.e. a contiguous slice of the hash space
// and its buckets.  The send buffer holds, per owner, that owner's
// partitions in partition order (one chunk: tb1 as it is).
uint32_t tab_part_lo(uint32_t o, uint32_t world) { return (uint32_t)((uint64_t)o * TAB_NB / world); }

kmer_status kmer_table_exchange_prepare(kmer_ctx *c, uint32_t world, const void **d_send, uint64_t *counts,
                                        uint64_t *parts) {
    if (!c || !d_send || !counts || !parts || world == 0 || world > TAB_NB) return KMER_E_BAD_PARAM;
    SETTLE(c);
    if (c->mode != MODE_TABLE) return fail(c, KMER_E_STATE, "not a table-mode context (KMER_FLAG_UNORDERED)");
    if (!c->open_stream) return fail(c, KMER_E_STATE, "exchange without reset/feed");
    if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
    hipStream_t s = c->stream;
    const size_t nch = c->t_cbase.size();
    for (uint32_t p = 0; p < TAB_NB; ++p) {
        uint64_t x = 0;
        for (size_t ch = 0; ch < nch; ++ch) x += c->t_coff[ch][p + 1] - c->t_coff[ch][p];
        parts[p] = x;
    }
    for (uint32_t o = 0; o < world; ++o) {
        uint64_t x = 0;
        for (uint32_t p = tab_part_lo(o, world); p < tab_part_lo(o + 1, world); ++p) x += parts[p];
        counts[o] = x;
    }
    *d_send = nullptr;
    const uint64_t n = c->t_keys;
    if (n == 0) return KMER_OK;
    // (narrow keys: the 32-bit pass-1 keys go out widened to h, the receiving
    // side's table_finish reads 64-bit keys)
    const bool narrow = c->p.k <= TAB_NARROW_K;
    if (nch == 1 && c->t_cbase[0] == 0 && !narrow) {
        *d_send = c->tb1.p;
        return KMER_OK;
    }
    std::vector<TabSeg> segs;
    uint64_t dst = 0;
    for (uint32_t p = 0; p < TAB_NB; ++p)
        for (size_t ch = 0; ch < nch; ++ch) {
            const uint64_t a0 = c->t_coff[ch][p], a1 = c->t_coff[ch][p + 1];
            if (a1 > a0) segs.push_back(TabSeg{c->t_cbase[ch] + a0, dst, a1 - a0, p});
            dst += a1 - a0;
        }
    if (segs.size() >= (1ull << 31)) return fail(c, KMER_E_BAD_PARAM, "too many table segments");
    HIPCHK(c, c->tsend.ensure(n, s));
    HIPCHK(c, c->tseg.ensure(segs.size(), s));
    kmer_status st = upload(c, c->tseg.p, segs.data(), segs.size() * sizeof(TabSeg), s);
    if (st) return st;
    if (narrow)
        HIPCHK(c, launch_tab_widen((const uint32_t *)c->tb1.p, c->tseg.p, (uint32_t)segs.size(), c->tsend.p, s));
    else
        HIPCHK(c, launch_tab_segcopy(c->tb1.p, c->tseg.p, (uint32_t)segs.size(), c->tsend.p, s));
    HIPCHK(c, hipStreamSynchronize(s));        // (the caller's collective follows)
    *d_send = c->tsend.p;
    return KMER_OK;
}

kmer_status kmer_table_finish_exchanged(kmer_ctx *c, void *d_recv, uint64_t n, const uint64_t *parts,
                                        uint32_t world, uint32_t rank, void *wait_stream) {
    if (!c || (n && !d_recv) || !parts || world == 0 || world > TAB_NB || rank >= world) return KMER_E_BAD_PARAM;
    SETTLE(c);
    if (c->mode != MODE_TABLE) return fail(c, KMER_E_STATE, "not a table-mode context (KMER_FLAG_UNORDERED)");
    if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
    const uint32_t plo = tab_part_lo(rank, world), phi = tab_part_lo(rank + 1, world);
    // the received runs, by source rank: source r's keys of this rank's
    // partitions, partition-major -- one "chunk" per source
    std::vector<uint64_t> cbase;
    std::vector<std::vector<uint64_t>> coff;
    uint64_t base = 0;
    for (uint32_t r = 0; r < world; ++r) {
        std::vector<uint64_t> off(TAB_NB + 1, 0);
        uint64_t x = 0;
        for (uint32_t p = 0; p < TAB_NB; ++p) {
            off[p] = x;
            if (p >= plo && p < phi) x += parts[(uint64_t)r * TAB_NB + p];
        }
        off[TAB_NB] = x;
        cbase.push_back(base);
        coff.push_back(std::move(off));
        base += x;
    }
    if (base != n) return fail(c, KMER_E_BAD_PARAM, "received key count does not match the partition counts");
    hipStream_t s = c->stream;
    HIPCHK(c, hipEventRecord(c->evw, (hipStream_t)wait_stream));
    HIPCHK(c, hipStreamWaitEvent(s, c->evw, 0));
    c->t_cbase = std::move(cbase);
    c->t_coff = std::move(coff);
    c->t_keys = n;
    HIPCHK(c, hipEventRecord(c->ev2, s));
    kmer_status st = table_finish(c, n ? (const uint64_t *)d_recv : nullptr, plo << TAB_L2, phi << TAB_L2);
    if (st) return st;
    HIPCHK(c, hipEventRecord(c->ev3, s));
    c->timing_pending = true;
    c->open_stream = false;
    return KMER_OK;
}

kmer_status kmer_records_export(kmer_ctx *c, kmer_result **out) {
    if (!c || !out) return KMER_E_BAD_PARAM;
    SETTLE(c);
    if (c->gm_on && c->gm_n) {              // (general-path entries held on the device travel as records)
        if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
        kmer_status st = general_to_host(c);
        if (st) return st;
    }
    kmer_result *r = new (std::nothrow) kmer_result();
    if (!r) return KMER_E_OOM;
    std::vector<std::pair<uint64_t, const std::pair<const std::string, Ent> *>> ex;
    for (auto &kv : c->exotic) ex.emplace_back(kv.second.first, &kv);
    std::sort(ex.begin(), ex.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
    for (auto &e : ex) {
        r->keys.insert(r->keys.end(), e.second->first.begin(), e.second->first.end());
        r->offsets.push_back(r->keys.size());
        r->counts.push_back(e.second->second.count);
        r->firsts.push_back(e.first);
    }
    *out = r;
    return KMER_OK;
}

kmer_status kmer_records_import(kmer_ctx *c, const char *keys, const uint64_t *offsets, const uint64_t *counts,
                                const uint64_t *firsts, uint64_t n) {
    if (!c || (n && (!keys || !offsets || !counts || !firsts))) return KMER_E_BAD_PARAM;
    SETTLE(c);
    for (uint64_t i = 0; i < n; ++i) {
        std::string key(keys + offsets[i], offsets[i + 1] - offsets[i]);
        auto it = c->exotic.find(key);
        if (it == c->exotic.end()) {
            c->exotic.emplace(key, Ent{counts[i], firsts[i]});
        } else {
            it->second.count += counts[i];
            it->second.first = std::min(it->second.first, firsts[i]);
        }
    }
    return KMER_OK;
}

kmer_status kmer_records_clear(kmer_ctx *c) {
    if (!c) return KMER_E_BAD_PARAM;
    SETTLE(c);
    c->exotic.clear();
    return KMER_OK;
}

kmer_status kmer_set_position(kmer_ctx *c, uint64_t lines_before, uint64_t byte_offset) {
    if (!c) return KMER_E_BAD_PARAM;
    SETTLE(c);
    if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
    c->prep_flags |= PREP_SETPOS;      // applied by the next feed's prologue (flush_prep)
    c->prep_lines = lines_before;
    c->abs_offset = byte_offset;
    c->host_lines = lines_before;
    return KMER_OK;
}

kmer_status kmer_lines(kmer_ctx *c, uint64_t *lines) {
    if (!c || !lines) return KMER_E_BAD_PARAM;
    SETTLE(c);
    StreamPos pos;
    kmer_status st = read_pos(c, &pos);
    if (st) return st;
    *lines = c->fasta ? c->fa_lines : pos.lines + pos.ends_open;
    return KMER_OK;
}

kmer_status kmer_result_device(kmer_ctx *c, const void **d_keys, const void **d_counts, const void **d_firsts,
                               uint64_t *n) {
    if (!c || !n) return KMER_E_BAD_PARAM;
    SETTLE(c);
    if (c->mode == MODE_TABLE) return fail(c, KMER_E_STATE, "table mode: use kmer_table_device");
    kmer_status st = resolve_out(c);
    if (st) return st;
    if (d_keys) *d_keys = c->keys_out.p;
    if (d_counts) *d_counts = c->cnt_out.p;
    if (d_firsts) *d_firsts = c->first.p;
    *n = c->n_out;
    return KMER_OK;
}

kmer_status kmer_table_stats(kmer_ctx *c, uint64_t *canonical, uint64_t *keys, uint64_t *total) {
    if (!c) return KMER_E_BAD_PARAM;
    if (!c->group.empty()) {                         // a group: its children's shares add up
        if (c->mode != MODE_TABLE || !c->t_done) return fail(c, KMER_E_STATE, "no table finish on this group yet");
        uint64_t a[3] = {0, 0, 0};
        for (kmer_ctx *x : c->group) {
            uint64_t b[3] = {0, 0, 0};
            if (hipSetDevice(x->device) != hipSuccess) return KMER_E_DEVICE;
            const kmer_status st = kmer_table_stats(x, &b[0], &b[1], &b[2]);
            if (st) return fail(c, st, x->err);
            for (int i = 0; i < 3; ++i) a[i] += b[i];
        }
        if (canonical) *canonical = a[0];
        if (keys) *keys = a[1];
        if (total) *total = a[2];
        return KMER_OK;
    }
    SETTLE(c);
    if (c->mode != MODE_TABLE) return fail(c, KMER_E_STATE, "not a table-mode context (KMER_FLAG_UNORDERED)");
    if (!c->t_done) return fail(c, KMER_E_STATE, "no table finish yet");
    uint64_t rk = 0, rs = 0;
    if (c->p.flags & KMER_FLAG_CANONICAL) {
        for (auto &kv : canonical_records(c))
            if (kv.first.compare(0, c->prefix.size(), c->prefix) == 0) {
                rk += 1;
                rs += kv.second;
            }
    } else {
        for (auto &kv : c->exotic) {
            rk += 1;
            rs += kv.second.count;
        }
    }
    if (canonical) *canonical = c->t_canon;
    if (keys) *keys = c->t_nkeys + rk;
    if (total) *total = c->t_sum + rs;
    return KMER_OK;
}

kmer_status kmer_table_device(kmer_ctx *c, const void **d_entries, const void **d_bucket_start,
                              const void **d_bucket_len, const void **d_big, uint64_t *n_big) {
    if (!c) return KMER_E_BAD_PARAM;
    SETTLE(c);
    if (c->mode != MODE_TABLE) return fail(c, KMER_E_STATE, "not a table-mode context (KMER_FLAG_UNORDERED)");
    if (!c->t_done) return fail(c, KMER_E_STATE, "no table finish yet");
    const bool any = c->t_keys != 0;
    if (d_entries) *d_entries = any ? c->t_ent : nullptr;
    if (d_bucket_start) *d_bucket_start = any ? c->tstart.p : nullptr;
    if (d_bucket_len) *d_bucket_len = any ? c->tnd.p : nullptr;
    if (d_big) *d_big = any ? c->tbig.p : nullptr;
    if (n_big) *n_big = c->t_nbig;
    return KMER_OK;
}

kmer_status kmer_table_digest(kmer_ctx *c, uint64_t *digest) {
    if (!c || !digest) return KMER_E_BAD_PARAM;
    if (!c->group.empty()) {                         // a group: its children's digests add up
        if (c->mode != MODE_TABLE || !c->t_done) return fail(c, KMER_E_STATE, "no table finish on this group yet");
        uint64_t a = 0;
        for (kmer_ctx *x : c->group) {
            uint64_t d = 0;
            if (hipSetDevice(x->device) != hipSuccess) return KMER_E_DEVICE;
            const kmer_status st = kmer_table_digest(x, &d);
            if (st) return fail(c, st, x->err);
            a += d;
        }
        *digest = a;
        return KMER_OK;
    }
    SETTLE(c);
    if (c->mode != MODE_TABLE) return fail(c, KMER_E_STATE, "not a table-mode context (KMER_FLAG_UNORDERED)");
    if (!c->t_done) return fail(c, KMER_E_STATE, "no table finish yet");
    *digest = 0;
    if (!c->t_keys) return KMER_OK;
    hipStream_t s = c->stream;
    unsigned long long *d = c->tstats.p + 4;
    HIPCHK(c, hipMemsetAsync(d, 0, 8, s));
    const bool narrow = c->p.k <= TAB_NARROW_K;
    HIPCHK(c, launch_tab_digest(c->t_ent, c->tstart.p, c->tnd.p, c->p.k, narrow ? 1u : 0u, d, s));
    uint64_t acc = 0;
    std::vector<TabBig> big(c->t_nbig);
    HIPCHK(c, hipMemcpyAsync(&acc, d, 8, hipMemcpyDeviceToHost, s));
    if (!big.empty())
        HIPCHK(c, hipMemcpyAsync(big.data(), c->tbig.p, big.size() * sizeof(TabBig), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    for (const TabBig &b : big)   // (entries hold TAB_CMAX)
        acc += (b.count - TAB_CMAX) * tab_digest_mix(tab_digest_key(b.h, c->p.k, narrow));
    *digest = acc;
    return KMER_OK;
}

// ---- table lookup (kmer_lookup.hip) ----
constexpr uint64_t LOOKUP_PIECE = 1ull << 20;   // keys per upload of the host call (<= 32 MiB of the arena)

static kmer_status lookup_state(kmer_ctx *c) {
    if (c->mode != MODE_TABLE) return fail(c, KMER_E_STATE, "not a table-mode context (KMER_FLAG_UNORDERED)");
    if (!c->t_done) return fail(c, KMER_E_STATE, "no table finish yet");
    return KMER_OK;
}

// The finished table (not empty) as its readers see it: the one place that
// names the context's table buffers (the lookup below; the matcher's probe
// through table_view)
static void view_key_params(const kmer_ctx *c, TabView *v) {
    v->k = c->p.k;
    v->plo = v->phi = 0;
    for (size_t i = 0; i < c->prefix.size(); ++i) {
        const uint8_t ch = (uint8_t)c->prefix[i];
        v->plo |= ((((uint32_t)ch >> 1) ^ ((uint32_t)ch >> 2)) & 1u) << i;
        v->phi |= (((uint32_t)ch >> 2) & 1u) << i;
    }
    v->pmask = c->prefix.size() >= 32 ? ~0u : ((1u << c->prefix.size()) - 1u);
    v->canonical = (c->p.flags & KMER_FLAG_CANONICAL) ? 1u : 0u;
}

static kmer_status fill_view(kmer_ctx *c, TabView *v) {
    if (!c->t_ent || !c->tstart.p || !c->tnd.p || !c->tbig.p) return fail(c, KMER_E_STATE, "no table finish yet");
    HIPCHK(c, c->tlk_bad.ensure(1, c->stream));
    memset(v, 0, sizeof(*v));
    v->ent = c->t_ent;
    v->start = c->tstart.p;
    v->nd = c->tnd.p;
    v->cap = c->t_keys;
    v->big = c->tbig.p;
    v->n_big = std::min<uint64_t>(c->t_nbig, c->tbig.cap);
    view_key_params(c, v);
    v->err = c->d_err;
    v->badq = c->tlk_bad.p;
    return KMER_OK;
}

// The lookup of n device-resident keys, queued on the context's stream and
// waited for; a refused bucket extent (ERR_TAB_LOOKUP) is reported here.
static kmer_status lookup_run(kmer_ctx *c, const uint8_t *d_keys, uint64_t n, uint64_t *d_counts) {
    hipStream_t s = c->stream;
    if (!c->t_keys) {                                // an empty table: every answer is 0
        HIPCHK(c, hipMemsetAsync(d_counts, 0, n * 8, s));
        HIPCHK(c, hipStreamSynchronize(s));
        return KMER_OK;
    }
    TabLookup a;
    memset(&a, 0, sizeof(a));
    const kmer_status vs = fill_view(c, &a);
    if (vs) return vs;
    a.keys = d_keys;
    a.n = n;
    a.counts = d_counts;
    HIPCHK(c, launch_tab_lookup(a, (uint32_t)std::max(c->n_cu, 1), s));
    uint32_t e = 0, q = 0;
    HIPCHK(c, hipMemcpyAsync(&e, c->d_err, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&q, c->tlk_bad.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (e & ERR_TAB_LOOKUP) {
        HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)c->d_err, (int)(e & ~ERR_TAB_LOOKUP), 1, s));
        HIPCHK(c, hipStreamSynchronize(s));
        return fail(c, KMER_E_DEVICE, "table lookup: the extent of bucket " + std::to_string(q) + " lies past the table");
    }
    return KMER_OK;
}

kmer_status kmer_table_lookup(kmer_ctx *c, const char *keys, uint64_t n, uint64_t *counts) {
    if (!c || (n && (!keys || !counts))) return KMER_E_BAD_PARAM;
    const uint64_t k = c->p.k;
    if (!c->group.empty()) {                         // a group: the children's slices are disjoint, their answers add
        if (c->mode != MODE_TABLE || !c->t_done) return fail(c, KMER_E_STATE, "no table finish on this group yet");
        std::vector<uint64_t> part;
        for (uint64_t n0 = 0; n0 < n; n0 += LOOKUP_PIECE) {
            const uint64_t m = std::min(LOOKUP_PIECE, n - n0);
            part.resize(m);
            std::fill(counts + n0, counts + n0 + m, 0);
            for (kmer_ctx *x : c->group) {
                if (hipSetDevice(x->device) != hipSuccess) return KMER_E_DEVICE;
                const kmer_status st = kmer_table_lookup(x, keys + n0 * k, m, part.data());
                if (st) return fail(c, st, x->err);
                for (uint64_t i = 0; i < m; ++i) counts[n0 + i] += part[i];
            }
        }
        return KMER_OK;
    }
    SETTLE(c);
    kmer_status st = lookup_state(c);
    if (st || n == 0) return st;
    if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
    hipStream_t s = c->stream;
    for (uint64_t n0 = 0; n0 < n; n0 += LOOKUP_PIECE) {
        const uint64_t m = std::min(LOOKUP_PIECE, n - n0);
        HIPCHK(c, c->tlk_keys.ensure(m * k, s));
        HIPCHK(c, c->tlk_cnt.ensure(m, s));
        st = upload(c, c->tlk_keys.p, keys + n0 * k, m * k, s);
        if (st) return st;
        st = lookup_run(c, c->tlk_keys.p, m, c->tlk_cnt.p);
        if (st) return st;
        HIPCHK(c, hipMemcpyAsync(counts + n0, c->tlk_cnt.p, m * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
    }
    if (c->exotic.empty()) return KMER_OK;
    // keys with a byte other than A/C/G/T: the record keys, as the host result lists them
    std::unordered_map<std::string, uint64_t> rec;
    if (c->p.flags & KMER_FLAG_CANONICAL) {
        for (auto &kv : canonical_records(c))
            if (kv.first.compare(0, c->prefix.size(), c->prefix) == 0) rec.emplace(kv.first, kv.second);
    } else {
        for (auto &kv : c->exotic) rec.emplace(kv.first, kv.second.count);
    }
    std::string key;
    for (uint64_t i = 0; i < n; ++i) {
        const char *x = keys + i * k;
        bool acgt = true;
        for (uint64_t j = 0; j < k && acgt; ++j) acgt = x[j] == 'A' || x[j] == 'C' || x[j] == 'G' || x[j] == 'T';
        if (acgt) continue;
        key.assign(x, k);
        const auto it = rec.find(key);
        if (it != rec.end()) counts[i] = it->second;
    }
    return KMER_OK;
}

kmer_status kmer_table_lookup_device(kmer_ctx *c, const void *d_keys, uint64_t n, void *d_counts, void *stream) {
    if (!c || (n && (!d_keys || !d_counts))) return KMER_E_BAD_PARAM;
    SETTLE(c);
    kmer_status st = lookup_state(c);
    if (st || n == 0) return st;
    if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
    HIPCHK(c, hipEventRecord(c->evw, (hipStream_t)stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->evw, 0));
    return lookup_run(c, (const uint8_t *)d_keys, n, (uint64_t *)d_counts);
}

// ---- read screen (kmer_screen.hip) ----
static_assert(sizeof(kmer_read_screen) == sizeof(ScreenRow) && sizeof(ScreenRow) == 32,
              "kmer_read_screen: the reduce kernel's row");
constexpr uint64_t SCREEN_BATCH = 64ull << 20;   // bytes per upload of the host call (batch_bytes overrides)

static bool screen_bad_flags(uint32_t flags) {
    const uint32_t all = KMER_SCREEN_DIRECT | KMER_SCREEN_SORTED | KMER_SCREEN_PIECE_TEST;
    return (flags & ~all) || ((flags & KMER_SCREEN_DIRECT) && (flags & KMER_SCREEN_SORTED));
}

// the state a screen needs, checked before any device call
static kmer_status screen_state(kmer_ctx *c) {
    if (!c->group.empty()) return fail(c, KMER_E_STATE, "single-device call on a group context");
    if (c->mode != MODE_TABLE) return fail(c, KMER_E_STATE, "not a table-mode context (KMER_FLAG_UNORDERED)");
    if (c->fasta) return fail(c, KMER_E_STATE, "read screen: FASTQ input only (the context has KMER_FLAG_FASTA)");
    const kmer_status st = settle(c);
    if (st) return st;
    if (!c->t_done) return fail(c, KMER_E_STATE, "no table finish yet");
    return KMER_OK;
}

// The screen of len device-resident bytes that start at a record start, queued
// on the context's stream and waited for: c->tsc_rows holds *n_reads rows.
static kmer_status screen_run(kmer_ctx *c, const uint8_t *d, uint64_t len, uint64_t min_count, uint32_t flags,
                              uint64_t *n_reads) {
    hipStream_t s = c->stream;
    *n_reads = 0;
    const uint64_t n_tiles64 = (len + TILE - 1) / TILE;
    if (n_tiles64 > 0x7FFFFFFFull) return fail(c, KMER_E_BAD_PARAM, "read screen: input too large for one call");
    const uint32_t n_tiles = (uint32_t)n_tiles64;
    if (!screen_ensure(c->tcount, n_tiles, s) || !screen_ensure(c->tbase, n_tiles, s) ||
        !screen_ensure(c->nlslots, (uint64_t)n_tiles * NL_SLOTS, s))
        return fail(c, KMER_E_OOM, "device allocation failed (read screen: line finder)");
    // the line finder from line phase 0, whatever the session's position is
    const uint64_t saved_lines = c->host_lines;
    c->host_lines = 0;
    uint64_t n_nl = 0, n_seq = 0;
    kmer_status st = chunk_lines(c, d, len, n_tiles, s, false, &n_nl, &n_seq);
    c->host_lines = saved_lines;
    if (st == KMER_E_NONASCII) {                     // (reported, not kept: the table stays readable)
        const std::string msg = c->err;
        HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)c->d_err, (int)((uint32_t)c->h_small[5] & ~ERR_NONASCII), 1, s));
        HIPCHK(c, hipStreamSynchronize(s));
        return fail(c, st, msg);
    }
    if (st) return st;
    *n_reads = n_seq;
    if (!n_seq) return KMER_OK;
    if (!screen_ensure(c->tsc_rows, n_seq, s) || !screen_ensure(c->wbase, n_seq, s))
        return fail(c, KMER_E_OOM, "device allocation failed (" + std::to_string(n_seq) + " screened reads)");
    HIPCHK(c, hipMemsetAsync(c->tsc_rows.p, 0, n_seq * sizeof(ScreenRow), s));
    ROCPRIM_RUN(c, rocprim::exclusive_scan(t, b, c->wcount.p, c->wbase.p, (uint64_t)0, (size_t)n_seq,
                                           rocprim::plus<uint64_t>(), s));
    HIPCHK(c, hipMemcpyAsync(c->h_small + 14, c->wbase.p + n_seq - 1, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(c->h_small + 15, c->wcount.p + n_seq - 1, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const uint64_t total = (c->h_small[14] + c->h_small[15]) / 2;   // (wcount: both strands' windows)
    if (!total) return KMER_OK;
    const bool table = c->t_keys != 0;               // (an empty table: every value is 0)
    const bool sorted = table && ((flags & KMER_SCREEN_SORTED) ||
                                  (!(flags & KMER_SCREEN_DIRECT) &&
                                   c->t_canon > (uint64_t)KMER_SCREEN_DIRECT_MAX * std::max(c->t_nq, 1u)));
    const uint64_t piece = (flags & KMER_SCREEN_PIECE_TEST) ? SC_PIECE_TEST : SC_PIECE;
    const uint64_t cap = std::min(total, piece);
    size_t tmp_bytes = 0;
    bool ok = screen_ensure(c->tsc_h, cap, s) && screen_ensure(c->tsc_val, cap, s) && screen_ensure(c->tsc_code, cap, s);
    if (ok && sorted) {
        HIPCHK(c, bucket_sort_bytes(cap, &tmp_bytes));
        for (auto *b : {&c->tsc_bkt, &c->tsc_bkt2, &c->tsc_idx, &c->tsc_idx2}) ok = ok && screen_ensure(*b, cap, s);
        ok = ok && screen_ensure(c->tmp, tmp_bytes + 16, s);
    }
    if (!ok) return fail(c, KMER_E_OOM, "device allocation failed (read screen: " + std::to_string(cap) + " windows)");
    TabScreen a;
    memset(&a, 0, sizeof(a));
    if (table) {
        st = fill_view(c, &a);
        if (st) return st;
    } else {
        view_key_params(c, &a);
    }
    const uint32_t cus = (uint32_t)std::max(c->n_cu, 1);
    a.data = d;
    a.len = len;
    a.lines = c->lines.p;
    a.wbase2 = c->wbase.p;
    a.n = n_seq;
    a.total = total;
    a.h = c->tsc_h.p;
    a.code = c->tsc_code.p;
    a.val = c->tsc_val.p;
    a.bkt = sorted ? c->tsc_bkt.p : nullptr;
    a.idx = sorted ? c->tsc_idx.p : nullptr;
    a.min_count = std::max<uint64_t>(min_count, 1);
    a.rows = c->tsc_rows.p;
    for (uint64_t p0 = 0; p0 < total; p0 += piece) {
        a.p0 = p0;
        a.m = std::min(piece, total - p0);
        HIPCHK(c, launch_screen_keys(a, cus, s));
        if (!table) {
            HIPCHK(c, hipMemsetAsync(a.val, 0, a.m * 8, s));
        } else if (sorted) {
            const uint32_t *sb = nullptr, *si = nullptr;
            HIPCHK(c, launch_bucket_sort(c->tsc_bkt.p, c->tsc_bkt2.p, c->tsc_idx.p, c->tsc_idx2.p, a.m, c->tmp.p,
                                         tmp_bytes, &sb, &si, s));
            HIPCHK(c, launch_screen_probe(a, sb, si, cus, s));
        } else {
            HIPCHK(c, launch_screen_probe(a, nullptr, nullptr, cus, s));
        }
        HIPCHK(c, launch_screen_reduce(a, s));
    }
    uint32_t e = 0, q = 0;
    if (table) {
        HIPCHK(c, hipMemcpyAsync(&e, c->d_err, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(&q, c->tlk_bad.p, 4, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(c, hipStreamSynchronize(s));
    if (e & ERR_TAB_LOOKUP) {
        HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)c->d_err, (int)(e & ~ERR_TAB_LOOKUP), 1, s));
        HIPCHK(c, hipStreamSynchronize(s));
        return fail(c, KMER_E_DEVICE, "read screen: the extent of bucket " + std::to_string(q) + " lies past the table");
    }
    return KMER_OK;
}

kmer_status kmer_table_screen_device(kmer_ctx *c, const void *d_bytes, size_t len, uint64_t min_count, uint32_t flags,
                                     void *stream, const void **d_rows, uint64_t *n_reads) {
    if (d_rows) *d_rows = nullptr;
    if (n_reads) *n_reads = 0;
    if (!c || !d_rows || !n_reads || (len && !d_bytes) || screen_bad_flags(flags)) return KMER_E_BAD_PARAM;
    if (len == 0) return KMER_OK;
    kmer_status st = screen_state(c);
    if (st) return st;
    if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
    HIPCHK(c, hipEventRecord(c->evw, (hipStream_t)stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->evw, 0));
    st = screen_run(c, (const uint8_t *)d_bytes, len, min_count, flags, n_reads);
    if (st) {
        *n_reads = 0;
        return st;
    }
    *d_rows = *n_reads ? c->tsc_rows.p : nullptr;
    return KMER_OK;
}

// The end of the host calls' next piece from pos: whole units of `unit` lines
// (4: a record, 8: a pair of mates), as many as fit the batch, at least one;
// the input's tail goes with the last piece.
static uint64_t screen_piece_end(const uint8_t *bytes, uint64_t len, uint64_t pos, uint64_t batch, uint64_t unit) {
    uint64_t e = pos, good = 0, cnt = 0;
    bool more = false;
    while (e < len) {
        const void *nl = memchr(bytes + e, '\n', len - e);
        if (!nl) break;
        e = (uint64_t)((const uint8_t *)nl - bytes) + 1;
        if ((++cnt % unit) != 0) continue;
        if (e - pos <= batch || !good) good = e;
        if (e - pos >= batch) {
            more = true;
            break;
        }
    }
    if (!more && (len - pos <= batch || !good)) good = len;  // the input's tail
    return good;
}

kmer_status kmer_table_screen(kmer_ctx *c, const uint8_t *bytes, size_t len, uint64_t min_count, uint32_t flags,
                              kmer_read_screen *rows, uint64_t cap, uint64_t *n_reads) {
    if (n_reads) *n_reads = 0;
    if (!c || !n_reads || (len && !bytes) || (cap && !rows) || screen_bad_flags(flags)) return KMER_E_BAD_PARAM;
    if (len == 0) return KMER_OK;
    kmer_status st = screen_state(c);
    if (st) return st;
    const uint64_t n_nl = count_newlines(bytes, len);
    const uint64_t n = n_nl ? (n_nl - 1) / 4 + 1 : 0;            // lines 1, 5, 9, .. of n_nl + 1
    *n_reads = n;
    if (cap < n) return fail(c, KMER_E_BAD_PARAM, "read screen: " + std::to_string(n) + " reads, room for " + std::to_string(cap));
    if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
    hipStream_t s = c->stream;
    const uint64_t batch = c->p.batch_bytes ? c->p.batch_bytes : SCREEN_BATCH;
    uint64_t done = 0;
    for (uint64_t pos = 0; pos < len;) {
        const uint64_t good = screen_piece_end(bytes, len, pos, batch, 4);
        const uint64_t m = good - pos;
        if (!screen_ensure(c->tsc_in, m, s)) return fail(c, KMER_E_OOM, "device allocation failed (read screen: input piece)");
        st = upload(c, c->tsc_in.p, bytes + pos, m, s);
        if (st) return st;
        uint64_t np = 0;
        st = screen_run(c, c->tsc_in.p, m, min_count, flags, &np);
        if (st) return st;
        if (done + np > n) return fail(c, KMER_E_DEVICE, "read screen: more rows than reads");
        if (np) {
            HIPCHK(c, hipMemcpyAsync(rows + done, c->tsc_rows.p, np * sizeof(ScreenRow), hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
        }
        done += np;
        pos = good;
    }
    if (done != n) return fail(c, KMER_E_DEVICE, "read screen: rows and reads differ");
    return KMER_OK;
}

// ---- read filter (kmer_filter.hip) ----
static_assert(sizeof(kmer_filter_params) == 32 && sizeof(kmer_filter_result) == 32, "kmer_filter_params / _result");
static_assert(KMER_FILTER_DROP == FILTER_DROP && KMER_FILTER_PAIRED == FILTER_PAIRED, "KMER_FILTER_*: the mark kernel's bits");

static bool filter_bad_params(const kmer_filter_params *p) {
    return p->frac_den == 0 || p->frac_num > p->frac_den || (p->flags & ~(KMER_FILTER_DROP | KMER_FILTER_PAIRED)) ||
           screen_bad_flags(p->screen_flags);
}

// The filter of len device-resident bytes that start at a record start: the
// screen (c->tsc_rows), then c->tfl_keep and, if want_out, the kept records in
// c->tfl_out; queued on the context's stream and waited for.
static kmer_status filter_run(kmer_ctx *c, const uint8_t *d, uint64_t len, const kmer_filter_params *p, bool want_out,
                              kmer_filter_result *res) {
    hipStream_t s = c->stream;
    memset(res, 0, sizeof(*res));
    uint64_t n = 0;
    kmer_status st = screen_run(c, d, len, p->min_count, p->screen_flags, &n);
    if (st || !n) return st;
    const uint64_t pad = ((len + 15) & ~15ull) + 16;
    if (!screen_ensure(c->tfl_rend, n, s) || !screen_ensure(c->tfl_keep, n, s) || !screen_ensure(c->tfl_scan, n, s) ||
        !screen_ensure(c->tfl_seg_src, n + 1, s) || !screen_ensure(c->tfl_seg_out, n + 1, s) ||
        (want_out && !screen_ensure(c->tfl_out, pad, s)))
        return fail(c, KMER_E_OOM, "device allocation failed (read filter: " + std::to_string(n) + " records, " +
                                       std::to_string(len) + " bytes)");
    FilterArgs a;
    memset(&a, 0, sizeof(a));
    a.data = d;
    a.len = len;
    a.n_nl = c->cl_nl;
    a.n_reads = n;
    a.slots = c->cl_slots ? c->nlslots.p : nullptr;
    a.tcount = c->tcount.p;
    a.tbase = c->tbase.p;
    a.n_tiles = (uint32_t)((len + TILE - 1) / TILE);
    a.cap = NL_SLOTS;
    a.nl = c->nlpos.p;
    a.rows = c->tsc_rows.p;
    a.min_hits = p->min_hits;
    a.frac_num = p->frac_num;
    a.frac_den = p->frac_den;
    a.flags = p->flags;
    a.rend = c->tfl_rend.p;
    a.keep = c->tfl_keep.p;
    a.scan = c->tfl_scan.p;
    a.seg_src = c->tfl_seg_src.p;
    a.seg_out = c->tfl_seg_out.p;
    a.out = c->tfl_out.p;
    HIPCHK(c, launch_filter_ends(a, s));
    HIPCHK(c, launch_filter_mark(a, s));
    ROCPRIM_RUN(c, rocprim::inclusive_scan(t, b, c->tfl_scan.p, c->tfl_scan.p, (size_t)n, FilterScanPlus(), s));
    HIPCHK(c, launch_filter_segments(a, s));
    HIPCHK(c, hipMemcpyAsync(c->h_small + 18, c->tfl_scan.p + n - 1, sizeof(FilterScan), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(c->h_small + 21, c->tfl_rend.p + n - 1, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    res->n_reads = n;
    res->n_kept = c->h_small[18];
    res->out_len = c->h_small[19];
    res->consumed = c->h_small[21];
    a.n_segs = c->h_small[20];
    a.out_len = res->out_len;
    if (res->n_kept > n || res->out_len > len || res->consumed > len || a.n_segs > res->n_kept)
        return fail(c, KMER_E_DEVICE, "read filter: the kept records exceed the input");
    if (want_out && a.out_len) {
        HIPCHK(c, launch_filter_copy(a, (uint32_t)std::max(c->n_cu, 1), s));
        HIPCHK(c, hipStreamSynchronize(s));
    }
    return KMER_OK;
}

kmer_status kmer_table_filter_device(kmer_ctx *c, const void *d_bytes, size_t len, const kmer_filter_params *p,
                                     void *stream, const void **d_out, const void **d_keep, const void **d_rows,
                                     kmer_filter_result *res) {
    if (d_out) *d_out = nullptr;
    if (d_keep) *d_keep = nullptr;
    if (d_rows) *d_rows = nullptr;
    if (res) memset(res, 0, sizeof(*res));
    if (!c || !p || !res || (len && !d_bytes) || filter_bad_params(p)) return KMER_E_BAD_PARAM;
    if (len == 0) return KMER_OK;
    kmer_status st = screen_state(c);
    if (st) return st;
    if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
    HIPCHK(c, hipEventRecord(c->evw, (hipStream_t)stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->evw, 0));
    st = filter_run(c, (const uint8_t *)d_bytes, len, p, d_out != nullptr, res);
    if (st) {
        memset(res, 0, sizeof(*res));
        return st;
    }
    if (d_out && res->out_len) *d_out = c->tfl_out.p;
    if (d_keep && res->n_reads) *d_keep = c->tfl_keep.p;
    if (d_rows && res->n_reads) *d_rows = c->tsc_rows.p;
    return KMER_OK;
}

kmer_status kmer_table_filter(kmer_ctx *c, const uint8_t *bytes, size_t len, const kmer_filter_params *p, uint8_t *out,
                              uint64_t out_cap, uint8_t *keep, uint64_t keep_cap, kmer_filter_result *res) {
    if (res) memset(res, 0, sizeof(*res));
    if (!c || !p || !res || (len && !bytes) || (out_cap && !out) || (keep_cap && !keep) || filter_bad_params(p))
        return KMER_E_BAD_PARAM;
    if (len == 0) return KMER_OK;
    kmer_status st = screen_state(c);
    if (st) return st;
    const uint64_t n_nl = count_newlines(bytes, len);
    const uint64_t n = n_nl ? (n_nl - 1) / 4 + 1 : 0;
    if (keep && keep_cap < n)
        return fail(c, KMER_E_BAD_PARAM, "read filter: " + std::to_string(n) + " records, room for " +
                                             std::to_string(keep_cap) + " keep flags");
    if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
    hipStream_t s = c->stream;
    const uint64_t batch = c->p.batch_bytes ? c->p.batch_bytes : SCREEN_BATCH;
    const uint64_t unit = (p->flags & KMER_FILTER_PAIRED) ? 8 : 4;   // lines per cut: a record, or a pair of mates
    kmer_filter_result tot;
    memset(&tot, 0, sizeof(tot));
    for (uint64_t pos = 0; pos < len;) {
        const uint64_t good = screen_piece_end(bytes, len, pos, batch, unit);
        const uint64_t m = good - pos;
        if (!screen_ensure(c->tsc_in, m, s)) return fail(c, KMER_E_OOM, "device allocation failed (read filter: input piece)");
        st = upload(c, c->tsc_in.p, bytes + pos, m, s);
        if (st) return st;
        kmer_filter_result r;
        st = filter_run(c, c->tsc_in.p, m, p, out != nullptr, &r);
        if (st) return st;
        if (tot.n_reads + r.n_reads > n) return fail(c, KMER_E_DEVICE, "read filter: more records than reads");
        if (out && tot.out_len + r.out_len > out_cap)
            return fail(c, KMER_E_BAD_PARAM, "read filter: the kept records need at least " +
                                                 std::to_string(tot.out_len + r.out_len) + " bytes, room for " +
                                                 std::to_string(out_cap));
        if (keep && r.n_reads)
            HIPCHK(c, hipMemcpyAsync(keep + tot.n_reads, c->tfl_keep.p, r.n_reads, hipMemcpyDeviceToHost, s));
        if (out && r.out_len)
            HIPCHK(c, hipMemcpyAsync(out + tot.out_len, c->tfl_out.p, r.out_len, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        tot.n_reads += r.n_reads;
        tot.n_kept += r.n_kept;
        tot.out_len += r.out_len;
        tot.consumed = pos + r.consumed;
        pos = good;
    }
    if (tot.n_reads != n) return fail(c, KMER_E_DEVICE, "read filter: records and reads differ");
    *res = tot;
    return KMER_OK;
}

kmer_status kmer_table_routes(kmer_ctx *c, uint64_t *p1_fixed, uint64_t *p1_merged, uint64_t *p1_counted,
                              uint64_t *p2_fixed) {
    if (!c) return KMER_E_BAD_PARAM;
    uint64_t f = 0, m = 0, n = 0, f2 = 0;
    if (!c->group.empty()) {                         // a group: its children's routes add up
        for (kmer_ctx *x : c->group) {
            if (hipSetDevice(x->device) != hipSuccess) return KMER_E_DEVICE;
            SETTLE(x);
            f += x->t_p1_fixed;
            m += x->t_p1_merged;
            n += x->t_p1_counted;
            f2 += x->t_p2_fixed;
        }
    } else {
        SETTLE(c);
        f = c->t_p1_fixed;
        m = c->t_p1_merged;
        n = c->t_p1_counted;
        f2 = c->t_p2_fixed;
    }
    if (p1_fixed) *p1_fixed = f;
    if (p1_merged) *p1_merged = m;
    if (p1_counted) *p1_counted = n;
    if (p2_fixed) *p2_fixed = f2;
    return KMER_OK;
}

kmer_status kmer_dense_routes(kmer_ctx *c, uint64_t *chunks, uint64_t *lines_per_wave) {
    if (!c) return KMER_E_BAD_PARAM;
    SETTLE(c);
    if (chunks) *chunks = c->d_chunks;
    if (lines_per_wave) *lines_per_wave = c->d_lpw;
    return KMER_OK;
}

// ---- table spectrum and extraction (kmer_abundance.hip) ----
static_assert(KMER_SPECTRUM_REG_MAX == AB_REGS && KMER_SPECTRUM_LDS_BINS == AB_LDS_BINS &&
                  KMER_SPECTRUM_MAX_BINS == AB_HIST_BINS,
              "include/kmer_api.h names the spectrum kernel's tiers");

// the record keys as the host result lists them (build_table_result): (key, value)
static std::vector<std::pair<std::string, uint64_t>> record_rows(const kmer_ctx *c) {
    std::vector<std::pair<std::string, uint64_t>> out;
    if (c->p.flags & KMER_FLAG_CANONICAL) {
        for (auto &kv : canonical_records(c))
            if (kv.first.compare(0, c->prefix.size(), c->prefix) == 0) out.emplace_back(kv.first, kv.second);
    } else {
        for (auto &kv : c->exotic) out.emplace_back(kv.first, kv.second.count);
    }
    return out;
}

// The error word after a walk of the table (read back by the caller with the
// refused bucket): ERR_TAB_LOOKUP / ERR_TAB_EXTRACT are reported and cleared.
static kmer_status abund_errors(kmer_ctx *c, uint32_t e, uint32_t q, const char *what) {
    if (!(e & (ERR_TAB_LOOKUP | ERR_TAB_EXTRACT))) return KMER_OK;
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)c->d_err, (int)(e & ~(ERR_TAB_LOOKUP | ERR_TAB_EXTRACT)), 1, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (e & ERR_TAB_LOOKUP)
        return fail(c, KMER_E_DEVICE, std::string(what) + ": the extent of bucket " + std::to_string(q) + " lies past the table");
    return fail(c, KMER_E_DEVICE, std::string(what) + ": more keys written than counted");
}

// the table's view and the scratch words behind the device histogram
static kmer_status abund_view(kmer_ctx *c, TabAbund *a) {
    memset(a, 0, sizeof(*a));
    const kmer_status vs = fill_view(c, a);
    if (vs) return vs;
    if (c->tab_hist.ensure(AB_HIST_BINS + 4, c->stream) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, KMER_E_OOM, "device allocation failed (spectrum histogram)");
    }
    a->hist = c->tab_hist.p;
    a->n_out = c->tab_hist.p + AB_HIST_BINS + 2;
    return KMER_OK;
}

// one context's spectrum added to hist (nbins bins, the last one open) and *top
static kmer_status spectrum_one(kmer_ctx *c, uint32_t nbins, uint64_t *hist, uint64_t *top) {
    auto add = [&](uint64_t v, uint64_t w) {
        if (!v || !w) return;
        if (v >= nbins - 1) {
            hist[nbins - 1] += w;
            *top += v * w;
        } else {
            hist[v] += w;
        }
    };
    if (c->t_keys) {
        if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
        hipStream_t s = c->stream;
        TabAbund a;
        const kmer_status vs = abund_view(c, &a);
        if (vs) return vs;
        unsigned long long *tail = c->tab_hist.p + AB_HIST_BINS;
        HIPCHK(c, hipMemsetAsync(a.hist, 0, (AB_HIST_BINS + 4) * 8, s));
        HIPCHK(c, launch_tab_spectrum(a, s));
        HIPCHK(c, launch_tab_spectrum_tail(a.hist, nbins - 1, tail, s));
        std::vector<uint64_t> part(nbins - 1);
        std::vector<TabBig> big(a.n_big);
        uint64_t last[2] = {0, 0};
        uint32_t e = 0, q = 0;
        HIPCHK(c, hipMemcpyAsync(part.data(), a.hist, part.size() * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(last, tail, 16, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(&e, c->d_err, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(&q, c->tlk_bad.p, 4, hipMemcpyDeviceToHost, s));
        if (!big.empty())
            HIPCHK(c, hipMemcpyAsync(big.data(), a.big, big.size() * sizeof(TabBig), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        const kmer_status es = abund_errors(c, e, q, "table spectrum");
        if (es) return es;
        for (uint32_t v = 0; v + 1 < nbins; ++v) hist[v] += part[v];
        hist[nbins - 1] += last[0];
        *top += last[1];
        for (const TabBig &b : big) {                // (entries hold TAB_CMAX: the kernel skipped them)
            uint64_t keys[2];
            bool dbl;
            const uint32_t w = tab_entry_keys(b.h, a.k, a.plo, a.phi, a.pmask, a.canonical != 0, keys, &dbl);
            add(dbl ? 2 * b.count : b.count, w);
        }
    }
    for (auto &kv : record_rows(c)) add(kv.second, 1);
    return KMER_OK;
}

kmer_status kmer_table_spectrum(kmer_ctx *c, uint32_t nbins, uint64_t *hist, uint64_t *top_sum) {
    if (!c || !hist || nbins < 2 || nbins > KMER_SPECTRUM_MAX_BINS) return KMER_E_BAD_PARAM;
    uint64_t top = 0;
    if (!c->group.empty()) {                         // a group: disjoint classes, the records in child 0
        if (c->mode != MODE_TABLE || !c->t_done) return fail(c, KMER_E_STATE, "no table finish on this group yet");
        std::fill(hist, hist + nbins, 0);
        for (kmer_ctx *x : c->group) {
            if (hipSetDevice(x->device) != hipSuccess) return KMER_E_DEVICE;
            const kmer_status st = settle(x);
            if (st) return fail(c, st, x->err);
            const kmer_status ss = spectrum_one(x, nbins, hist, &top);
            if (ss) return fail(c, ss, x->err);
        }
        if (top_sum) *top_sum = top;
        return KMER_OK;
    }
    SETTLE(c);
    const kmer_status st = lookup_state(c);
    if (st) return st;
    std::fill(hist, hist + nbins, 0);
    const kmer_status ss = spectrum_one(c, nbins, hist, &top);
    if (ss) return ss;
    if (top_sum) *top_sum = top;
    return KMER_OK;
}

// The device extract of one context: n keys of k bytes at *keys, their values
// at *counts, sorted by key bytes; complete when this returns.
static kmer_status extract_run(kmer_ctx *c, uint64_t lo, uint64_t hi, const uint8_t **keys, const uint64_t **counts,
                               uint64_t *n_out) {
    *keys = nullptr;
    *counts = nullptr;
    *n_out = 0;
    if (lo == 0) lo = 1;
    if ((hi && hi < lo) || !c->t_keys) return KMER_OK;
    if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
    hipStream_t s = c->stream;
    const uint32_t k = c->p.k, cus = (uint32_t)std::max(c->n_cu, 1);
    TabAbund a;
    const kmer_status vs = abund_view(c, &a);
    if (vs) return vs;
    a.lo = lo;
    a.hi = hi ? hi : ~0ull;
    uint64_t n = 0;
    uint32_t e = 0, q = 0;
    HIPCHK(c, hipMemsetAsync(a.n_out, 0, 8, s));
    HIPCHK(c, launch_tab_extract_count(a, s));
    HIPCHK(c, hipMemcpyAsync(&n, a.n_out, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&e, c->d_err, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&q, c->tlk_bad.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    kmer_status es = abund_errors(c, e, q, "table extract");
    if (es || !n) return es;
    size_t tmp_bytes = 0;
    HIPCHK(c, tab_extract_sort_bytes(n, k, &tmp_bytes));
    bool ok = c->tmp.ensure(tmp_bytes + 16, s) == hipSuccess && c->tex_keys.ensure(n * k + 4, s) == hipSuccess;
    for (auto *b : {&c->tex_code, &c->tex_code2, &c->tex_val, &c->tex_val2}) ok = ok && b->ensure(n, s) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        return fail(c, KMER_E_OOM, "device allocation failed (" + std::to_string(n) + " extracted keys)");
    }
    a.cap_out = n;
    a.codes = c->tex_code.p;
    a.vals = c->tex_val.p;
    const uint64_t *sc = nullptr, *sv = nullptr;
    uint64_t wrote = 0;
    HIPCHK(c, hipMemsetAsync(a.n_out, 0, 8, s));
    HIPCHK(c, launch_tab_extract_write(a, s));
    HIPCHK(c, launch_tab_extract_sort(c->tex_code.p, c->tex_code2.p, c->tex_val.p, c->tex_val2.p, n, k, c->tmp.p,
                                      tmp_bytes, &sc, &sv, s));
    HIPCHK(c, launch_tab_extract_decode(sc, n, k, c->tex_keys.p, cus, s));
    HIPCHK(c, hipMemcpyAsync(&wrote, a.n_out, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&e, c->d_err, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&q, c->tlk_bad.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    es = abund_errors(c, e, q, "table extract");
    if (es) return es;
    if (wrote != n) return fail(c, KMER_E_DEVICE, "table extract: counted and written keys differ");
    *keys = c->tex_keys.p;
    *counts = sv;
    *n_out = n;
    return KMER_OK;
}

kmer_status kmer_table_extract_device(kmer_ctx *c, uint64_t lo, uint64_t hi, const void **d_keys, const void **d_counts,
                                      uint64_t *n) {
    if (!c || !d_keys || !d_counts || !n) return KMER_E_BAD_PARAM;
    SETTLE(c);
    const kmer_status st = lookup_state(c);
    if (st) return st;
    const uint8_t *dk = nullptr;
    const uint64_t *dc = nullptr;
    const kmer_status es = extract_run(c, lo, hi, &dk, &dc, n);
    *d_keys = dk;
    *d_counts = dc;
    return es;
}

// rows = the n sorted A/C/G/T keys (k bytes each in kb, values in cnt) and the
// record keys recs, merged by key bytes
static void merge_rows(const std::vector<char> &kb, const std::vector<uint64_t> &cnt, uint64_t k,
                       std::vector<std::pair<std::string, uint64_t>> &recs,
                       std::vector<std::pair<std::string, uint64_t>> &rows) {
    const uint64_t n = cnt.size();
    std::sort(recs.begin(), recs.end());
    rows.clear();
    rows.reserve(n + recs.size());
    size_t j = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const char *x = kb.data() + i * k;
        while (j < recs.size() && recs[j].first.compare(0, std::string::npos, x, k) < 0) rows.push_back(recs[j++]);
        rows.emplace_back(std::string(x, k), cnt[i]);
    }
    while (j < recs.size()) rows.push_back(recs[j++]);
}

// One context's rows with a value in range, sorted by key bytes: the device
// extract copied to the host, the record keys merged in.
static kmer_status extract_rows(kmer_ctx *c, uint64_t lo, uint64_t hi, std::vector<std::pair<std::string, uint64_t>> &rows) {
    const uint8_t *dk = nullptr;
    const uint64_t *dc = nullptr;
    uint64_t n = 0;
    const kmer_status es = extract_run(c, lo, hi, &dk, &dc, &n);
    if (es) return es;
    const uint64_t k = c->p.k;
    std::vector<char> kb(n * k);
    std::vector<uint64_t> cnt(n);
    if (n) {
        hipStream_t s = c->stream;
        HIPCHK(c, hipMemcpyAsync(kb.data(), dk, n * k, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(cnt.data(), dc, n * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
    }
    if (lo == 0) lo = 1;
    std::vector<std::pair<std::string, uint64_t>> recs;
    for (auto &kv : record_rows(c))
        if (kv.second >= lo && (hi == 0 || kv.second <= hi)) recs.push_back(kv);
    merge_rows(kb, cnt, k, recs, rows);
    return KMER_OK;
}

kmer_status kmer_table_extract(kmer_ctx *c, uint64_t lo, uint64_t hi, kmer_result **out) {
    if (!c || !out) return KMER_E_BAD_PARAM;
    std::vector<std::pair<std::string, uint64_t>> rows;
    uint64_t lines = 0;
    if (!c->group.empty()) {                         // a group: the children's key sets are disjoint
        if (c->mode != MODE_TABLE || !c->t_done) return fail(c, KMER_E_STATE, "no table finish on this group yet");
        std::vector<std::pair<std::string, uint64_t>> part;
        for (kmer_ctx *x : c->group) {
            if (hipSetDevice(x->device) != hipSuccess) return KMER_E_DEVICE;
            kmer_status st = settle(x);
            if (!st) st = extract_rows(x, lo, hi, part);
            if (st) return fail(c, st, x->err);
            const size_t mid = rows.size();
            rows.insert(rows.end(), part.begin(), part.end());
            std::inplace_merge(rows.begin(), rows.begin() + mid, rows.end());
        }
        lines = c->t_lines;
    } else {
        SETTLE(c);
        kmer_status st = lookup_state(c);
        if (st) return st;
        if (hipSetDevice(c->device) != hipSuccess) return KMER_E_DEVICE;
        st = extract_rows(c, lo, hi, rows);
        if (st) return st;
        StreamPos pos;
        st = read_pos(c, &pos);
        if (st) return st;
        lines = c->fasta ? c->fa_lines : pos.lines + pos.ends_open;
    }
    kmer_result *r = new (std::nothrow) kmer_result();
    if (!r) return fail(c, KMER_E_OOM, "host allocation failed");
    r->lines = lines;
    for (auto &e : rows) {
        r->keys.insert(r->keys.end(), e.first.begin(), e.first.end());
        r->offsets.push_back(r->keys.size());
        r->counts.push_back(e.second);
        r->firsts.push_back(0);
    }
    *out = r;
    return KMER_OK;
}

// ---- set operations of two tables (kmer_setops.hip) ----
static_assert(KMER_JOIN_TILE == JOIN_TILE && (int)KMER_SETOP_INTERSECT == (int)JOIN_INTERSECT &&
                  (int)KMER_SETOP_SUBTRACT == (int)JOIN_SUBTRACT && (int)KMER_SETOP_UNION == (int)JOIN_UNION,
              "include/kmer_api.h names the join kernel's tile and operations");
static_assert(sizeof(kmer_table_overlap) == 8 * sizeof(uint64_t), "kmer_table_overlap: the kernel's eight sums");

static kmer_status table_view_impl(kmer_ctx *c, TabView *v, TabOwner *o);

// The parameter and state checks of a call on two contexts: no device call yet.
static kmer_status join_params(kmer_ctx *a, kmer_ctx *b) {
    if (a->device != b->device) return fail(a, KMER_E_BAD_PARAM, "the two contexts are on different devices");
    if (a->p.k != b->p.k || ((a->p.flags ^ b->p.flags) & KMER_FLAG_CANONICAL) || a->prefix != b->prefix)
        return fail(a, KMER_E_BAD_PARAM, "the two contexts differ in k, KMER_FLAG_CANONICAL or prefix");
    for (kmer_ctx *c : {a, b}) {
        const char *who = c == a ? "first" : "second";
        if (!c->group.empty()) return fail(a, KMER_E_STATE, std::string("single-device call: the ") + who + " context is a group");
        if (c->mode != MODE_TABLE) return fail(a, KMER_E_STATE, std::string("the ") + who + " context is not in table mode");
        if (!c->t_done) return fail(a, KMER_E_STATE, std::string("no table finish yet on the ") + who + " context");
    }
    return KMER_OK;
}

// Both contexts settled, their tables' views filled (an empty table: nd ==
// nullptr), the scratch words of context a behind the outputs, and a's stream
// ordered after the work queued on b's.  *empty: both tables are empty.
static kmer_status join_views(kmer_ctx *a, kmer_ctx *b, uint64_t min_a, uint64_t min_b, TabJoin *j, bool *empty) {
    memset(j, 0, sizeof(*j));
    TabOwner oa, ob;
    kmer_status st = table_view_impl(a, &j->a, &oa);
    if (st) return st;
    if (b != a) {
        st = table_view_impl(b, &j->b, &ob);
        if (st) return fail(a, st, "second context: " + b->err);
    } else {
        j->b = j->a;
        ob = oa;
    }
    *empty = oa.empty && ob.empty;
    if (*empty) return KMER_OK;
    auto hollow = [](TabView *v, const TabView &from) {  // (the key parameters are the same on both sides)
        *v = from;
        v->ent = nullptr;
        v->start = nullptr;
        v->nd = nullptr;
        v->big = nullptr;
        v->n_big = 0;
        v->cap = 0;
    };
    if (oa.empty) hollow(&j->a, j->b);
    if (ob.empty) hollow(&j->b, j->a);
    if (hipSetDevice(a->device) != hipSuccess) return fail(a, KMER_E_DEVICE, "hipSetDevice failed");
    hipStream_t s = a->stream;
    if (a->tlk_bad.ensure(2, s) != hipSuccess || a->tjoin.ensure(16, s) != hipSuccess) {
        (void)hipGetLastError();
        return fail(a, KMER_E_OOM, "device allocation failed (set operation scratch)");
    }
    j->min_a = std::max<uint64_t>(min_a, 1);
    j->min_b = std::max<uint64_t>(min_b, 1);
    j->sums = a->tjoin.p;
    j->n_out = a->tjoin.p + 8;
    j->err = a->d_err;
    j->badq = a->tlk_bad.p;
    if (b != a) {
        HIPCHK(a, hipEventRecord(a->evw, b->stream));
        HIPCHK(a, hipStreamWaitEvent(s, a->evw, 0));
    }
    return KMER_OK;
}

// The error word after a walk of the two tables (read back by the caller with
// the refused bucket and its side): reported on context a and cleared.
static kmer_status join_errors(kmer_ctx *a, uint32_t e, const uint32_t bad[2], const char *what) {
    if (!(e & (ERR_TAB_LOOKUP | ERR_TAB_EXTRACT))) return KMER_OK;
    hipStream_t s = a->stream;
    HIPCHK(a, hipMemsetD32Async((hipDeviceptr_t)a->d_err, (int)(e & ~(ERR_TAB_LOOKUP | ERR_TAB_EXTRACT)), 1, s));
    HIPCHK(a, hipStreamSynchronize(s));
    if (e & ERR_TAB_LOOKUP)
        return fail(a, KMER_E_DEVICE, std::string(what) + ": the extent of bucket " + std::to_string(bad[0]) + " of the " +
                                          (bad[1] ? "second" : "first") + " context lies past the table");
    return fail(a, KMER_E_DEVICE, std::string(what) + ": more keys written than counted");
}

// the record keys that are in a side (value >= max(min, 1))
static std::unordered_map<std::string, uint64_t> join_records(const kmer_ctx *c, uint64_t min) {
    std::unordered_map<std::string, uint64_t> out;
    for (auto &kv : record_rows(c))
        if (kv.second >= std::max<uint64_t>(min, 1)) out.emplace(kv.first, kv.second);
    return out;
}

kmer_status kmer_table_compare(kmer_ctx *a, kmer_ctx *b, uint64_t min_a, uint64_t min_b, kmer_table_overlap *out) {
    if (!a || !b || !out) return KMER_E_BAD_PARAM;
    kmer_status st = join_params(a, b);
    if (st) return st;
    TabJoin j;
    bool empty = false;
    st = join_views(a, b, min_a, min_b, &j, &empty);
    if (st) return st;
    uint64_t sums[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (!empty) {
        hipStream_t s = a->stream;
        uint32_t e = 0, bad[2] = {0, 0};
        HIPCHK(a, hipMemsetAsync(j.sums, 0, sizeof(sums), s));
        HIPCHK(a, launch_tab_join_compare(j, s));
        HIPCHK(a, hipMemcpyAsync(sums, j.sums, sizeof(sums), hipMemcpyDeviceToHost, s));
        HIPCHK(a, hipMemcpyAsync(&e, a->d_err, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(a, hipMemcpyAsync(bad, j.badq, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(a, hipStreamSynchronize(s));
        st = join_errors(a, e, bad, "table compare");
        if (st) return st;
    }
    // the record keys of the two contexts, joined by the same rules
    const auto ra = join_records(a, min_a), rb = join_records(b, min_b);
    for (auto &kv : ra) {
        sums[0] += 1;
        sums[3] += kv.second;
        const auto it = rb.find(kv.first);
        if (it == rb.end()) continue;
        sums[2] += 1;
        sums[5] += kv.second;
        sums[6] += it->second;
        sums[7] += std::min(kv.second, it->second);
    }
    for (auto &kv : rb) {
        sums[1] += 1;
        sums[4] += kv.second;
    }
    out->keys_a = sums[0];
    out->keys_b = sums[1];
    out->keys_both = sums[2];
    out->total_a = sums[3];
    out->total_b = sums[4];
    out->shared_a = sums[5];
    out->shared_b = sums[6];
    out->sum_min = sums[7];
    return KMER_OK;
}

// The device set operation: n keys of k bytes at *keys, their values at
// *counts, sorted by key bytes, in context a's extract buffers; complete when
// this returns.  The extract's tail: count, exact allocation, write, sort, decode.
static kmer_status setop_run(kmer_ctx *a, kmer_ctx *b, uint32_t op, uint64_t min_a, uint64_t min_b,
                             const uint8_t **keys, const uint64_t **counts, uint64_t *n_out) {
    *keys = nullptr;
    *counts = nullptr;
    *n_out = 0;
    TabJoin j;
    bool empty = false;
    kmer_status st = join_views(a, b, min_a, min_b, &j, &empty);
    if (st || empty) return st;
    hipStream_t s = a->stream;
    const uint32_t k = a->p.k, cus = (uint32_t)std::max(a->n_cu, 1);
    const uint32_t walks = op == JOIN_UNION ? 2u : 1u;           // UNION: A's keys, then B's that are not in A
    j.op = op;
    uint64_t n = 0;
    uint32_t e = 0, bad[2] = {0, 0};
    HIPCHK(a, hipMemsetAsync(j.n_out, 0, 8, s));
    for (j.second = 0; j.second < walks; ++j.second) HIPCHK(a, launch_tab_join_count(j, s));
    HIPCHK(a, hipMemcpyAsync(&n, j.n_out, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(a, hipMemcpyAsync(&e, a->d_err, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(a, hipMemcpyAsync(bad, j.badq, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(a, hipStreamSynchronize(s));
    st = join_errors(a, e, bad, "table setop");
    if (st || !n) return st;
    size_t tmp_bytes = 0;
    HIPCHK(a, tab_extract_sort_bytes(n, k, &tmp_bytes));
    bool ok = a->tmp.ensure(tmp_bytes + 16, s) == hipSuccess && a->tex_keys.ensure(n * k + 4, s) == hipSuccess;
    for (auto *x : {&a->tex_code, &a->tex_code2, &a->tex_val, &a->tex_val2}) ok = ok && x->ensure(n, s) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        return fail(a, KMER_E_OOM, "device allocation failed (" + std::to_string(n) + " keys of a set operation)");
    }
    j.cap_out = n;
    j.codes = a->tex_code.p;
    j.vals = a->tex_val.p;
    const uint64_t *sc = nullptr, *sv = nullptr;
    uint64_t wrote = 0;
    HIPCHK(a, hipMemsetAsync(j.n_out, 0, 8, s));
    for (j.second = 0; j.second < walks; ++j.second) HIPCHK(a, launch_tab_join_write(j, s));
    HIPCHK(a, launch_tab_extract_sort(a->tex_code.p, a->tex_code2.p, a->tex_val.p, a->tex_val2.p, n, k, a->tmp.p,
                                      tmp_bytes, &sc, &sv, s));
    HIPCHK(a, launch_tab_extract_decode(sc, n, k, a->tex_keys.p, cus, s));
    HIPCHK(a, hipMemcpyAsync(&wrote, j.n_out, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(a, hipMemcpyAsync(&e, a->d_err, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(a, hipMemcpyAsync(bad, j.badq, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(a, hipStreamSynchronize(s));
    st = join_errors(a, e, bad, "table setop");
    if (st) return st;
    if (wrote != n) return fail(a, KMER_E_DEVICE, "table setop: counted and written keys differ");
    *keys = a->tex_keys.p;
    *counts = sv;
    *n_out = n;
    return KMER_OK;
}

// the record keys of the two contexts, joined by the setop's rules: (key, value), in no order
static std::vector<std::pair<std::string, uint64_t>> setop_records(const kmer_ctx *a, const kmer_ctx *b, uint32_t op,
                                                                   uint64_t min_a, uint64_t min_b) {
    const auto ra = join_records(a, min_a), rb = join_records(b, min_b);
    std::vector<std::pair<std::string, uint64_t>> recs;
    for (auto &kv : ra) {
        const auto it = rb.find(kv.first);
        if (op == KMER_SETOP_INTERSECT) {
            if (it != rb.end()) recs.emplace_back(kv.first, std::min(kv.second, it->second));
        } else if (op == KMER_SETOP_SUBTRACT) {
            if (it == rb.end()) recs.push_back(kv);
        } else {
            recs.emplace_back(kv.first, kv.second + (it != rb.end() ? it->second : 0));
        }
    }
    if (op == KMER_SETOP_UNION)
        for (auto &kv : rb)
            if (!ra.count(kv.first)) recs.push_back(kv);
    return recs;
}

kmer_status kmer_table_setop_device(kmer_ctx *a, kmer_ctx *b, uint32_t op, uint64_t min_a, uint64_t min_b,
                                    const void **d_keys, const void **d_counts, uint64_t *n) {
    if (!a || !b || !d_keys || !d_counts || !n || op > KMER_SETOP_UNION) return KMER_E_BAD_PARAM;
    const kmer_status st = join_params(a, b);
    if (st) return st;
    const uint8_t *dk = nullptr;
    const uint64_t *dc = nullptr;
    const kmer_status es = setop_run(a, b, op, min_a, min_b, &dk, &dc, n);
    *d_keys = dk;
    *d_counts = dc;
    return es;
}

kmer_status kmer_table_setop(kmer_ctx *a, kmer_ctx *b, uint32_t op, uint64_t min_a, uint64_t min_b, kmer_result **out) {
    if (!a || !b || !out || op > KMER_SETOP_UNION) return KMER_E_BAD_PARAM;
    kmer_status st = join_params(a, b);
    if (st) return st;
    const uint8_t *dk = nullptr;
    const uint64_t *dc = nullptr;
    uint64_t n = 0;
    st = setop_run(a, b, op, min_a, min_b, &dk, &dc, &n);
    if (st) return st;
    const uint64_t k = a->p.k;
    std::vector<char> kb(n * k);
    std::vector<uint64_t> cnt(n);
    if (n) {
        hipStream_t s = a->stream;
        HIPCHK(a, hipMemcpyAsync(kb.data(), dk, n * k, hipMemcpyDeviceToHost, s));
        HIPCHK(a, hipMemcpyAsync(cnt.data(), dc, n * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(a, hipStreamSynchronize(s));
    }
    std::vector<std::pair<std::string, uint64_t>> recs = setop_records(a, b, op, min_a, min_b), rows;
    merge_rows(kb, cnt, k, recs, rows);
    StreamPos pos;
    st = read_pos(a, &pos);
    if (st) return st;
    kmer_result *r = new (std::nothrow) kmer_result();
    if (!r) return fail(a, KMER_E_OOM, "host allocation failed");
    r->lines = a->fasta ? a->fa_lines : pos.lines + pos.ends_open;
    for (auto &e : rows) {
        r->keys.insert(r->keys.end(), e.first.begin(), e.first.end());
        r->offsets.push_back(r->keys.size());
        r->counts.push_back(e.second);
        r->firsts.push_back(0);
    }
    *out = r;
    return KMER_OK;
}

// The set operation whose result stays a table: the device part, on dst's
// stream and scratch (errors are left on dst; the caller reports them on a).
// dst has been reset; nothing of it is committed before the last check, so a
// failure leaves it in its reset state.  Count per bucket, scan, exact
// allocation, write -- no sort and no decode.
static kmer_status setop_into_run(kmer_ctx *a, kmer_ctx *b, uint32_t op, uint64_t min_a, uint64_t min_b, kmer_ctx *dst,
                                  TabJoin &j) {
    hipStream_t s = dst->stream;
    bool ok = dst->tjoin.ensure(16, s) == hipSuccess && dst->tlk_bad.ensure(2, s) == hipSuccess &&
              dst->tnd.ensure(TAB_NQ + 1, s) == hipSuccess && dst->tstart.ensure(TAB_NQ + 1, s) == hipSuccess &&
              dst->tstats.ensure(5, s) == hipSuccess && dst->tbig.ensure(1 << 16, s) == hipSuccess &&
              (op != JOIN_UNION || dst->tH.ensure(TAB_NQ, s) == hipSuccess);
    if (!ok) {
        (void)hipGetLastError();
        return fail(dst, KMER_E_OOM, "device allocation failed (the result table's bucket index)");
    }
    // dst's stream after the work queued on a's and on b's
    HIPCHK(dst, hipEventRecord(dst->evw, a->stream));
    HIPCHK(dst, hipStreamWaitEvent(s, dst->evw, 0));
    if (b != a) {
        HIPCHK(dst, hipEventRecord(dst->evw, b->stream));
        HIPCHK(dst, hipStreamWaitEvent(s, dst->evw, 0));
    }
    const uint32_t walks = op == JOIN_UNION ? 2u : 1u;           // UNION: A's classes, then B's that are not in A
    j.min_a = std::max<uint64_t>(min_a, 1);
    j.min_b = std::max<uint64_t>(min_b, 1);
    j.op = op;
    j.n_out = dst->tjoin.p + 8;
    j.err = dst->d_err;
    j.badq = dst->tlk_bad.p;
    j.nd_dst = dst->tnd.p;
    j.cur_dst = op == JOIN_UNION ? dst->tH.p : nullptr;
    auto errors = [&](uint32_t e, const uint32_t bad[2]) -> kmer_status {
        if (!(e & (ERR_TAB_LOOKUP | ERR_TAB_EXTRACT))) return KMER_OK;
        HIPCHK(dst, hipMemsetD32Async((hipDeviceptr_t)dst->d_err, (int)(e & ~(ERR_TAB_LOOKUP | ERR_TAB_EXTRACT)), 1, s));
        HIPCHK(dst, hipStreamSynchronize(s));
        if (e & ERR_TAB_LOOKUP)
            return fail(dst, KMER_E_DEVICE, "table setop into: the extent of bucket " + std::to_string(bad[0]) + " of the " +
                                                (bad[1] ? "second" : "first") + " context lies past the table");
        return fail(dst, KMER_E_DEVICE, "table setop into: more entries written than counted");
    };
    uint64_t total = 0, nbig = 0;
    uint32_t e = 0, bad[2] = {0, 0};
    HIPCHK(dst, hipMemsetAsync(j.n_out, 0, 8, s));
    HIPCHK(dst, hipMemsetAsync(dst->tnd.p + TAB_NQ, 0, sizeof(uint32_t), s));   // (the scan's last input)
    for (j.second = 0; j.second < walks; ++j.second) HIPCHK(dst, launch_tab_join_tcount(j, s));
    ROCPRIM_RUN(dst, rocprim::exclusive_scan(t, b, dst->tnd.p, dst->tstart.p, (uint64_t)0, (size_t)(TAB_NQ + 1),
                                             rocprim::plus<uint64_t>(), s));
    HIPCHK(dst, hipMemcpyAsync(&total, dst->tstart.p + TAB_NQ, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(dst, hipMemcpyAsync(&nbig, j.n_out, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(dst, hipMemcpyAsync(&e, dst->d_err, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(dst, hipMemcpyAsync(bad, j.badq, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(dst, hipStreamSynchronize(s));
    kmer_status st = errors(e, bad);
    if (st) return st;
    uint64_t stats[3] = {0, 0, 0};
    if (total) {
        if (dst->tb1.ensure(total, s) != hipSuccess || dst->tbig.ensure(nbig, s) != hipSuccess) {
            (void)hipGetLastError();
            return fail(dst, KMER_E_OOM, "device allocation failed (" + std::to_string(total) + " entries of a set operation)");
        }
        j.start_dst = dst->tstart.p;
        j.ent_dst = dst->tb1.p;
        j.cap_dst = total;
        j.big_dst = dst->tbig.p;
        j.big_cap = nbig;
        j.stats = dst->tstats.p;
        uint64_t wrote_big = 0;
        HIPCHK(dst, hipMemsetAsync(j.n_out, 0, 8, s));
        HIPCHK(dst, hipMemsetAsync(j.stats, 0, 3 * sizeof(unsigned long long), s));
        for (j.second = 0; j.second < walks; ++j.second) HIPCHK(dst, launch_tab_join_twrite(j, s));
        HIPCHK(dst, hipMemcpyAsync(stats, j.stats, sizeof(stats), hipMemcpyDeviceToHost, s));
        HIPCHK(dst, hipMemcpyAsync(&wrote_big, j.n_out, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(dst, hipMemcpyAsync(&e, dst->d_err, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(dst, hipMemcpyAsync(bad, j.badq, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(dst, hipStreamSynchronize(s));
        st = errors(e, bad);
        if (st) return st;
        if (stats[0] != total || wrote_big != nbig)
            return fail(dst, KMER_E_DEVICE, "table setop into: counted and written entries differ");
    }
    // the state a table finish leaves
    dst->t_ent = total ? dst->tb1.p : nullptr;
    dst->t_keys = total;
    dst->t_canon = stats[0];
    dst->t_nkeys = stats[1];
    dst->t_sum = stats[2];
    dst->t_nbig = total ? nbig : 0;
    dst->n_out = dst->t_nkeys;
    return KMER_OK;
}

kmer_status kmer_table_setop_into(kmer_ctx *a, kmer_ctx *b, uint32_t op, uint64_t min_a, uint64_t min_b, kmer_ctx *dst) {
    if (!a || !b || !dst || op > KMER_SETOP_UNION || dst == a || dst == b) return KMER_E_BAD_PARAM;
    // parameters, then states: no device call yet
    for (kmer_ctx *c : {b, dst}) {
        const char *who = c == dst ? "result" : "second";
        if (c->device != a->device)
            return fail(a, KMER_E_BAD_PARAM, std::string("the ") + who + " context is on another device than the first");
        if (c->p.k != a->p.k || ((c->p.flags ^ a->p.flags) & KMER_FLAG_CANONICAL) || c->prefix != a->prefix)
            return fail(a, KMER_E_BAD_PARAM,
                        std::string("the ") + who + " context differs from the first in k, KMER_FLAG_CANONICAL or prefix");
    }
    for (kmer_ctx *c : {a, b, dst}) {
        const char *who = c == dst ? "result" : c == a ? "first" : "second";
        if (!c->group.empty()) return fail(a, KMER_E_STATE, std::string("single-device call: the ") + who + " context is a group");
        if (c->mode != MODE_TABLE) return fail(a, KMER_E_STATE, std::string("the ") + who + " context is not in table mode");
        if (c != dst && !c->t_done) return fail(a, KMER_E_STATE, std::string("no table finish yet on the ") + who + " context");
    }
    if (hipSetDevice(a->device) != hipSuccess) return fail(a, KMER_E_DEVICE, "hipSetDevice failed");
    // both inputs settled, their views filled (an empty table: nd == nullptr)
    TabJoin j;
    memset(&j, 0, sizeof(j));
    TabOwner oa, ob;
    kmer_status st = table_view_impl(a, &j.a, &oa);
    if (st) return st;
    if (b != a) {
        st = table_view_impl(b, &j.b, &ob);
        if (st) return fail(a, st, "second context: " + b->err);
    } else {
        j.b = j.a;
        ob = oa;
    }
    auto hollow = [](TabView *v, const TabView &from) {          // (the key parameters are the same on both sides)
        *v = from;
        v->ent = nullptr;
        v->start = nullptr;
        v->nd = nullptr;
        v->big = nullptr;
        v->n_big = 0;
        v->cap = 0;
    };
    if (oa.empty && !ob.empty) hollow(&j.a, j.b);
    if (ob.empty && !oa.empty) hollow(&j.b, j.a);
    // what dst takes over from a, and the record keys joined on the host
    StreamPos pos;
    st = read_pos(a, &pos);
    if (st) return st;
    const uint64_t lines = a->fasta ? a->fa_lines : pos.lines + pos.ends_open;
    const std::vector<std::pair<std::string, uint64_t>> recs = setop_records(a, b, op, min_a, min_b);
    // dst: a chunk in flight settled, then the reset; its position is a's
    st = reset(dst);
    if (st) return fail(a, st, "result context: " + dst->err);
    dst->t_canon = dst->t_nkeys = dst->t_sum = dst->t_nbig = 0;
    dst->prep_flags |= PREP_SETPOS;
    dst->prep_lines = lines;
    dst->host_lines = lines;
    if (dst->fasta) dst->fa_lines = lines;
    st = flush_prep(dst, dst->stream, 0);                        // (clears dst's device error word as well)
    if (!st && !(oa.empty && ob.empty)) st = setop_into_run(a, b, op, min_a, min_b, dst, j);
    if (st) return fail(a, st, "result context: " + dst->err);
    for (auto &kv : recs) dst->exotic.emplace(kv.first, Ent{kv.second, 0});
    dst->t_nq = a->t_nq;
    dst->t_done = true;
    dst->open_stream = false;
    return KMER_OK;
}

kmer_status kmer_phase_times(kmer_ctx *c, uint32_t max, const char **names, double *ms, uint32_t *n) {
    if (!c || !n || (max && (!names || !ms))) return KMER_E_BAD_PARAM;
    SETTLE(c);
    static const char *tab_names[7] = {"lines", "hist1", "scatter1", "hist2", "scatter2", "final", "fasta"};
    static const char *ord_names[3] = {"scan", "feed", "finish"};
    if (c->mode == MODE_TABLE) {
        *n = c->fasta ? 7 : 6;                   // (fasta: the FASTA rewrite of the chunks)
        for (uint32_t i = 0; i < *n && i < max; ++i) {
            names[i] = tab_names[i];
            ms[i] = c->t_ms[i];
        }
        return KMER_OK;
    }
    kmer_status st = resolve_out(c);
    if (st) return st;
    const double v[3] = {c->scan_ms, c->feed_ms, c->finish_ms};
    *n = 3;
    for (uint32_t i = 0; i < 3 && i < max; ++i) {
        names[i] = ord_names[i];
        ms[i] = v[i];
    }
    return KMER_OK;
}

kmer_status kmer_last_timing(kmer_ctx *c, double *scan_ms, double *feed_ms, double *finish_ms) {
    if (!c) return KMER_E_BAD_PARAM;
    SETTLE(c);
    // (the finish is waited for only when its time is asked for)
    if (finish_ms) {
        const kmer_status st = resolve_out(c);
        if (st) return st;
    }
    if (scan_ms) *scan_ms = c->scan_ms;
    if (feed_ms) *feed_ms = c->feed_ms;
    if (finish_ms) *finish_ms = c->finish_ms;
    return KMER_OK;
}

kmer_status kmer_synth_fastq_device(void *d_out, uint64_t seed, uint64_t first_read, uint64_t n_reads,
                                    void *stream) {
    if (!d_out && n_reads) return KMER_E_BAD_PARAM;
    hipError_t e = launch_synth_fastq((uint8_t *)d_out, seed, first_read, n_reads, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    return e == hipSuccess ? KMER_OK : KMER_E_DEVICE;
}

uint64_t kmer_result_size(const kmer_result *r) { return r ? r->counts.size() : 0; }
uint64_t kmer_result_lines(const kmer_result *r) { return r ? r->lines : 0; }

kmer_status kmer_result_get(const kmer_result *r, uint64_t i, const char **key, uint32_t *klen, uint64_t *count) {
    if (!r || i >= r->counts.size()) return KMER_E_BAD_PARAM;
    if (key) *key = r->keys.data() + r->offsets[i];
    if (klen) *klen = (uint32_t)(r->offsets[i + 1] - r->offsets[i]);
    if (count) *count = r->counts[i];
    return KMER_OK;
}

kmer_status kmer_result_arrays(const kmer_result *r, const char **keys, const uint64_t **offsets,
                               const uint64_t **counts) {
    if (!r) return KMER_E_BAD_PARAM;
    if (keys) *keys = r->keys.data();
    if (offsets) *offsets = r->offsets.data();
    if (counts) *counts = r->counts.data();
    return KMER_OK;
}

kmer_status kmer_result_firsts(const kmer_result *r, const uint64_t **firsts) {
    if (!r || !firsts) return KMER_E_BAD_PARAM;
    *firsts = r->firsts.data();
    return KMER_OK;
}

// Serialise a result in Map order.  KMER_WRITE_JSON: JSON.stringify of
// mapToJSON(map) (lib/kmers.js:46-54): {"key":count,...}, keys escaped as
// JSON.stringify does (\" \\ \b \f \n \r \t, other bytes < 0x20 as \u00XX).
// KMER_WRITE_LEGACY: the npm main's dump (lib/index.js:381-388):
// "{\n" then "key: count," per entry, then "}\n".
kmer_status kmer_result_write(const kmer_result *r, const char *path, uint32_t format) {
    if (!r || !path || format > KMER_WRITE_LEGACY) return KMER_E_BAD_PARAM;
    FILE *f = fopen(path, "wb");
    if (!f) return KMER_E_IO;
    std::string out;
    out.reserve(1 << 22);
    const uint64_t n = r->counts.size();
    char num[32];
    auto flush = [&]() -> bool {
        const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
        out.clear();
        return ok;
    };
    bool ok = true;
    out += format == KMER_WRITE_JSON ? "{" : "{\n";
    for (uint64_t i = 0; i < n && ok; ++i) {
        const char *k = r->keys.data() + r->offsets[i];
        const uint64_t kl = r->offsets[i + 1] - r->offsets[i];
        const int nl = snprintf(num, sizeof(num), "%llu", (unsigned long long)r->counts[i]);
        if (format == KMER_WRITE_JSON) {
            if (i) out += ',';
            out += '"';
            for (uint64_t j = 0; j < kl; ++j) {
                const unsigned char ch = (unsigned char)k[j];
                switch (ch) {
                case '"': out += "\\\""; break;
                case '\\': out += "\\\\"; break;
                case '\b': out += "\\b"; break;
                case '\f': out += "\\f"; break;
                case '\n': out += "\\n"; break;
                case '\r': out += "\\r"; break;
                case '\t': out += "\\t"; break;
                default:
                    if (ch < 0x20) {
                        char u[8];
                        snprintf(u, sizeof(u), "\\u%04x", ch);
                        out += u;
                    } else {
                        out += (char)ch;
                    }
                }
            }
            out += "\":";
            out.append(num, nl);
        } else {
            out.append(k, kl);
            out += ": ";
            out.append(num, nl);
            out += ',';
        }
        if (out.size() > (1u << 22)) ok = flush();
    }
    out += format == KMER_WRITE_JSON ? "}" : "}\n";
    ok = ok && flush();
    ok = (fclose(f) == 0) && ok;
    return ok ? KMER_OK : KMER_E_IO;
}

void kmer_result_free(kmer_result *r) { delete r; }

}  // extern "C"

// kmer_match_open_table (kmer_match.hip): see kmer_internal.hpp
static kmer_status table_view_impl(kmer_ctx *c, TabView *v, TabOwner *o) {
    SETTLE(c);                                       // (a group context: KMER_E_STATE)
    const kmer_status st = lookup_state(c);
    if (st) return st;
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, KMER_E_DEVICE, "hipSetDevice failed");
    o->stream = c->stream;
    o->device = c->device;
    o->k = c->p.k;
    o->n_cu = (uint32_t)std::max(c->n_cu, 1);
    o->empty = c->t_keys == 0;
    return o->empty ? KMER_OK : fill_view(c, v);
}

int kmerhip::table_view(kmer_ctx *c, TabView *v, TabOwner *o) { return (int)table_view_impl(c, v, o); }
