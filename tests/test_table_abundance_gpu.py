"""GPU parity of the table's by-value readers (kmer_table_spectrum,
kmer_table_extract_device, kmer_table_extract; kmer_abundance.hip) and of the
matcher's min_count route.  Every comparison is exact.  Expected values come
from the CPU restatement's Map (canonical counts derived from it as
test_table_lookup_gpu.py::_oracle_map does), never from the library's own host
result -- but for the one test that says it compares against it."""
import ctypes

import numpy as np
import pytest

from oracle import kmerfinder_oracle as ko
from tests import test_table_lookup_gpu as L

pytestmark = pytest.mark.gpu

N_READS = 3000
MAX_BINS = 1 << 21


@pytest.fixture(scope="module")
def native():
    from kmerjs_amd import _native
    return _native


@pytest.fixture(scope="module")
def kf():
    from kmerjs_amd import kmerfinder
    return kmerfinder


def _host_input():
    from oracle import oracle
    raw = oracle.synth_fastq(3, 0, N_READS)
    return b"".join(raw[317 * i:317 * (i + 1)] * (i % 5 + 1) for i in range(N_READS))


@pytest.fixture(scope="module")
def data():
    """3,000 synthetic reads, read i repeated i % 5 + 1 times (9,000 records,
    2.85 MB): (device buffer, the same bytes on the host)."""
    import torch
    host = _host_input()
    assert len(host) == 9000 * 317
    return torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda(), host


_MAPS = {}


def _omap(host, prefix, k, canonical):
    """The expected Map of the module's input, sorted by key bytes: (digit rows, 2-bit codes, values)."""
    from oracle import oracle
    if (prefix, k) not in _MAPS:
        keys, cnt = oracle.count_arrays(host, prefix, k)
        d = L._LUT[keys]
        assert (d < 4).all()                                  # an all-A/C/G/T input: no record keys
        _MAPS.clear()                                         # (one Map at a time: k = 31 holds 1.4 M rows)
        _MAPS[(prefix, k)] = (d, L._pack(d), cnt.astype(np.uint64))
    d, code, cnt = _MAPS[(prefix, k)]
    if canonical:                              # one key per class: the smaller string, counted per forward window
        r = L._pack(L._rc(d))
        keep = code <= r
        cnt = np.where(code == r, cnt // np.uint64(2), cnt)[keep]
        code, d = code[keep], d[keep]
    o = np.argsort(code)
    return d[o], code[o], cnt[o]


def _fold(values, nbins):
    """(hist, top_sum) of a Map's values: np.bincount with the last bin open."""
    v = np.asarray(values, dtype=np.uint64)
    hist = np.bincount(np.minimum(v, np.uint64(nbins - 1)).astype(np.int64), minlength=nbins).astype(np.uint64)
    return hist, int(v[v >= np.uint64(nbins - 1)].sum(dtype=np.uint64))


def _check_spectrum(native, ctr, values, nbins_list):
    canon, keys, total = ctr.table_stats()
    for nbins in nbins_list:
        hist, top = ctr.table_spectrum(nbins)
        want, want_top = _fold(values, nbins)
        assert hist.dtype == np.uint64 and len(hist) == nbins
        assert np.array_equal(hist, want), (nbins, np.nonzero(hist != want)[0][:8])
        assert top == want_top and hist[0] == 0
        # the two identities against kmer_table_stats
        assert int(hist.sum()) == keys == len(values)
        v = np.arange(nbins - 1, dtype=np.uint64)
        assert int((v * hist[:-1]).sum(dtype=np.uint64)) + top == total


def _flags(native, canonical, extra=0):
    return (native.FLAG_CANONICAL if canonical else native.FLAG_UNORDERED) | extra


def _nbins_list(native):
    R, B = native.SPECTRUM_REG_MAX, native.SPECTRUM_LDS_BINS
    return [2, 4, B - 96, B + 904, MAX_BINS], R, B


# (k, prefix): wide and narrow keys, both sides of k = 21 / 22, odd and even k, with and without a prefix;
# k = 6 / 4 / 3: a few hundred keys with values in the hundreds, above 10,000 and above 40,000
SHAPES = [(31, b""), (22, b"AC"), (21, b""), (21, b"AC"), (16, b"ATGAC"), (32, b"T"), (6, b""), (4, b"A"), (3, b"")]


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,prefix", SHAPES)
def test_spectrum_equals_bincount_of_the_oracle_map(native, data, k, prefix, canonical):
    buf, host = data
    _, _, cnt = _omap(host, prefix, k, canonical)
    nbins, R, B = _nbins_list(native)
    # the shapes straddle the kernel's tiers: registers (<= R), LDS (< B), global atomics
    if k == 31:
        assert sorted(set(cnt.tolist())) == [1, 2, 3, 4, 5] and (cnt <= R).any() and (cnt > R).any()
        assert len(cnt) == (360_000 if canonical else 720_000)   # 144,000 Map keys per bin
    if k == 6:
        assert ((cnt > R) & (cnt < B)).sum() > 100 and len(set(cnt.tolist())) > 100
    if k in (4, 3):
        assert (cnt >= B).any() and cnt.max() < MAX_BINS - 1
    for cuts in (None, [0, 317 * 2999, 317 * 3000, len(host)]):     # fed whole, and in three chunks
        ctr = L._fed(native, buf, len(host), k, prefix, _flags(native, canonical), cuts=cuts)
        _check_spectrum(native, ctr, cnt, nbins if cuts is None else nbins[1:4])
        ctr.close()


@pytest.mark.parametrize("route", ["fixed", "split"])
@pytest.mark.parametrize("k,prefix,canonical", [(31, b"", False), (21, b"AC", True)])
def test_spectrum_and_extract_on_the_other_routes(native, data, k, prefix, canonical, route):
    # fixed: pass 2 runs with fixed-capacity regions (nd[q] counts a bucket's entries, the
    # starts bound its region) and, without a prefix, pass 1 writes fixed runs with filler
    # slots; split: the table comes from the general final kernel
    buf, host = data
    d, code, cnt = _omap(host, prefix, k, canonical)
    extra = native.FLAG_TABLE_FIXED_TEST if route == "fixed" else native.FLAG_TABLE_SPLIT_TEST
    ctr = L._fed(native, buf, len(host), k, prefix, _flags(native, canonical, extra))
    if route == "fixed":
        routes = ctr.table_routes()
        assert routes["p2_fixed"] == 1 and (prefix or routes["fixed"] >= 1), routes
    _check_spectrum(native, ctr, cnt, _nbins_list(native)[0][1:4])
    keys, got = _device_extract(ctr, 3, 4)
    sel = (cnt >= 3) & (cnt <= 4)
    assert keys == L._key_bytes(d[sel]) and np.array_equal(got, cnt[sel]) and sel.sum() > 100
    ctr.close()


def _device_extract(ctr, lo=1, hi=0):
    """table_extract_device copied to the host through torch: (key bytes, values)."""
    import torch
    from kmerjs_amd.multi import _CudaArray, device_u64
    d_keys, d_counts, n = ctr.table_extract_device(lo, hi)
    if n == 0:
        return b"", np.zeros(0, dtype=np.uint64)
    assert d_keys and d_counts
    dev = torch.device("cuda", torch.cuda.current_device())
    keys = torch.as_tensor(_CudaArray(d_keys, n * ctr.k, "|u1"), device=dev).cpu().numpy().tobytes()
    cnt = device_u64(d_counts, n, dev).cpu().numpy().view(np.uint64).copy()
    return keys, cnt


RANGES = [(1, 0), (2, 0), (3, 4), (5, 5), (6, 0), (4, 2)]


@pytest.mark.parametrize("k,prefix,canonical", [(21, b"", False), (21, b"", True), (22, b"AC", False), (32, b"T", False),
                                                (16, b"ATGAC", False), (6, b"", False), (21, b"AC", True)])
def test_extract_equals_the_oracle_rows_in_range(native, data, k, prefix, canonical):
    buf, host = data
    d, code, cnt = _omap(host, prefix, k, canonical)
    ctr = L._fed(native, buf, len(host), k, prefix, _flags(native, canonical))
    for lo, hi in RANGES:
        sel = (cnt >= max(lo, 1)) & ((cnt <= hi) if hi else True)
        if hi and hi < lo:
            sel = np.zeros(len(cnt), dtype=bool)
        if (lo, hi) == (6, 0) and k > 6:
            assert not sel.any()                              # selects nothing
        want_keys, want_cnt = L._key_bytes(d[sel]), cnt[sel]
        keys, got = _device_extract(ctr, lo, hi)
        assert len(got) == int(sel.sum()) and keys == want_keys and np.array_equal(got, want_cnt), (lo, hi)
        keys2, got2 = _device_extract(ctr, lo, hi)            # again: the same bytes (the first call's pointers are gone)
        assert keys2 == keys and np.array_equal(got2, got)
        if (lo, hi) in ((2, 0), (3, 4), (6, 0)):              # the host call: the same rows (no record keys in this input)
            r = ctr.table_extract(lo, hi)
            assert r.keybuf == want_keys and np.array_equal(r.counts, want_cnt) and r.lines == 4 * 9000
            assert np.array_equal(r.offsets, np.arange(len(want_cnt) + 1, dtype=np.uint64) * np.uint64(k))
        if (lo, hi) == (2, 0):
            assert len(got) > 100
    assert _device_extract(ctr, 0, 0)[0] == L._key_bytes(d)   # lo 0 is 1: the whole Map
    ctr.close()


def _long_bucket_input(k=31, q=0x5A5A5):
    """~5,000 distinct 31-mers of ONE bucket (test_lookup_scans_a_long_bucket's
    construction), record i repeated i % 7 + 1 times."""
    rng = np.random.default_rng(31)
    rem = np.unique(rng.integers(0, 1 << 44, 120_000, dtype=np.uint64))
    rem = rem[rng.permutation(len(rem))]
    h = (np.uint64(q) << np.uint64(44)) | rem
    with np.errstate(over="ignore"):
        c = h * np.uint64(L._INV)
    c = c[c < np.uint64(1 << 62)]
    d = L._planar_digits(c, k)
    d = d[c <= L._planar(L._rc(d))][:5000]
    assert len(d) == 5000
    recs = [(b"@r%d\n%s\n+\n%s\n" % (i, L._key_bytes(row[None, :]), b"I" * k)) * (i % 7 + 1) for i, row in enumerate(d)]
    return b"".join(recs), len(d)


@pytest.mark.parametrize("split", [False, True])
def test_spectrum_and_extract_walk_a_long_bucket(native, split):
    import torch
    from kmerjs_amd.multi import _CudaArray
    from oracle import oracle
    k, q = 31, 0x5A5A5
    text, n = _long_bucket_input(k, q)
    m = dict(oracle.count_buffer(text, b"", k, 1))
    assert len(m) == 2 * n
    ctr = native.Counter(k=k, prefix=b"", flags=native.FLAG_UNORDERED | (native.FLAG_TABLE_SPLIT_TEST if split else 0))
    ctr.count_buffer(text)
    _, _, ln, _, _ = ctr.table_device()
    lens = torch.as_tensor(_CudaArray(ln, 1 << 20, "<i4"), device=torch.device("cuda", torch.cuda.current_device()))
    assert int(lens[q]) == n and int(lens.sum()) == n        # one long bucket: ten wave rounds, the last one ragged
    assert n % 512 != 0 and n > 9 * 512
    rows = sorted(m.items())
    values = [v for _, v in rows]
    assert sorted(set(values)) == [1, 2, 3, 4, 5, 6, 7]
    _check_spectrum(native, ctr, values, [2, 6, 256])
    for lo, hi in ((1, 0), (5, 6), (7, 0)):
        want = [(x, v) for x, v in rows if v >= lo and (hi == 0 or v <= hi)]
        keys, got = _device_extract(ctr, lo, hi)
        assert keys == b"".join(x for x, _ in want) and got.tolist() == [v for _, v in want] and len(want) > 1000
    ctr.close()


@pytest.mark.parametrize("k,prefix", [(15, b""), (16, b"A"), (16, b"")])
def test_big_counts_in_the_spectrum_and_the_extract(native, k, prefix):
    # one class seen > 2^20 times (its count lies in the big list), and AT-repeat palindromes at even k
    from oracle import oracle
    polya = b"".join(b"@r%010d\n%s\n+\n%s\n" % (i, b"A" * 150, b"I" * 150) for i in range(9000))
    at = b"".join(b"@s%010d\n%s\n+\n%s\n" % (i, b"AT" * 75, b"I" * 150) for i in range(300))
    text = polya + at
    m = dict(oracle.count_buffer(text, prefix, k, 1))
    big = 9000 * (151 - k)
    assert big >= (1 << 20) - 1 and m[b"A" * k] == big
    for canonical in (False, True):
        want = L._canonical_from_map(m) if canonical else m
        rows = sorted(want.items())
        values = [v for _, v in rows]
        ctr = native.Counter(k=k, prefix=prefix, flags=_flags(native, canonical))
        ctr.count_buffer(text)
        _check_spectrum(native, ctr, values, [2, 8, 5000, MAX_BINS])
        hist, top = ctr.table_spectrum(MAX_BINS)
        assert hist[big] == values.count(big) >= 1            # at its true value ...
        hist, top = ctr.table_spectrum(8)
        assert hist[7] == sum(1 for v in values if v >= 7) and top == sum(v for v in values if v >= 7) >= big
        keys, got = _device_extract(ctr, 1 << 20, 0)          # ... and extracted with its true count
        hot = [(x, v) for x, v in rows if v >= 1 << 20]
        assert keys == b"".join(x for x, _ in hot) and got.tolist() == [v for _, v in hot] and big in got.tolist()
        keys, got = _device_extract(ctr)
        assert keys == b"".join(x for x, _ in rows) and got.tolist() == values
        ctr.close()


@pytest.mark.parametrize("k,prefix,canonical", [(16, b"", False), (21, b"GT", False), (21, b"", True), (16, b"A", True)])
def test_record_keys_in_the_spectrum_and_the_host_extract(native, inputs, k, prefix, canonical):
    # keys with N / lowercase / '\r' live on the host: in the spectrum and the host
    # extract, absent from the device extract
    from oracle import oracle
    ctr = native.Counter(k=k, prefix=prefix, flags=_flags(native, canonical))
    seen = 0
    for text in (L._n_rich(600, 12), inputs["edge_exotic.fastq"]):
        m = dict(oracle.count_buffer(text, prefix, k, 1))
        if canonical:
            m = L._canonical_from_map(m)
        rows = sorted(m.items())
        acgt = [(x, v) for x, v in rows if all(ch in b"ACGT" for ch in x)]
        seen += len(rows) - len(acgt)
        ctr.count_buffer(text)
        _check_spectrum(native, ctr, [v for _, v in rows], [2, 3, 64])
        for lo, hi in ((1, 0), (2, 0), (1, 1), (2, 3)):
            inr = lambda v: v >= lo and (hi == 0 or v <= hi)
            r = ctr.table_extract(lo, hi)
            assert r.entries() == [(x, v) for x, v in rows if inr(v)], (lo, hi)
            keys, got = _device_extract(ctr, lo, hi)
            assert keys == b"".join(x for x, v in acgt if inr(v)) and got.tolist() == [v for _, v in acgt if inr(v)]
    assert seen > 100                                         # record keys there were
    ctr.close()


def test_host_extract_equals_the_host_result_filtered(native, inputs):
    """The one comparison against the library's own host result: table_extract(lo, hi)
    is kmer_count_buffer's result restricted to the values in range, row for row."""
    for k, prefix, canonical in ((16, b"ATGAC", False), (21, b"", True), (16, b"", False)):
        for text in (L._n_rich(600, 12), _host_input()[:317 * 2500]):
            ctr = native.Counter(k=k, prefix=prefix, flags=_flags(native, canonical))
            res = ctr.count_buffer(text)
            rows = res.entries()
            assert rows == sorted(rows)
            for lo, hi in ((1, 0), (2, 0), (2, 3), (4, 2)):
                r = ctr.table_extract(lo, hi)
                assert r.entries() == [(x, v) for x, v in rows if v >= lo and (hi == 0 or v <= hi) and not (hi and hi < lo)]
                assert r.lines == res.lines
            ctr.close()


def test_empty_tables_states_and_reuse(native, data):
    buf, host = data
    k = 21
    ctr = native.Counter(k=k, prefix=b"", flags=native.FLAG_UNORDERED)
    calls = (lambda c: c.table_spectrum(16), lambda c: c.table_extract_device(1, 0), lambda c: c.table_extract(1, 0))
    for call in calls:                                        # no finish yet
        with pytest.raises(native.KmerError) as e:
            call(ctr)
        assert e.value.status == 8
    ctr.reset()
    ctr.feed_device(buf.data_ptr(), 317 * 100)
    for call in calls:                                        # fed, not finished
        with pytest.raises(native.KmerError) as e:
            call(ctr)
        assert e.value.status == 8
    ctr.finish(want_result=False)
    assert ctr.table_extract_device()[2] > 0
    ctr.reset()                                               # an empty input
    ctr.finish(want_result=False)
    hist, top = ctr.table_spectrum(16)
    assert not hist.any() and top == 0 and len(hist) == 16
    assert ctr.table_extract_device(1, 0) == (0, 0, 0) and len(ctr.table_extract(1, 0)) == 0
    # after a reset and a second count: the second count's Map
    n2 = 317 * 4000
    d, code, cnt = _second_map(host[:n2], k)
    ctr.reset()
    ctr.feed_device(buf.data_ptr(), n2)
    ctr.finish(want_result=False)
    _check_spectrum(native, ctr, cnt, [2, 64])
    keys, got = _device_extract(ctr, 2, 0)
    assert keys == L._key_bytes(d[cnt >= 2]) and np.array_equal(got, cnt[cnt >= 2]) and len(got) > 1000
    ctr.close()
    ordered = native.Counter(k=16, prefix=b"ATGAC")           # an ordered-mode context has no table
    ordered.count_buffer(host[:317 * 500])
    for call in calls:
        with pytest.raises(native.KmerError) as e:
            call(ordered)
        assert e.value.status == 8
    ordered.close()
    ctr = native.Counter(k=k, prefix=b"", flags=native.FLAG_UNORDERED)
    ctr.count_buffer(host[:317 * 500])
    for bad in (0, 1, MAX_BINS + 1):                          # nbins outside [2, 2^21]
        with pytest.raises(native.KmerError) as e:
            ctr.table_spectrum(bad)
        assert e.value.status == 2
    ctr.close()


def _second_map(text, k):
    from oracle import oracle
    keys, cnt = oracle.count_arrays(text, b"", k)
    d = L._LUT[keys]
    code = L._pack(d)
    o = np.argsort(code)
    return d[o], code[o], cnt.astype(np.uint64)[o]


@pytest.mark.parametrize("k,prefix,canonical", [(31, b"", False), (21, b"A", True)])
def test_spectrum_and_extract_on_a_group(native, data, k, prefix, canonical):
    # devices=[0, 0]: the children hold disjoint classes; their histograms add, their extracts merge by key
    buf, host = data
    d, code, cnt = _omap(host, prefix, k, canonical)
    grp = native.Counter(k=k, prefix=prefix, flags=_flags(native, canonical), devices=[0, 0])
    r = ctypes.c_void_p()
    assert native.LIB.kmer_count_buffer(grp.h, host, len(host), ctypes.byref(r)) == 0
    lines = native.LIB.kmer_result_lines(r)
    native.LIB.kmer_result_free(r)
    before = (grp.table_digest(), grp.table_stats())
    _check_spectrum(native, grp, cnt, [2, 4, 256])
    sel = cnt >= 4
    res = grp.table_extract(4, 0)
    assert res.keybuf == L._key_bytes(d[sel]) and np.array_equal(res.counts, cnt[sel]) and res.lines == lines == 36000
    assert (grp.table_digest(), grp.table_stats()) == before
    with pytest.raises(native.KmerError) as e:                # the device extract is single-device only
        grp.table_extract_device(1, 0)
    assert e.value.status == 8
    grp.close()


@pytest.mark.parametrize("k,flags_name", [(31, "FLAG_UNORDERED"), (21, "FLAG_CANONICAL")])
def test_spectrum_and_extract_on_exchanged_tables(native, data, k, flags_name):
    """World 2 in one process (test_lookup_on_exchanged_tables' construction): each
    rank's table describes its own share, so the histograms add up to the whole
    and the two extracts are disjoint and merge to the whole."""
    import torch
    from kmerjs_amd.multi import device_u64
    buf, host = data
    world, n_rec = 2, 9000
    canonical = flags_name == "FLAG_CANONICAL"
    d, code, cnt = _omap(host, b"", k, canonical)
    cuts = [317 * (n_rec * r // world) for r in range(world + 1)]
    ctrs = [native.Counter(k=k, prefix=b"", flags=getattr(native, flags_name)) for _ in range(world)]
    sends = []
    for r, c in enumerate(ctrs):
        c.reset()
        c.feed_device(buf.data_ptr() + cuts[r], cuts[r + 1] - cuts[r])
        dsend, counts, parts = c.table_exchange_prepare(world)
        sends.append((device_u64(dsend, sum(counts), buf.device).clone(), counts, parts))
    parts_all = np.array([p for _, _, p in sends], dtype=np.uint64)
    recvs = []
    for o, c in enumerate(ctrs):
        recv = torch.cat([keys[sum(counts[:o]):sum(counts[:o]) + counts[o]] for keys, counts, _ in sends])
        recvs.append(recv)
        c.table_finish_exchanged(recv.data_ptr(), recv.numel(), parts_all, world, o,
                                 stream=torch.cuda.current_stream().cuda_stream)
    nbins = 8
    hists = [c.table_spectrum(nbins) for c in ctrs]
    want, want_top = _fold(cnt, nbins)
    assert np.array_equal(hists[0][0] + hists[1][0], want) and hists[0][1] + hists[1][1] == want_top
    assert hists[0][0].any() and hists[1][0].any()
    ex = [_device_extract(c, 2, 0) for c in ctrs]
    rows = [[(kb[i * k:(i + 1) * k], int(v)) for i, v in enumerate(vals)] for kb, vals in ex]
    assert rows[0] == sorted(rows[0]) and rows[1] == sorted(rows[1]) and rows[0] and rows[1]
    assert not set(x for x, _ in rows[0]) & set(x for x, _ in rows[1])
    merged = sorted(rows[0] + rows[1])
    sel = cnt >= 2
    assert b"".join(x for x, _ in merged) == L._key_bytes(d[sel]) and [v for _, v in merged] == cnt[sel].tolist()
    for c in ctrs:
        c.close()
    del recvs


def test_spectrum_and_extract_leave_the_table_untouched(native, data):
    buf, host = data
    k = 21
    d, code, cnt = _omap(host, b"", k, True)
    ctr = L._fed(native, buf, len(host), k, b"", native.FLAG_CANONICAL)
    before = (ctr.table_digest(), ctr.table_stats())
    q = d[::7]
    for _ in range(2):
        ctr.table_spectrum(64)
        assert (ctr.table_digest(), ctr.table_stats()) == before
        ctr.table_extract_device(2, 4)
        ctr.table_extract(5, 0)
        assert (ctr.table_digest(), ctr.table_stats()) == before
        assert np.array_equal(ctr.table_lookup(L._key_bytes(q)), cnt[::7])    # a lookup still answers right
    ctr.close()


@pytest.mark.parametrize("k,prefix,canonical", [(21, b"", True), (22, b"AC", False)])
def test_find_matches_table_with_a_minimum_count(native, kf, data, k, prefix, canonical):
    """find_matches_table(counter, min_count=3) = the oracle restatement of kmerFinder
    over the oracle Map filtered to v >= 3 and sorted by bytes (the reference's
    `v >= coverage`); min_count=1 is the table probe, as before."""
    from tests import test_match_table_gpu as T
    buf, host = data
    d, code, cnt = _omap(host, prefix, k, canonical)
    whole = (d, cnt, code, cnt)                               # (the tuple test_table_lookup_gpu._oracle_map returns)
    keep = cnt >= 3
    cut = (d[keep], cnt[keep], code[keep], cnt[keep])
    db = T._winner_db(whole, k, np.random.default_rng(k))     # templates hold keys of every value, 1 .. 5
    summary = T._summary(db)
    tdb = kf.TemplateDB(db, k, summary)
    ctr = L._fed(native, buf, len(host), k, prefix, _flags(native, canonical))
    q0 = T._query(cut, db, k)
    assert 0 < len(q0) < len(T._query(whole, db, k)) and min(q0.values()) >= 3
    size = int(keep.sum())                                    # kmerMapSize of the filtered Map
    qo = dict(q0)
    want = ko.winner_scoring(qo, db, summary, size)
    assert len(want) >= 3                                     # the loop is not vacuous
    deleted = sorted(km.encode() for km in q0 if km not in qo)
    assert len(deleted) >= 3 * 100
    got, removed = kf.KmerFinder(tdb, "winner").find_matches_table(ctr, with_removed=True, min_count=3)
    assert got == want and removed == deleted
    assert kf.KmerFinder(tdb, "winner").find_matches_table(ctr, min_count=3) == want
    assert kf.KmerFinder(tdb, "winner").find_matches_table(ctr, query_size=size, min_count=3) == want
    assert kf.KmerFinder(tdb, "standard").find_matches_table(ctr, min_count=3) == ko.standard_scoring(dict(q0), db, summary, size)
    # min_count = 1: exactly what the table probe returns
    full = T._query(whole, db, k)
    want1 = ko.winner_scoring(dict(full), db, summary, len(cnt))
    assert kf.KmerFinder(tdb, "winner").find_matches_table(ctr, min_count=1) == want1
    assert kf.KmerFinder(tdb, "winner").find_matches_table(ctr) == want1 and want1 != want
    ctr.close()
    tdb.close()
