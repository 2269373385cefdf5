"""GPU parity of the table lookup (kmer_table_lookup / kmer_table_lookup_device,
kmer_lookup.hip): Map.get for batches of query keys against the device table.
Expected values come from the CPU restatement's Map (canonical counts derived
from it as test_table_gpu.py::_canonical_from_map does), never from the
library's own host result."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_LUT = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _LUT[_c] = _i
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_MUL = 0x9E3779B97F4A7C15                     # the documented hash multiplier (include/kmer_api.h)
_INV = pow(_MUL, -1, 1 << 64)


@pytest.fixture(scope="module")
def native():
    from kmerjs_amd import _native
    return _native


@pytest.fixture(scope="module")
def reads():
    """30,000 synthetic reads: (device buffer, the same bytes on the host)."""
    import torch
    from kmerjs_amd import synth_fastq_device
    n = 30_000
    buf = torch.empty(n * 317, dtype=torch.uint8, device="cuda")
    synth_fastq_device(buf.data_ptr(), 3, 0, n)
    torch.cuda.synchronize()
    return buf, buf.cpu().numpy().tobytes()


# ---- keys as digit rows (A C G T = 0 1 2 3) and as 2-bit codes in string order ----
def _pack(d):
    n, k = d.shape
    p = np.zeros((n, 32), dtype=np.uint8)
    p[:, 32 - k:] = d                                     # code = sum of d[j] << 2 (k - 1 - j)
    b = (p[:, 0::4] << 6) | (p[:, 1::4] << 4) | (p[:, 2::4] << 2) | p[:, 3::4]
    return np.ascontiguousarray(b).view(">u8").reshape(n).astype(np.uint64)


def _rc(d):
    return (3 - d[:, ::-1]).astype(np.uint8)


def _key_bytes(d):
    return _ACGT[d].tobytes()


@functools.lru_cache(maxsize=2)
def _oracle_raw(data, prefix, k):
    from oracle import oracle
    keys, cnt = oracle.count_arrays(data, prefix, k)
    d = _LUT[keys]
    assert (d < 4).all()                                  # an all-A/C/G/T input: no record keys
    return d, _pack(d), cnt.astype(np.uint64)


def _oracle_map(data, prefix, k, canonical):
    """The expected Map: (digit rows, counts) in Map order, and (codes, counts) sorted by code."""
    d, code, cnt = _oracle_raw(data, prefix, k)
    if canonical:                              # one key per class: the smaller string, counted per forward window
        r = _pack(_rc(d))
        keep = code <= r
        cnt = np.where(code == r, cnt // np.uint64(2), cnt)[keep]
        code, d = code[keep], d[keep]
    o = np.argsort(code)
    return d, cnt, code[o], cnt[o]


def _get(code_sorted, cnt_sorted, q):
    """Map.get(q, 0) for an array of query codes."""
    if len(code_sorted) == 0:
        return np.zeros(len(q), dtype=np.uint64)
    i = np.minimum(np.searchsorted(code_sorted, q), len(code_sorted) - 1)
    return np.where(code_sorted[i] == q, cnt_sorted[i], np.uint64(0)).astype(np.uint64)


def _batch(m, k, prefix, rng, n_absent=5000):
    """One scrambled batch and its expected answers: every Map key, present
    keys' reverse complements (no prefix: the Map holds both orientations of
    every class already, so a sixteenth of them), random k-mers, and keys that
    fail the prefix."""
    d, cnt, cs, cnts = m
    extra = [_rc(d if prefix else d[::16]), rng.integers(0, 4, (n_absent, k), dtype=np.uint8)]
    if prefix:
        bad = d[::max(1, len(d) // 5000)].copy()
        bad[:, 0] = (bad[:, 0] + rng.integers(1, 4, len(bad))) % 4
        extra.append(bad.astype(np.uint8))
    extra = np.concatenate(extra)
    q = np.concatenate([d, extra])
    want = np.concatenate([cnt, _get(cs, cnts, _pack(extra))])
    o = rng.permutation(len(q))
    return q[o], want[o]


def _ask_host(ctr, d):
    return ctr.table_lookup(_key_bytes(d))


def _ask_device(ctr, keys_bytes, n):
    import torch
    keys = torch.from_numpy(np.frombuffer(keys_bytes, dtype=np.uint8).copy()).cuda()
    out = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda").view(torch.uint64)
    ctr.table_lookup_device(keys.data_ptr() if n else 0, n, out.data_ptr() if n else 0,
                            torch.cuda.current_stream().cuda_stream)
    return out.cpu().numpy()[:n]


def _fed(native, buf, nbytes, k, prefix, flags, cuts=None):
    ctr = native.Counter(k=k, prefix=prefix, flags=flags)
    ctr.reset()
    cuts = cuts or [0, nbytes]
    for lo, hi in zip(cuts, cuts[1:]):
        ctr.feed_device(buf.data_ptr() + lo, hi - lo)
    ctr.finish(want_result=False)
    return ctr


def _check_all_ways(ctr, d, want, kb=None):
    """Host call, device call, host call again: all equal `want`; the table untouched.
    kb: the keys' bytes where they are not those of the digit rows d."""
    before = (ctr.table_digest(), ctr.table_stats())
    kb = _key_bytes(d) if kb is None else kb
    got = ctr.table_lookup(kb)
    assert got.dtype == np.uint64 and np.array_equal(got, want), int((got != want).sum())
    got = _ask_device(ctr, kb, len(d))
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(ctr.table_lookup(kb), want)
    assert (ctr.table_digest(), ctr.table_stats()) == before


# unordered: (31, ""), (32, "GT"), (22, ""), (21, "A"), (21, ""), (20, ""), (16, "ATGAC"), (15, "T"), (1, "");
# canonical: (21, ""), (21, "A"), (16, ""), (31, "") -- each next to its unordered twin (one oracle count for both)
MODES = [(31, b"", False), (31, b"", True), (32, b"GT", False), (22, b"", False), (21, b"A", False), (21, b"A", True),
         (21, b"", False), (21, b"", True), (20, b"", False), (16, b"ATGAC", False), (16, b"", True), (15, b"T", False),
         (1, b"", False)]


@pytest.mark.parametrize("k,prefix,canonical", MODES)
def test_lookup_encodings_and_modes(native, reads, k, prefix, canonical):
    # wide (k >= 22) and narrow keys, odd and even narrow k, both sides of k = 21 / 22
    buf, host = reads
    m = _oracle_map(host, prefix, k, canonical)
    ctr = _fed(native, buf, len(host), k, prefix, native.FLAG_CANONICAL if canonical else native.FLAG_UNORDERED)
    q, want = _batch(m, k, prefix, np.random.default_rng(k))
    _check_all_ways(ctr, q, want)
    ctr.close()


def _canonical_from_map(m):
    from oracle import oracle
    out = {}
    for key, v in m.items():
        rc = oracle.complement(key)
        if key <= rc:
            out[key] = v // 2 if key == rc else v
    return out


def _ask_list(ctr, keys):
    """The iterable route of the host call, and the device call over the same keys."""
    host = ctr.table_lookup(keys)
    assert isinstance(host, list) and len(host) == len(keys)
    dev = _ask_device(ctr, b"".join(keys), len(keys)).tolist()
    return host, dev


@pytest.mark.parametrize("k", [16, 15])
@pytest.mark.parametrize("prefix", [b"", b"A", b"T"])
def test_lookup_palindromes_and_big_counts(native, k, prefix):
    # one class seen > 2^20 times (its count is in the big list), and AT-repeat
    # palindromes at even k: doubled in the Map, undoubled in canonical mode
    from oracle import oracle
    polya = b"".join(b"@r%010d\n%s\n+\n%s\n" % (i, b"A" * 150, b"I" * 150) for i in range(9000))
    at = b"".join(b"@s%010d\n%s\n+\n%s\n" % (i, b"AT" * 75, b"I" * 150) for i in range(300))
    data = polya + at
    m = dict(oracle.count_buffer(data, prefix, k, 1))
    every = dict(oracle.count_buffer(data, b"", k, 1))
    rng = np.random.default_rng(k)
    keys = list(every) + [oracle.complement(x) for x in every] + [b"A" * k, b"T" * k, (b"AT" * k)[:k], (b"TA" * k)[:k]]
    keys += [_key_bytes(row[None, :]) for row in rng.integers(0, 4, (200, k), dtype=np.uint8)]
    keys = [keys[i] for i in rng.permutation(len(keys))]
    for canonical in (False, True):
        want_map = _canonical_from_map(m) if canonical else m
        want = [want_map.get(x, 0) for x in keys]
        ctr = native.Counter(k=k, prefix=prefix, flags=native.FLAG_CANONICAL if canonical else native.FLAG_UNORDERED)
        ctr.count_buffer(data)
        host, dev = _ask_list(ctr, keys)
        assert host == want and dev == want, (k, prefix, canonical)
        a, t = ctr.table_lookup([b"A" * k, b"T" * k])
        if k == 15 and not canonical:
            assert a == (9000 * 136 if prefix in (b"", b"A") else 0) and t == (9000 * 136 if prefix in (b"", b"T") else 0)
            assert 9000 * 136 > (1 << 20) - 1
        if k == 15 and canonical:
            assert a == (9000 * 136 if prefix in (b"", b"A") else 0) and t == 0
        if k == 16 and prefix in (b"", b"A"):
            pal = b"AT" * 8
            assert oracle.complement(pal) == pal
            got = ctr.table_lookup([pal])[0]
            assert got == (every[pal] // 2 if canonical else every[pal]) and got > 0 and every[pal] % 2 == 0
        ctr.close()


def _planar_digits(c, k):
    """Digit rows of planar codes (low plane: bits 0..k-1, high plane: bits k..2k-1)."""
    j = np.arange(k, dtype=np.uint64)
    lo = (c[:, None] >> j[None, :]) & np.uint64(1)
    hi = (c[:, None] >> (j[None, :] + np.uint64(k))) & np.uint64(1)
    return (2 * hi + lo).astype(np.uint8)


def _planar(d):
    k = d.shape[1]
    j = np.arange(k, dtype=np.uint64)
    lo = ((d & 1).astype(np.uint64) << j[None, :]).sum(axis=1, dtype=np.uint64)
    hi = ((d >> 1).astype(np.uint64) << j[None, :]).sum(axis=1, dtype=np.uint64)
    return (hi << np.uint64(k)) | lo


@pytest.mark.parametrize("split", [False, True])
def test_lookup_scans_a_long_bucket(native, split):
    """~5,000 distinct 31-mers that all fall into ONE bucket (the documented
    hash inverted on the CPU): the wave-cooperative scan over many rounds,
    which random small inputs (0-2 entries per bucket) never reach.  split:
    the table comes from the other final kernel (FLAG_TABLE_SPLIT_TEST)."""
    import torch
    from kmerjs_amd.multi import _CudaArray
    from oracle import oracle
    k, q = 31, 0x5A5A5
    rng = np.random.default_rng(31)
    rem = np.unique(rng.integers(0, 1 << 44, 120_000, dtype=np.uint64))
    rem = rem[rng.permutation(len(rem))]
    h = (np.uint64(q) << np.uint64(44)) | rem
    with np.errstate(over="ignore"):
        c = h * np.uint64(_INV)                           # (mod 2^64)
    ok = c < np.uint64(1 << 62)                           # a 31-mer's planar code ...
    c = c[ok]
    d = _planar_digits(c, k)
    canon = c <= _planar(_rc(d))                          # ... and the class's canonical one
    d = d[canon]
    assert len(d) >= 10_000
    written, absent = d[:5000], d[5000:10_000]
    recs = []
    for i, row in enumerate(written):
        rec = b"@r%d\n%s\n+\n%s\n" % (i, _key_bytes(row[None, :]), b"I" * k)
        recs.append(rec * (3 if i % 97 == 0 else 1))
    data = b"".join(recs)
    m = dict(oracle.count_buffer(data, b"", k, 1))
    assert len(m) == 2 * len(written)
    ctr = native.Counter(k=k, prefix=b"", flags=native.FLAG_UNORDERED | (native.FLAG_TABLE_SPLIT_TEST if split else 0))
    ctr.count_buffer(data)
    _, _, ln, _, _ = ctr.table_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    lens = torch.as_tensor(_CudaArray(ln, 1 << 20, "<i4"), device=dev)
    assert int(lens[q]) == len(written) and int(lens.sum()) == len(written)   # the test's point: one long bucket
    qs = np.concatenate([written, _rc(written), absent, _rc(absent)])
    qs = qs[rng.permutation(len(qs))]
    want = np.array([m.get(_key_bytes(row[None, :]), 0) for row in qs], dtype=np.uint64)
    assert (want == 3).sum() == 2 * len(range(0, 5000, 97)) and (want == 0).sum() == 10_000
    _check_all_ways(ctr, qs, want)
    # A second order, for a scan that works on runs of neighbouring queries of
    # one bucket: keys of the long bucket alternate, lane by lane, with random
    # k-mers (empty buckets) and keys holding a non-A/C/G/T byte, so that runs
    # of length 1 of the same bucket recur inside a wave; one present key is
    # asked 130 times in a row (a whole wave of one remainder, across a wave
    # edge); and the batch starts after 1 and after 63 other queries.
    n = 2000
    rows = _ACGT[np.stack([qs[:n], rng.integers(0, 4, (n, k), dtype=np.uint8), qs[n:2 * n]], axis=1)]
    rows[np.arange(n), 2, rng.integers(0, k, n)] = ord("N")
    rows = np.concatenate([rows[:n // 2].reshape(-1, k), np.repeat(_ACGT[written[97:98]], 130, axis=0),
                           rows[n // 2:].reshape(-1, k)])
    for shift in (1, 63):
        kb = np.concatenate([_ACGT[rng.integers(0, 4, (shift, k), dtype=np.uint8)], rows])
        want = np.array([m.get(row.tobytes(), 0) for row in kb], dtype=np.uint64)
        assert (want[shift + 3 * (n // 2):][:130] == 3).all() and (want[shift:][0::3][:n // 2] > 0).sum() > n // 8
        assert (want[shift:][2::3][:n // 2] == 0).all()
        _check_all_ways(ctr, kb, want, kb.tobytes())
    ctr.close()


def _n_rich(n_reads, seed):
    from oracle import oracle
    rng = np.random.default_rng(seed)
    arr = np.frombuffer(bytearray(oracle.synth_fastq(4, 0, n_reads)), dtype=np.uint8).reshape(-1, 317).copy()
    seq = arr[:, 13:163]
    seq[rng.random(seq.shape) < 0.002] = ord("N")
    seq[rng.random(len(seq)) < 0.8, 0] = ord("N")
    seq[rng.random(seq.shape) < 0.0005] = ord("a")
    arr[:, 13:163] = seq
    return arr.tobytes()


@pytest.mark.parametrize("k,prefix,canonical", [(16, b"", False), (21, b"GT", False), (21, b"", True), (16, b"A", True)])
def test_lookup_record_keys(native, inputs, k, prefix, canonical):
    # keys with N / lowercase / '\r': the host call answers their Map values from
    # the context's records, the device call answers 0 for them
    from oracle import oracle
    rng = np.random.default_rng(k)
    flags = native.FLAG_CANONICAL if canonical else native.FLAG_UNORDERED
    ctr = native.Counter(k=k, prefix=prefix, flags=flags)
    answered = 0
    for data in (_n_rich(600, 12), inputs["edge_exotic.fastq"]):
        m = dict(oracle.count_buffer(data, prefix, k, 1))
        if canonical:
            m = _canonical_from_map(m)
        keys = list(m) + [oracle.complement(x) for x in m]
        keys += [x[:-1] + b"N" for x in list(m)[:50]] + [x.lower() for x in list(m)[:50]]
        keys += [b"A" * (k - 1), b"A" * (k + 1), b""]                 # not k bytes: 0, without reaching the library
        keys = [keys[i] for i in rng.permutation(len(keys))]
        want = [m.get(x, 0) for x in keys]
        ctr.count_buffer(data)
        assert ctr.table_lookup(keys) == want
        full = [x for x in keys if len(x) == k]
        dev = _ask_device(ctr, b"".join(full), len(full)).tolist()
        assert dev == [m.get(x, 0) if all(ch in b"ACGT" for ch in x) else 0 for x in full]
        answered += sum(1 for x in full if m.get(x, 0) and any(ch not in b"ACGT" for ch in x))
    assert answered > 100                              # record keys the host call answered
    ctr.close()


def test_lookup_chunked_feeds_reuse_and_states(native, reads):
    import torch
    from oracle import oracle
    buf, host = reads
    k, n1 = 31, 317 * 8000
    first = host[:n1]
    m1 = _oracle_map(first, b"", k, False)
    ctr = native.Counter(k=k, prefix=b"", flags=native.FLAG_UNORDERED)
    with pytest.raises(native.KmerError) as e:         # no finish yet
        ctr.table_lookup(b"A" * k)
    assert e.value.status == 8
    ctr.reset()
    ctr.feed_device(buf.data_ptr(), 317 * 3000)
    ctr.feed_device(buf.data_ptr() + 317 * 3000, n1 - 317 * 3000)
    with pytest.raises(native.KmerError) as e:         # fed, not finished
        _ask_device(ctr, b"A" * k, 1)
    assert e.value.status == 8
    ctr.finish(want_result=False)
    rng = np.random.default_rng(5)
    q, want = _batch(m1, k, b"", rng)
    _check_all_ways(ctr, q, want)
    # n = 0: an empty answer, nothing touched
    assert len(ctr.table_lookup(b"")) == 0 and ctr.table_lookup([]) == []
    ctr.table_lookup_device(0, 0, 0)
    # the same context, another input: nothing of the first table survives
    second = oracle.synth_fastq(11, 0, 3000)
    m2 = _oracle_map(second, b"", k, False)
    buf2 = torch.frombuffer(bytearray(second), dtype=torch.uint8).cuda()
    ctr.reset()
    with pytest.raises(native.KmerError) as e:
        ctr.table_lookup(b"A" * k)
    assert e.value.status == 8
    ctr.feed_device(buf2.data_ptr(), len(second))
    ctr.finish(want_result=False)
    qb, wb = _batch(m2, k, b"", rng)
    q2 = np.concatenate([q[::4], qb])
    want2 = np.concatenate([_get(m2[2], m2[3], _pack(q[::4])), wb])
    assert (want2[:len(q[::4])] == 0).sum() > 1000
    _check_all_ways(ctr, q2, want2)
    ctr.close()
    ordered = native.Counter(k=16, prefix=b"ATGAC")    # an ordered-mode context has no table
    ordered.count_buffer(first)
    with pytest.raises(native.KmerError) as e:
        ordered.table_lookup(b"A" * 16)
    assert e.value.status == 8
    with pytest.raises(native.KmerError) as e:
        _ask_device(ordered, b"A" * 16, 1)
    assert e.value.status == 8
    ordered.close()


@pytest.mark.parametrize("k,prefix,canonical", [(31, b"", False), (21, b"A", True)])
def test_lookup_on_a_group(native, reads, k, prefix, canonical):
    # devices=[0, 0]: the children hold disjoint slices of the hash space, their answers add
    buf, host = reads
    flags = native.FLAG_CANONICAL if canonical else native.FLAG_UNORDERED
    q, want = _batch(_oracle_map(host, prefix, k, canonical), k, prefix, np.random.default_rng(k + 100))
    one = _fed(native, buf, len(host), k, prefix, flags)
    assert np.array_equal(_ask_host(one, q), want)     # the single-context answers
    one.close()
    grp = native.Counter(k=k, prefix=prefix, flags=flags, devices=[0, 0])
    # (kmer_count_buffer itself: its host result -- 7.2 M entries at k = 31 -- is freed, not copied to Python)
    r = ctypes.c_void_p()
    assert native.LIB.kmer_count_buffer(grp.h, host, len(host), ctypes.byref(r)) == 0
    native.LIB.kmer_result_free(r)
    before = (grp.table_digest(), grp.table_stats())
    assert np.array_equal(_ask_host(grp, q), want)
    assert np.array_equal(_ask_host(grp, q), want)
    assert (grp.table_digest(), grp.table_stats()) == before
    with pytest.raises(native.KmerError) as e:         # device-resident calls are single-device only
        _ask_device(grp, _key_bytes(q[:4]), 4)
    assert e.value.status == 8
    grp.close()


@pytest.mark.parametrize("k,flags_name", [(31, "FLAG_UNORDERED"), (21, "FLAG_CANONICAL")])
def test_lookup_on_exchanged_tables(native, reads, k, flags_name):
    """World 2 in one process (the pattern of test_table_exchange_matches_one_table):
    each rank's table holds its buckets only, keys it does not own answer 0,
    so the ranks' answers add up to the one-table answers."""
    import torch
    from kmerjs_amd.multi import device_u64
    buf, host = reads
    world, n_reads = 2, 30_000
    flags = getattr(native, flags_name)
    canonical = flags_name == "FLAG_CANONICAL"
    m = _oracle_map(host, b"", k, canonical)
    q, want = _batch(m, k, b"", np.random.default_rng(k + 200))
    cuts = [317 * (n_reads * r // world) for r in range(world + 1)]
    ctrs = [native.Counter(k=k, prefix=b"", flags=flags) for _ in range(world)]
    sends = []
    for r, c in enumerate(ctrs):
        c.reset()
        c.feed_device(buf.data_ptr() + cuts[r], cuts[r + 1] - cuts[r])
        d, counts, parts = c.table_exchange_prepare(world)
        keys = device_u64(d, sum(counts), buf.device).clone()
        sends.append((keys, counts, parts))
    parts_all = np.array([p for _, _, p in sends], dtype=np.uint64)
    recvs, got = [], []
    for o, c in enumerate(ctrs):
        recv = torch.cat([keys[sum(counts[:o]):sum(counts[:o]) + counts[o]] for keys, counts, _ in sends])
        recvs.append(recv)
        c.table_finish_exchanged(recv.data_ptr(), recv.numel(), parts_all, world, o,
                                 stream=torch.cuda.current_stream().cuda_stream)
    for c in ctrs:
        host_ans = _ask_host(c, q)
        assert np.array_equal(_ask_device(c, _key_bytes(q), len(q)), host_ans)
        got.append(host_ans)
    assert np.array_equal(got[0] + got[1], want)
    present = want != 0
    assert present.sum() >= len(m[0])
    assert (((got[0] != 0).astype(int) + (got[1] != 0).astype(int))[present] == 1).all()
    assert (got[0] != 0).any() and (got[1] != 0).any()
    for c in ctrs:
        c.close()
    del recvs


def test_lookup_leaves_the_table_untouched(native, reads):
    buf, host = reads
    n = 317 * 4000
    ctr = _fed(native, buf, n, 21, b"", native.FLAG_CANONICAL)
    before = (ctr.table_digest(), ctr.table_stats())
    q, want = _batch(_oracle_map(host[:n], b"", 21, True), 21, b"", np.random.default_rng(8))
    for _ in range(2):
        assert np.array_equal(_ask_host(ctr, q), want)
        assert (ctr.table_digest(), ctr.table_stats()) == before
        assert np.array_equal(_ask_device(ctr, _key_bytes(q), len(q)), want)
        assert (ctr.table_digest(), ctr.table_stats()) == before
    ctr.close()
