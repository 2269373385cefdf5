"""GPU parity of the read screen (kmer_table_screen / kmer_table_screen_device,
kmer_screen.hip): per read {windows, hits, skipped, sum} against a finished
table.  Every case goes through the device call with the direct and with the
sorted route and through the host call; all must agree.  Expected values come
from the oracle: the table's Map from oracle.count_arrays of the table's input,
a read's own Map from oracle.count_buffer of that record alone (canonical
counts derived from it as test_table_gpu.py::_canonical_from_map does).  Bulk
cases use a numpy restatement of the definition (the sums over the read's own
Map, window by window), checked against the oracle on a sample.  Nothing is
taken from the library's own host result."""
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
_M64 = (1 << 64) - 1
MIN_COUNTS = (1, 2, 3, 1 << 40)
E_BAD_PARAM, E_NONASCII, E_STATE = 2, 6, 8


@pytest.fixture(scope="module")
def native():
    from kmerjs_amd import _native
    return _native


def _synth(seed, first, n):
    from oracle import oracle
    return oracle.synth_fastq(seed, first, n)


@pytest.fixture(scope="module")
def table_input():
    """3,000 synthetic reads: the table's input."""
    return _synth(3, 0, 3000)


@pytest.fixture(scope="module")
def screened_input():
    """2,000 reads: half from the table's range, half from another seed."""
    return _synth(3, 1000, 1000) + _synth(9, 0, 1000)


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


def _synth_digits(data):
    arr = np.frombuffer(data, dtype=np.uint8).reshape(-1, 317)[:, 13:163]
    d = _LUT[arr]
    assert (d < 4).all()
    return d


def _table_map(data, prefix, k, canonical):
    """T, the table's expected Map over A/C/G/T keys: (codes ascending, values)."""
    from oracle import oracle
    keys, cnt = oracle.count_arrays(data, prefix, k)
    d = _LUT[keys]
    assert (d < 4).all()                                  # an all-A/C/G/T input: no record keys
    code, cnt = _pack(d), cnt.astype(np.uint64)
    if canonical:                              # one key per class: the smaller string, counted per forward window
        r = _pack(_rc(d))
        keep = code <= r
        cnt = np.where(code == r, cnt // np.uint64(2), cnt)[keep]
        code = code[keep]
    o = np.argsort(code)
    return code[o], cnt[o]


def _get(T, q):
    """T.get(q, 0) for an array of query codes."""
    cs, cnts = T
    q = np.asarray(q, dtype=np.uint64)
    if len(cs) == 0 or q.size == 0:
        return np.zeros(q.shape, dtype=np.uint64)
    i = np.minimum(np.searchsorted(cs, q.ravel()), len(cs) - 1)
    return np.where(cs[i] == q.ravel(), cnts[i], np.uint64(0)).astype(np.uint64).reshape(q.shape)


def _window_codes(d, k):
    """The codes of every forward window of equal-length A/C/G/T reads and of its reverse complement: (n, W) each."""
    n, L = d.shape
    if L < k or L <= 1:
        z = np.zeros((n, 0), dtype=np.uint64)
        return z, z
    win = np.lib.stride_tricks.sliding_window_view(d, k, axis=1)          # (n, W, k)
    sh = (2 * (k - 1 - np.arange(k))).astype(np.uint64)
    fw = (win.astype(np.uint64) << sh).sum(axis=2, dtype=np.uint64)
    rc = ((3 - win[..., ::-1]).astype(np.uint64) << sh).sum(axis=2, dtype=np.uint64)
    return fw, rc


def _model_rows(d, T, k, prefix, canonical, min_count):
    """The definition restated window by window for equal-length A/C/G/T reads.
    A forward window w adds 1 to the own Map's key w if w starts with the
    prefix and 1 to its key rc w if that does (canonical mode: 1 to the smaller
    of the two, if it does); windows / hits / sum are the sums over those
    additions of 1, [T(key) >= min_count] and T(key) [T(key) >= min_count]."""
    fw, rc = _window_codes(d, k)
    mc = np.uint64(max(min_count, 1))
    pc = _pack(_LUT[np.frombuffer(prefix, dtype=np.uint8)][None, :])[0] if prefix else np.uint64(0)
    sh = np.uint64(2 * (k - len(prefix)))
    rows = np.zeros((len(d), 4), dtype=np.uint64)
    with np.errstate(over="ignore"):
        if canonical:
            s = np.minimum(fw, rc)
            p, v = (s >> sh) == pc, _get(T, s)
            hit = p & (v >= mc)
            rows[:, 0] = p.sum(axis=1)
            rows[:, 1] = hit.sum(axis=1)
            rows[:, 3] = (v * hit).sum(axis=1, dtype=np.uint64)
        else:
            pf, pr = (fw >> sh) == pc, (rc >> sh) == pc
            vf, vr = _get(T, fw), _get(T, rc)
            hf, hr = pf & (vf >= mc), pr & (vr >= mc)
            rows[:, 0] = pf.sum(axis=1) + pr.sum(axis=1)
            rows[:, 1] = hf.sum(axis=1) + hr.sum(axis=1)
            rows[:, 3] = (vf * hf).sum(axis=1, dtype=np.uint64) + (vr * hr).sum(axis=1, dtype=np.uint64)
    return rows


def _canonical_from_map(m):
    from oracle import oracle
    out = {}
    for key, v in m.items():
        rc = oracle.complement(key)
        if key <= rc:
            out[key] = v // 2 if key == rc else v
    return out


@functools.lru_cache(maxsize=256)
def _own_map(seq, k, prefix, canonical):
    """A read's own Map from the oracle (the count of a file holding that record alone): the values of its
    A/C/G/T keys, their codes, and the read's forward windows that hold another byte."""
    from oracle import oracle
    own = dict(oracle.count_buffer(b"@r\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n", prefix, k, 1))
    if canonical:
        own = _canonical_from_map(own)
    acgt = [(x, v) for x, v in own.items() if not x.translate(None, b"ACGT")]
    skipped = 0
    if len(seq) > 1 and len(seq) >= k:                    # (a line of 0 or 1 bytes is ignored by the count)
        bad = np.concatenate([[0], np.cumsum(_LUT[np.frombuffer(seq, dtype=np.uint8)] > 3)])
        skipped = int(((bad[k:] - bad[:-k]) > 0).sum())
    keys = np.frombuffer(b"".join(x for x, _ in acgt), dtype=np.uint8).reshape(-1, k)
    code = _pack(_LUT[keys]) if acgt else np.zeros(0, np.uint64)
    return [v for _, v in acgt], code, skipped


def _oracle_rows(seqs, T, k, prefix, canonical, min_counts=MIN_COUNTS):
    """{min_count: rows} from the oracle's own Maps and T."""
    out = {mc: np.zeros((len(seqs), 4), dtype=np.uint64) for mc in min_counts}
    for i, seq in enumerate(seqs):
        own_v, code, skipped = _own_map(seq, k, prefix, canonical)
        tv = [int(x) for x in _get(T, code)]
        for mc in min_counts:
            m = max(mc, 1)
            out[mc][i] = (sum(own_v), sum(v for v, t in zip(own_v, tv) if t >= m), skipped,
                          sum(v * t for v, t in zip(own_v, tv) if t >= m) & _M64)
    return out


# ---- the three ways in ----
def _dev(data, offset=0):
    import torch
    t = torch.zeros(len(data) + 8, dtype=torch.uint8, device="cuda")
    t[offset:offset + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def _rows_at(ptr, n):
    import torch
    from kmerjs_amd.multi import device_u64
    if not n:
        return np.zeros((0, 4), dtype=np.uint64)
    dev = torch.device("cuda", torch.cuda.current_device())
    return device_u64(ptr, 4 * n, dev).cpu().numpy().view(np.uint64).reshape(n, 4).copy()


def _screen_device(ctr, buf, nbytes, min_count, flags, offset=0):
    import torch
    ptr, n = ctr.table_screen_device(buf.data_ptr() + offset, nbytes, min_count, flags,
                                     torch.cuda.current_stream().cuda_stream)
    return _rows_at(ptr, n)


def _all_ways(native, ctr, data, min_count, extra=0, buf=None):
    """Device call on the direct and on the sorted route, and the host call: equal rows, returned once."""
    buf = _dev(data) if buf is None else buf
    a = _screen_device(ctr, buf, len(data), min_count, native.SCREEN_DIRECT | extra)
    b = _screen_device(ctr, buf, len(data), min_count, native.SCREEN_SORTED | extra)
    c = ctr.table_screen(data, min_count, extra)
    assert c.dtype == np.uint64 and c.shape == a.shape == b.shape
    assert np.array_equal(a, b), np.argwhere(a != b)[:5]
    assert np.array_equal(a, c), np.argwhere(a != c)[:5]
    assert len(a) == len(data.split(b"\n")[1::4])
    return a


def _same(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (bad[:5].tolist(), got[bad[:5, 0]].tolist(), want[bad[:5, 0]].tolist())


def _counted(native, data, k, prefix, flags, cuts=None):
    """A table-mode context fed `data` from device memory (in chunks at `cuts`) and finished."""
    buf = _dev(data)
    ctr = native.Counter(k=k, prefix=prefix, flags=flags)
    ctr.reset()
    cuts = cuts or [0, len(data)]
    for lo, hi in zip(cuts, cuts[1:]):
        ctr.feed_device(buf.data_ptr() + lo, hi - lo)
    ctr.finish(want_result=False)
    return ctr


def _mode(native, canonical):
    return native.FLAG_CANONICAL if canonical else native.FLAG_UNORDERED


# unordered: (31, ""), (32, "GT"), (22, ""), (21, "A"), (21, ""), (20, ""), (16, "ATGAC"), (15, "T"), (1, "");
# canonical: (21, ""), (21, "A"), (16, ""), (31, "")
MODES = [(31, b"", False), (31, b"", True), (32, b"GT", False), (22, b"", False), (21, b"A", False), (21, b"A", True),
         (21, b"", False), (21, b"", True), (20, b"", False), (16, b"ATGAC", False), (16, b"", True), (15, b"T", False),
         (1, b"", False)]


@pytest.mark.parametrize("k,prefix,canonical", MODES)
def test_screen_parity_matrix(native, table_input, screened_input, k, prefix, canonical):
    T = _table_map(table_input, prefix, k, canonical)
    ctr = _counted(native, table_input, k, prefix, _mode(native, canonical))
    d = _synth_digits(screened_input)
    buf = _dev(screened_input)
    sample = list(range(0, 2000, 83))                     # 25 reads, both halves: the model against the oracle
    seqs = screened_input.split(b"\n")[1::4]
    orc = _oracle_rows([seqs[i] for i in sample], T, k, prefix, canonical)
    seen_hit = seen_miss = False
    for mc in MIN_COUNTS:
        want = _model_rows(d, T, k, prefix, canonical, mc)
        _same(want[sample], orc[mc])
        got = _all_ways(native, ctr, screened_input, mc, buf=buf)
        _same(got, want)
        if mc == 1:
            assert (got[:, 1] <= got[:, 0]).all() and (got[:, 2] == 0).all()
            _same(_screen_device(ctr, buf, len(screened_input), 1, 0), want)       # (auto)
            seen_hit = bool((got[:1000, 1] == got[:1000, 0]).all() and got[:1000, 0].sum() > 0)
            seen_miss = bool((got[1000:, 1] < got[1000:, 0]).any())
        if mc == 1 << 40:
            assert (got[:, 1] == 0).all() and (got[:, 3] == 0).all()
    assert seen_hit and (seen_miss or k == 1)                         # reads of the table's range hit everywhere, the others do not
    # the table's own input: every counted window hits, and sum adds up to the sum of T(x)^2
    own = _screen_device(ctr, _dev(table_input), len(table_input), 1, 0)
    assert len(own) == 3000 and np.array_equal(own[:, 1], own[:, 0])
    with np.errstate(over="ignore"):
        assert own[:, 3].sum(dtype=np.uint64) == (T[1] * T[1]).sum(dtype=np.uint64)
    assert int(own[:, 0].sum()) == int(T[1].sum())
    ctr.close()


def _shapes_file(k, table_input, rng):
    """One small hand-made file: the line shapes of the issue (see the test below)."""
    td = _synth_digits(table_input)

    def rnd(n):
        return _key_bytes(rng.integers(0, 4, (1, n), dtype=np.uint8))

    def known(n):                                         # bases of the table's reads, back to back: windows that hit
        rows = td[rng.integers(0, len(td), n // 150 + 1)]
        return _key_bytes(rows)[:n]

    seqs = [b"", b"A", known(k - 1) if k > 1 else b"", known(k), known(k + 63), known(k + 64), known(k + 65),
            rnd(k + 64), known(150), known(75) + rnd(75)]
    long5, long70 = bytearray(known(3000) + rnd(2000)), bytearray(rnd(10_000) + known(60_000))
    long70[40_000] = ord("N")
    long70[69_999] = ord("c")
    seqs += [bytes(long5), bytes(long70)]
    x = bytearray(known(150))
    x[40], x[41], x[100] = ord("N"), ord("n"), ord("a")
    seqs += [bytes(x), b"N" * 150, known(150).lower(), known(100) + b"\r", known(k) + b"\r", b"\r"]
    recs = [b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs)]
    recs[3] = recs[3].replace(b"\n", b"\r\n")             # a whole CRLF record
    return b"".join(recs)


@pytest.mark.parametrize("k,prefix,canonical", [(31, b"", False), (21, b"A", True), (16, b"ATGAC", False), (1, b"", False)])
def test_screen_line_shapes(native, table_input, k, prefix, canonical):
    """Sequence lines of 0, 1, k - 1, k, k + 63, k + 64 and k + 65 bytes (the
    wave edges), one of 5,000 and one of 70,000 bases, CRLF lines, N and
    lowercase bytes; the file ending in a sequence line without '\\n', in a
    header with no sequence line (with and without its '\\n'), and plainly;
    everything again with 4,096-window pieces (KMER_SCREEN_PIECE_TEST)."""
    rng = np.random.default_rng(k)
    T = _table_map(table_input, prefix, k, canonical)
    ctr = _counted(native, table_input, k, prefix, _mode(native, canonical))
    base = _shapes_file(k, table_input, rng)
    tail = _key_bytes(_synth_digits(table_input)[7:8])
    files = [base, base + b"@last\n" + tail, base + b"@trail\n", base + b"@trail", base + b"@last\n" + tail + b"\r"]
    for fi, data in enumerate(files):
        seqs = data.split(b"\n")[1::4]
        mcs = MIN_COUNTS if fi == 0 else (1, 2)
        orc = _oracle_rows(seqs, T, k, prefix, canonical, mcs)
        for mc in mcs:
            want = orc[mc]
            if fi == 0 and mc == 1:
                assert want[0].sum() == 0 and want[1].sum() == 0 and want[11, 0] > 0 and want[11, 2] > 0
                assert (want[:, 1] > 0).any() and ((want[:, 1] < want[:, 0]).any() or k == 1)   # (k 1: all four hit)
            _same(_all_ways(native, ctr, data, mc), want)
            _same(_all_ways(native, ctr, data, mc, extra=native.SCREEN_PIECE_TEST), want)
    ctr.close()


def test_screen_unaligned_input(native, table_input):
    # the same bytes at offsets 0 .. 3 of a device tensor, ending without '\n': equal rows
    k = 31
    T = _table_map(table_input, b"", k, False)
    ctr = _counted(native, table_input, k, b"", native.FLAG_UNORDERED)
    data = (_synth(3, 500, 300) + _shapes_file(k, table_input, np.random.default_rng(2)))[:-1]
    want = _all_ways(native, ctr, data, 1)
    seqs = data.split(b"\n")[1::4]
    pick = list(range(0, len(seqs), 7)) + [len(seqs) - 1]
    _same(want[pick], _oracle_rows([seqs[i] for i in pick], T, k, b"", False, (1,))[1])
    for off in (1, 2, 3):
        buf = _dev(data, off)
        for flags in (native.SCREEN_DIRECT, native.SCREEN_SORTED, native.SCREEN_SORTED | native.SCREEN_PIECE_TEST):
            _same(_screen_device(ctr, buf, len(data), 1, flags, offset=off), want)
    ctr.close()


@pytest.mark.parametrize("k", [16, 15])
@pytest.mark.parametrize("prefix", [b"", b"A", b"T"])
def test_screen_palindromes_and_big_counts(native, k, prefix):
    # one class seen > 2^20 times (its count is in the big list), and AT-repeat
    # palindromes at even k: weight 2 and a doubled value in table mode
    polya = b"".join(b"@r%010d\n%s\n+\n%s\n" % (i, b"A" * 150, b"I" * 150) for i in range(9000))
    at = b"".join(b"@s%010d\n%s\n+\n%s\n" % (i, b"AT" * 75, b"I" * 150) for i in range(300))
    data = polya + at
    rng = np.random.default_rng(k)
    seqs = [b"A" * 150, b"T" * 150, b"AT" * 75, b"TA" * 75, b"A" * 75 + b"AT" * 37 + b"C"]
    seqs += [_key_bytes(rng.integers(0, 4, (1, 150), dtype=np.uint8)) for _ in range(40)]
    screened = b"".join(b"@q%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))
    for canonical in (False, True):
        T = _table_map(data, prefix, k, canonical)
        orc = _oracle_rows(seqs, T, k, prefix, canonical)
        ctr = native.Counter(k=k, prefix=prefix, flags=_mode(native, canonical))
        ctr.count_buffer(data)
        for mc in MIN_COUNTS:
            got = _all_ways(native, ctr, screened, mc)
            _same(got, orc[mc])
        got = _all_ways(native, ctr, screened, 1)
        W = 150 - k + 1
        both = 2 if prefix == b"" and not canonical else 1               # (no prefix: both orientations are keys)
        assert 9000 * 136 > (1 << 20) - 1                 # poly-A: every window carries the count above 2^20
        if k == 15 and (prefix in (b"", b"A") or not canonical):         # (rc of a poly-A window starts with T)
            assert got[0, 0] == got[0, 1] == both * W and got[0, 3] == both * W * 9000 * 136
        if k == 15 and prefix == b"T" and canonical:
            assert got[0].sum() == 0
        if k == 16 and prefix == b"" and not canonical:   # AT repeats: windows at even offsets are palindromes
            assert got[2, 0] == 2 * W and got[2, 1] == 2 * W
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
def test_screen_one_long_bucket(native, split):
    """A table of 5,000 31-mers that all fall into ONE bucket (the documented
    hash inverted on the CPU, as test_lookup_scans_a_long_bucket does),
    screened with 10,000 reads of exactly 31 bases -- 5,000 present in
    scrambled order, 5,000 absent -- plus 200 random 150-base reads: the
    wave-cooperative scan and, on the sorted route, one long run.  split: the
    table comes from the other final kernel (FLAG_TABLE_SPLIT_TEST)."""
    import torch
    from kmerjs_amd.multi import _CudaArray
    k, q = 31, 0x5A5A5
    rng = np.random.default_rng(31)
    rem = np.unique(rng.integers(0, 1 << 44, 120_000, dtype=np.uint64))
    rem = rem[rng.permutation(len(rem))]
    h = (np.uint64(q) << np.uint64(44)) | rem
    with np.errstate(over="ignore"):
        c = h * np.uint64(_INV)                           # (mod 2^64)
    c = c[c < np.uint64(1 << 62)]                         # a 31-mer's planar code ...
    d = _planar_digits(c, k)
    d = d[c <= _planar(_rc(d))]                           # ... and the class's canonical one
    assert len(d) >= 10_000
    written, absent = d[:5000], d[5000:10_000]
    recs = []
    for i, row in enumerate(written):
        rec = b"@r%d\n%s\n+\n%s\n" % (i, _key_bytes(row[None, :]), b"I" * k)
        recs.append(rec * (3 if i % 97 == 0 else 1))
    data = b"".join(recs)
    T = _table_map(data, b"", k, False)
    assert len(T[0]) == 2 * len(written)
    ctr = native.Counter(k=k, prefix=b"", flags=native.FLAG_UNORDERED | (native.FLAG_TABLE_SPLIT_TEST if split else 0))
    ctr.count_buffer(data)
    _, _, ln, _, _ = ctr.table_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    lens = torch.as_tensor(_CudaArray(ln, 1 << 20, "<i4"), device=dev)
    assert int(lens[q]) == len(written) and int(lens.sum()) == len(written)   # the test's point: one long bucket
    short = np.concatenate([written, absent])
    flip = rng.random(len(short)) < 0.5                   # either orientation of a class
    short = np.where(flip[:, None], _rc(short), short)
    order = rng.permutation(len(short))
    short = short[order]
    rand = rng.integers(0, 4, (200, 150), dtype=np.uint8)
    screened = b"".join(b"@s%d\n%s\n+\n%s\n" % (i, _key_bytes(r[None, :]), b"I" * k) for i, r in enumerate(short))
    screened += b"".join(b"@t%d\n%s\n+\n%s\n" % (i, _key_bytes(r[None, :]), b"I" * 150) for i, r in enumerate(rand))
    for mc in (1, 3):
        want = np.concatenate([_model_rows(short, T, k, b"", False, mc), _model_rows(rand, T, k, b"", False, mc)])
        if mc == 1:
            assert (want[:10_000, 0] == 2).all() and (want[:10_000, 1] == 2).sum() == 5000
            assert (want[:10_000, 3] == 6).sum() == len(range(0, 5000, 97))
            assert np.array_equal(want[:10_000, 1] == 2, order < 5000)
        _same(_all_ways(native, ctr, screened, mc), want)
    sample = list(range(0, 10_200, 401))
    seqs = screened.split(b"\n")[1::4]
    _same(want[sample], _oracle_rows([seqs[i] for i in sample], T, k, b"", False, (3,))[3])
    ctr.close()


@pytest.mark.parametrize("route", ["chunks", "fixed"])
def test_screen_feeding_routes(native, table_input, screened_input, route):
    # a table fed in chunks, and one whose pass 1 wrote fixed runs with filler slots (FLAG_TABLE_FIXED_TEST)
    k = 31
    T = _table_map(table_input, b"", k, False)
    if route == "chunks":
        ctr = _counted(native, table_input, k, b"", native.FLAG_UNORDERED, [0, 317 * 700, 317 * 1900, 317 * 3000])
    else:
        ctr = _counted(native, table_input, k, b"", native.FLAG_UNORDERED | native.FLAG_TABLE_FIXED_TEST)
    want = _model_rows(_synth_digits(screened_input), T, k, b"", False, 2)
    _same(_all_ways(native, ctr, screened_input, 2), want)
    ctr.close()


@pytest.mark.parametrize("k,flags_name", [(31, "FLAG_UNORDERED"), (21, "FLAG_CANONICAL")])
def test_screen_on_exchanged_tables(native, table_input, screened_input, k, flags_name):
    """World 2 in one process (the pattern of test_lookup_on_exchanged_tables):
    each rank's table holds its buckets only, so hits and sum add up to the
    single table's, and windows and skipped are equal on both ranks."""
    import torch
    from kmerjs_amd.multi import device_u64
    world, n_reads = 2, 3000
    flags = getattr(native, flags_name)
    canonical = flags_name == "FLAG_CANONICAL"
    T = _table_map(table_input, b"", k, canonical)
    want = _model_rows(_synth_digits(screened_input), T, k, b"", canonical, 1)
    buf = _dev(table_input)
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
        got.append(_all_ways(native, c, screened_input, 1))
    for g in got:
        assert np.array_equal(g[:, 0], want[:, 0]) and np.array_equal(g[:, 2], want[:, 2])
    with np.errstate(over="ignore"):
        assert np.array_equal(got[0][:, 1] + got[1][:, 1], want[:, 1])
        assert np.array_equal(got[0][:, 3] + got[1][:, 3], want[:, 3])
    assert got[0][:, 1].sum() > 0 and got[1][:, 1].sum() > 0
    for c in ctrs:
        c.close()
    del recvs


def _status(native, f):
    with pytest.raises(native.KmerError) as e:
        f()
    return e.value.status


def test_screen_states_and_reuse(native, table_input, screened_input):
    import torch
    k = 31
    data = screened_input[:317 * 400]
    buf = _dev(data)
    d = _synth_digits(data)
    stream = torch.cuda.current_stream().cuda_stream
    ctr = native.Counter(k=k, prefix=b"", flags=native.FLAG_UNORDERED)
    assert _status(native, lambda: ctr.table_screen(data)) == E_STATE             # no finish yet
    assert _status(native, lambda: ctr.table_screen_device(buf.data_ptr(), len(data))) == E_STATE
    # an empty table: no hits, windows as for any table
    tiny = _dev(b"@r\nAC\n+\nII\n")
    ctr.reset()
    ctr.feed_device(tiny.data_ptr(), 11)
    ctr.finish(want_result=False)
    assert ctr.table_stats()[0] == 0
    empty_T = (np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64))
    want0 = _model_rows(d, empty_T, k, b"", False, 1)
    assert (want0[:, 0] == 240).all() and (want0[:, 1] == 0).all()
    _same(_all_ways(native, ctr, data, 1, buf=buf), want0)
    # the context counts again after a reset
    tbuf = _dev(table_input)
    ctr.reset()
    assert _status(native, lambda: ctr.table_screen(data)) == E_STATE
    ctr.feed_device(tbuf.data_ptr(), len(table_input))
    assert _status(native, lambda: ctr.table_screen_device(buf.data_ptr(), len(data))) == E_STATE   # fed, not finished
    ctr.finish(want_result=False)
    T = _table_map(table_input, b"", k, False)
    want = _model_rows(d, T, k, b"", False, 1)
    keys = _key_bytes(_synth_digits(table_input)[::50, 20:20 + k])
    before = (ctr.table_digest(), ctr.table_stats(), ctr.lines(), ctr.table_lookup(keys).tolist())
    for _ in range(2):                                    # repeated calls
        _same(_all_ways(native, ctr, data, 1, buf=buf), want)
    # len == 0: no reads, nothing touched
    assert ctr.table_screen(b"").shape == (0, 4)
    assert ctr.table_screen_device(0, 0) == (0, 0)
    # a rows pointer fetched before an extract is still correct after it
    ptr, n = ctr.table_screen_device(buf.data_ptr(), len(data), 1, 0, stream)
    dk, dc, nk = ctr.table_extract_device(1, 0)
    assert nk > 0 and dk and dc
    _same(_rows_at(ptr, n), want)
    # non-ASCII input is refused as for a feed; the table stays readable
    bad = bytearray(data)
    bad[5000] = 0x80
    assert _status(native, lambda: ctr.table_screen(bytes(bad))) == E_NONASCII
    _same(ctr.table_screen(data), want)
    after = (ctr.table_digest(), ctr.table_stats(), ctr.lines(), ctr.table_lookup(keys).tolist())
    assert after == before and before[2] == 12_000
    ctr.close()
    # contexts that cannot screen
    ordered = native.Counter(k=16, prefix=b"ATGAC")       # an ordered-mode context has no table
    ordered.count_buffer(data)
    assert _status(native, lambda: ordered.table_screen(data)) == E_STATE
    assert _status(native, lambda: ordered.table_screen_device(buf.data_ptr(), len(data))) == E_STATE
    ordered.close()
    fasta = native.Counter(k=k, prefix=b"", flags=native.FLAG_UNORDERED | native.FLAG_FASTA)
    fasta.count_buffer(b">a\n" + _key_bytes(d[:1]) + b"\n")
    assert _status(native, lambda: fasta.table_screen(data)) == E_STATE
    assert _status(native, lambda: fasta.table_screen_device(buf.data_ptr(), len(data))) == E_STATE
    fasta.close()
    grp = native.Counter(k=k, prefix=b"", flags=native.FLAG_UNORDERED, devices=[0, 0])
    r = ctypes.c_void_p()
    assert native.LIB.kmer_count_buffer(grp.h, data, len(data), ctypes.byref(r)) == 0
    native.LIB.kmer_result_free(r)
    assert _status(native, lambda: grp.table_screen(data)) == E_STATE
    assert _status(native, lambda: grp.table_screen_device(buf.data_ptr(), len(data))) == E_STATE
    grp.close()


def test_screen_host_call_in_small_pieces(native, table_input, screened_input):
    # a small batch_bytes: the host call uploads the input in several pieces cut at record boundaries
    k = 31
    T = _table_map(table_input, b"", k, False)
    ctr = native.Counter(k=k, prefix=b"", flags=native.FLAG_UNORDERED, batch_bytes=100_000)
    r = ctypes.c_void_p()                                 # (the host result is freed, not copied to Python)
    assert native.LIB.kmer_count_buffer(ctr.h, table_input, len(table_input), ctypes.byref(r)) == 0
    native.LIB.kmer_result_free(r)
    data = screened_input + b"@last\n" + _key_bytes(_synth_digits(table_input)[3:4])      # (no '\n' at the end)
    d = np.concatenate([_synth_digits(screened_input), _synth_digits(table_input)[3:4]])
    assert len(data) > 6 * 100_000
    want = _model_rows(d, T, k, b"", False, 1)
    host = ctr.table_screen(data, 1)
    _same(host, want)
    _same(_screen_device(ctr, _dev(data), len(data), 1, 0), host)
    _same(ctr.table_screen(data, 1, native.SCREEN_SORTED | native.SCREEN_PIECE_TEST), want)
    # cap too small: KMER_E_BAD_PARAM with the true number of reads
    rows = (native.ReadScreen * 10)()
    n = ctypes.c_uint64()
    st = native.LIB.kmer_table_screen(ctr.h, data, len(data), 1, 0, rows, 10, ctypes.byref(n))
    assert st == E_BAD_PARAM and n.value == 2001
    assert all(r.windows == 0 for r in rows)
    ctr.close()
