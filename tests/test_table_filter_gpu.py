"""GPU parity of the read filter (kmer_table_filter / kmer_table_filter_device,
kmer_filter.hip): the records of the screened reads that pass the predicate,
compacted on the device.  Every case goes through the device call with the
direct and with the sorted route and through the host call; the three must
agree byte for byte on out, keep, the four result fields and the rows.
Expected values come from the model in tests/filter_util.py (records from
data.split, the predicate in Python integers), applied to rows from the screen
tests' models and oracle calls -- never from the library's own filter."""
import ctypes

import numpy as np
import pytest

from tests.filter_util import EDGE_INPUTS, FILTER_DROP, FILTER_PAIRED, filter_model
from tests.test_table_screen_gpu import (_key_bytes, _mode, _model_rows, _oracle_rows, _rows_at, _same, _status,
                                         _synth, _synth_digits, _table_map)

pytestmark = pytest.mark.gpu

E_NONASCII, E_STATE = 6, 8
CONFIGS = [(31, b"", False), (16, b"ATGAC", False), (21, b"A", True)]


@pytest.fixture(scope="module")
def native():
    from kmerjs_amd import _native
    assert (_native.FILTER_DROP, _native.FILTER_PAIRED) == (FILTER_DROP, FILTER_PAIRED)
    return _native


@pytest.fixture(scope="module")
def table_input():
    """3,000 synthetic reads: the table's input."""
    return _synth(3, 0, 3000)


@pytest.fixture(scope="module")
def two_sources():
    """2,000 records of 317 bytes: 1,000 from the table's range, 1,000 from another seed."""
    return _synth(3, 1000, 1000) + _synth(9, 0, 1000)


@pytest.fixture(scope="module")
def tables(native, table_input):
    """(k, prefix, canonical[, batch_bytes]) -> (a finished table-mode context of table_input, its expected Map)."""
    made = {}

    def get(k, prefix, canonical, batch_bytes=0):
        key = (k, prefix, canonical, batch_bytes)
        if key not in made:
            kw = {"batch_bytes": batch_bytes} if batch_bytes else {}
            ctr = native.Counter(k=k, prefix=prefix, flags=_mode(native, canonical), **kw)
            buf = _dev(table_input)
            ctr.reset()
            ctr.feed_device(buf.data_ptr(), len(table_input))
            ctr.finish(want_result=False)
            made[key] = (ctr, _table_map(table_input, prefix, k, canonical))
        return made[key]

    yield get
    for ctr, _ in made.values():
        ctr.close()


# ---- the three ways in ----
def _dev(data, offset=0):
    import torch
    t = torch.zeros(len(data) + 32, dtype=torch.uint8, device="cuda")
    if data:
        t[offset:offset + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def _bytes_at(ptr, n):
    import torch
    from kmerjs_amd.multi import _CudaArray
    if not n:
        return b""
    assert ptr
    dev = torch.device("cuda", torch.cuda.current_device())
    return torch.as_tensor(_CudaArray(ptr, n, "|u1"), device=dev).cpu().numpy().tobytes()


def _filter_device(ctr, buf, nbytes, offset=0, **kw):
    import torch
    d_out, d_keep, d_rows, res = ctr.table_filter_device(buf.data_ptr() + offset, nbytes,
                                                         stream=torch.cuda.current_stream().cuda_stream, **kw)
    keep = np.frombuffer(_bytes_at(d_keep, res.n_reads), dtype=np.uint8)
    assert ((keep == 0) | (keep == 1)).all()
    return _bytes_at(d_out, res.out_len), keep.astype(bool), _rows_at(d_rows, res.n_reads), res


def _fields(res):
    return {"n_reads": res.n_reads, "n_kept": res.n_kept, "out_len": res.out_len, "consumed": res.consumed}


def _first_diff(a, b):
    n = min(len(a), len(b))
    x = np.flatnonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))
    return (len(a), len(b), int(x[0]) if len(x) else n)


def _check(native, ctr, data, want_rows, min_hits=1, frac=(0, 1), flags=0, extra=0, min_count=1, buf=None, offset=0):
    """The model on want_rows (None: on the rows of table_screen) against the three ways; -> the model's result."""
    screen = ctr.table_screen(data, min_count, extra)
    if want_rows is not None:
        _same(screen, np.asarray(want_rows, dtype=np.uint64).reshape(-1, 4))
    out, keep, res = filter_model(data, screen if want_rows is None else want_rows, min_hits, frac, flags)
    assert data[res["consumed"]:].count(b"\n") == 0 or res["n_reads"] == 0
    buf = _dev(data, offset) if buf is None else buf
    kw = dict(min_count=min_count, min_hits=min_hits, frac=frac, flags=flags)
    ways = [_filter_device(ctr, buf, len(data), offset, screen_flags=native.SCREEN_DIRECT | extra, **kw),
            _filter_device(ctr, buf, len(data), offset, screen_flags=native.SCREEN_SORTED | extra, **kw)]
    h_out, h_keep, h_res = ctr.table_filter(data, screen_flags=extra, **kw)
    assert h_keep.dtype == bool
    ways.append((h_out, h_keep, screen, h_res))
    for wi, (g_out, g_keep, g_rows, g_res) in enumerate(ways):
        assert _fields(g_res) == res, (wi, _fields(g_res), res)
        assert g_keep.tolist() == keep, (wi, np.flatnonzero(g_keep != np.array(keep, dtype=bool))[:5])
        assert g_out == out, (wi, _first_diff(g_out, out))
        _same(g_rows, screen)
    return out, keep, res


# ---- 1. bulk ----
def _patterns():
    """Record indices into two_sources (0..999: the table's range, 1000..1999: the other seed), and whether both mix."""
    m, n = np.arange(1000), np.arange(1000, 2000)
    runs, mi, ni = [], 0, 0
    for _ in range(4):
        for run in (1, 2, 3, 63, 64, 65):
            runs += list(m[mi:mi + run]) + [n[ni]]
            mi, ni = mi + run, ni + 1
    return {"halves": (np.concatenate([m, n]), True),
            "alternating": (np.stack([m, n], axis=1).reshape(-1), True),
            "runs": (np.array(runs), True),
            "all": (m, False),
            "none": (n, False)}


@pytest.mark.parametrize("k,prefix,canonical", CONFIGS)
def test_filter_bulk(native, tables, two_sources, k, prefix, canonical):
    ctr, T = tables(k, prefix, canonical)
    rows_all = _model_rows(_synth_digits(two_sources), T, k, prefix, canonical, 1)
    recs = np.frombuffer(two_sources, dtype=np.uint8).reshape(2000, 317)
    for name, (idx, mixed) in _patterns().items():
        data = recs[idx].tobytes()
        rows = rows_all[idx]
        buf = _dev(data)
        for flags in (0, FILTER_DROP):
            for frac in ((0, 1), (1, 2)):
                out, keep, res = _check(native, ctr, data, rows, 1, frac, flags, buf=buf)
                assert res["n_reads"] == len(idx) and res["consumed"] == len(data)
                if mixed:
                    assert 0 < res["n_kept"] < res["n_reads"], (name, flags, frac, res)
                if name == "runs" and k == 31 and not flags:
                    assert np.array_equal(np.array(keep), idx < 1000)     # the runs of 1, 2, 3, 63, 64, 65 as laid out


# ---- 2. identity and emptiness ----
def _identity(native, ctr, data, n_reads=None, consumed=None, **kw):
    out, keep, res = _check(native, ctr, data, None, 0, (0, 1), 0, **kw)
    assert out == data[:res["consumed"]] and all(keep) and res["n_kept"] == res["n_reads"]
    if n_reads is not None:
        assert (res["n_reads"], res["consumed"]) == (n_reads, consumed)
    tail = len(data) - res["consumed"]
    out, keep, res2 = _check(native, ctr, data, None, 0, (0, 1), FILTER_DROP, **kw)
    assert out == b"" and not any(keep) and res2["n_kept"] == 0 and res2["consumed"] == res["consumed"]
    return res, tail


def _small_records(rng, n):
    """Records of 4 to 40 bytes: four lines of 0 to 9 bytes each."""
    out = []
    for i in range(n):
        lens = [0] * 4 if i == 1 else [9] * 4 if i == 2 else rng.integers(0, 10, 4)
        lines = [bytes(rng.choice(np.frombuffer(b"ACGTN@+I", np.uint8), int(x))) for x in lens]
        out.append(b"".join(x + b"\n" for x in lines))
    assert min(map(len, out)) == 4 and max(map(len, out)) == 40
    return b"".join(out)


def test_filter_identity_on_edge_inputs(native, tables):
    ctr, _ = tables(31, b"", False)
    for name, (data, n, consumed) in EDGE_INPUTS.items():
        res, tail = _identity(native, ctr, data, n, consumed)
        assert tail == len(data) - consumed, name
    assert _identity(native, ctr, EDGE_INPUTS["partial_header"][0])[1] == 7
    assert _identity(native, ctr, EDGE_INPUTS["no_newline"][0])[1] == 8


def test_filter_identity_on_short_and_long_records(native, tables, table_input):
    ctr, _ = tables(31, b"", False)
    rng = np.random.default_rng(4)
    res, tail = _identity(native, ctr, b"\n\n\n\n" * 2000, 2000, 8000)
    assert tail == 0
    small = _small_records(rng, 1500)
    _identity(native, ctr, small, 1500, len(small))
    _identity(native, ctr, small + b"@partial", 1500, len(small))
    _identity(native, ctr, small[:-1], 1500, len(small) - 1)
    # one record whose sequence line is 200,000 bases, between 300-byte records
    r300 = [b"@r%03d\n%s\n+\n%s\n" % (i, _key_bytes(rng.integers(0, 4, (1, 145), dtype=np.uint8)), b"I" * 145)
            for i in range(6)]
    assert all(len(x) == 300 for x in r300)
    seq = _key_bytes(_synth_digits(table_input))[:200_000]     # the table's reads back to back: it matches
    big = b"@long\n" + seq + b"\n+\n" + b"I" * 200_000 + b"\n"
    data = b"".join(r300[:3]) + big + b"".join(r300[3:])
    _identity(native, ctr, data, 7, len(data))
    # the long one alone kept, and alone dropped
    out, keep, res = _check(native, ctr, data, None, 1, (1, 2), 0)
    assert keep == [False] * 3 + [True] + [False] * 3 and out == big
    out, keep, res = _check(native, ctr, data, None, 1, (1, 2), FILTER_DROP)
    assert out == b"".join(r300)


def test_filter_input_at_every_byte_offset(native, tables, table_input):
    ctr, T = tables(31, b"", False)
    data, rows = _uneven(table_input, T, 31, 40)
    want = None
    for off in range(16):
        buf = _dev(data, off)
        got = _check(native, ctr, data, rows, 1, (1, 2), 0, buf=buf, offset=off)
        assert want is None or got == want
        want = got
        _identity(native, ctr, data, buf=buf, offset=off)
    assert 0 < want[2]["n_kept"] < want[2]["n_reads"]


# ---- 3. selective keep on uneven records ----
def _uneven(table_input, T, k, n=130, seed=5):
    """n records of 20 bytes to 5 KB; a fixed pseudo-random pattern decides which hold substrings of the table's
    source (they match) and which an unrelated random sequence; -> (data without a final '\\n', oracle rows)."""
    rng = np.random.default_rng(seed)
    td = _synth_digits(table_input)
    seqs = []
    for i in range(n):
        L = int(rng.choice([7, 30, 31, 60, 150, 400, 1200, 2490]))
        if i == 0:
            L = 7
        if i == 1:
            L = 2490                                       # about 5 KB
        if rng.random() < 0.5:
            row = td[int(rng.integers(0, len(td)))]
            reps = -(-L // 150)
            seqs.append((_key_bytes(row[None, :]) * reps)[:L] if L <= 150 else
                        b"".join(_key_bytes(td[int(j)][None, :]) for j in rng.integers(0, len(td), reps))[:L])
        else:
            seqs.append(_key_bytes(rng.integers(0, 4, (1, L), dtype=np.uint8)))
    recs = [b"@%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs)]
    recs[0] = recs[0][:1] + recs[0][2:]                   # "@\n" + 7 + "\n+\n" + 7 + "\n": 20 bytes
    assert min(map(len, recs)) == 20 and max(map(len, recs)) > 4900
    data = b"".join(recs)[:-1]
    return data, _oracle_rows(seqs, T, k, b"", False, (1,))[1]


def test_filter_selective_on_uneven_records(native, tables, table_input):
    k = 31
    ctr, T = tables(k, b"", False, batch_bytes=20_000)
    data, rows = _uneven(table_input, T, k)
    assert len(data) > 4 * 20_000                         # the host call cuts the input several times
    for extra in (0, native.SCREEN_PIECE_TEST):
        for flags in (0, FILTER_DROP):
            for min_hits, frac in ((1, (0, 1)), (1, (1, 2)), (200, (0, 1)), (1, (1, 1))):
                out, keep, res = _check(native, ctr, data, rows, min_hits, frac, flags, extra=extra)
                assert 0 < res["n_kept"] < res["n_reads"] == 130 and res["consumed"] == len(data)


# ---- 4. paired ----
@pytest.mark.parametrize("last", ["match", "miss"])
def test_filter_paired(native, tables, two_sources, last):
    k = 31
    ctr, T = tables(k, b"", False, batch_bytes=3 * 317)   # per-record cuts would take 3 records: inside a pair
    rows_all = _model_rows(_synth_digits(two_sources), T, k, b"", False, 1)
    recs = np.frombuffer(two_sources, dtype=np.uint8).reshape(2000, 317)
    M, N = 0, 1000
    idx = np.array([M, N + 1, N + 2, M + 3, N + 4, N + 5, M + 6, M + 7, N + 8, N + 9, N + 10, M + 11,
                    M + 12 if last == "match" else N + 12])
    data, rows = recs[idx].tobytes(), rows_all[idx]
    assert (rows[idx < 1000, 1] > 0).all() and (rows[idx >= 1000, 1] == 0).all()
    pairs = [True, True, True, True, False, False, True, True, False, False, True, True, last == "match"]
    out, keep, res = _check(native, ctr, data, rows, 1, (0, 1), FILTER_PAIRED)
    assert keep == pairs
    out, keep, res = _check(native, ctr, data, rows, 1, (1, 2), FILTER_PAIRED | FILTER_DROP)
    assert keep == [not x for x in pairs]
    out, keep, res = _check(native, ctr, data, rows, 1, (0, 1), 0)           # unpaired: each record on its own
    assert keep == (idx < 1000).tolist()
    _check(native, ctr, data[:-1], rows, 1, (0, 1), FILTER_PAIRED)


# ---- 5. bytes outside A/C/G/T ----
def test_filter_reads_with_n(native, tables, table_input):
    k = 31
    ctr, T = tables(k, b"", False)
    td = _synth_digits(table_input)
    a, b, c = (bytearray(_key_bytes(td[i:i + 1])) for i in (5, 6, 7))
    a[40:70] = b"N" * 30
    b[0:10] = b"N" * 10
    b[140:150] = b"n" * 10
    seqs = [bytes(a), b"N" * 150, bytes(b), bytes(c), b"N" * 31, b"N" * 30]
    data = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))
    rows = _oracle_rows(seqs, T, k, b"", False, (1,))[1]
    assert rows[1, 0] == 0 and rows[1, 2] > 0 and rows[0, 2] > 0 and rows[0, 1] > 0 and rows[3, 2] == 0
    out, keep, res = _check(native, ctr, data, rows, 1, (0, 1), 0)
    assert keep == [True, False, True, True, False, False]
    _check(native, ctr, data, rows, 1, (1, 1), FILTER_DROP)
    out, keep, res = _check(native, ctr, data, rows, 0, (0, 1), 0)
    assert all(keep)


# ---- 6. lifetime and state ----
def test_filter_leaves_the_table_and_feeds_a_second_context(native, tables, two_sources):
    import torch
    from oracle import oracle
    k = 31
    ctr, T = tables(k, b"", False)
    stream = torch.cuda.current_stream().cuda_stream
    data = np.frombuffer(two_sources, dtype=np.uint8).reshape(2000, 317)[np.arange(2000).reshape(2, 1000).T.ravel()]
    data = data[:600].tobytes()
    buf = _dev(data)
    rows = ctr.table_screen(data, 1)
    dk, dc, nk = ctr.table_extract_device(1, 0)
    assert nk > 0
    keys0, cnt0 = _bytes_at(dk, nk * k), _bytes_at(dc, nk * 8)
    before = (ctr.table_digest(), ctr.table_stats(), ctr.lines())
    d_out, d_keep, d_rows, res = ctr.table_filter_device(buf.data_ptr(), len(data), stream=stream)
    out, keep, want = filter_model(data, rows, 1, (0, 1), 0)
    assert _fields(res) == want and 0 < res.n_kept < res.n_reads and d_out % 16 == 0
    assert (ctr.table_digest(), ctr.table_stats(), ctr.lines()) == before and before[2] == 12_000
    assert _bytes_at(dk, nk * k) == keys0 and _bytes_at(dc, nk * 8) == cnt0
    # the output stays on the device: fed to a second context on the same stream
    second = native.Counter(k=16, prefix=b"ATGAC")
    second.reset()
    second.feed_device(d_out, res.out_len, stream)
    got = second.finish().entries()
    assert got == list(oracle.count_buffer(out, b"ATGAC", 16, 1)) and len(got) > 0
    second.close()
    # out-pointers may be NULL: counts only
    p = native.FilterParams(1, 1, 0, 1, 0, 0)
    r2 = native.FilterResult()
    assert native.LIB.kmer_table_filter_device(ctr.h, buf.data_ptr(), len(data), p, stream, None, None, None, r2) == 0
    assert _fields(r2) == want
    r3 = native.FilterResult()
    assert native.LIB.kmer_table_filter(ctr.h, data, len(data), p, None, 0, None, 0, r3) == 0
    assert _fields(r3) == want
    # a buffer that turns out too small: KMER_E_BAD_PARAM naming both sizes
    small = (ctypes.c_uint8 * 1000)()
    assert native.LIB.kmer_table_filter(ctr.h, data, len(data), p, small, 1000, None, 0, r3) == 2
    msg = native.LIB.kmer_last_error(ctr.h).decode()
    assert "1000" in msg and any(str(v) in msg for v in (want["out_len"],)), msg
    assert native.LIB.kmer_table_filter(ctr.h, data, len(data), p, None, 0, small, 10, r3) == 2
    msg = native.LIB.kmer_last_error(ctr.h).decode()
    assert "600" in msg and "10" in msg, msg
    _check(native, ctr, data, rows, 1, (0, 1), 0, buf=buf)                   # and the context goes on


def test_filter_states(native, tables, two_sources):
    k = 31
    ctr, T = tables(k, b"", False)
    data = two_sources[317 * 900:317 * 1100]
    rows = _model_rows(_synth_digits(data), T, k, b"", False, 1)
    buf = _dev(data)
    # an empty table: every hits is 0
    empty = native.Counter(k=k, prefix=b"", flags=native.FLAG_UNORDERED)
    assert _status(native, lambda: empty.table_filter(data)) == E_STATE       # no finish yet
    assert _status(native, lambda: empty.table_filter_device(buf.data_ptr(), len(data))) == E_STATE
    tiny = _dev(b"@r\nAC\n+\nII\n")
    empty.reset()
    empty.feed_device(tiny.data_ptr(), 11)
    empty.finish(want_result=False)
    assert empty.table_stats()[0] == 0
    rows0 = rows.copy()
    rows0[:, 1] = rows0[:, 3] = 0
    out, keep, res = _check(native, empty, data, rows0, 1, (0, 1), 0)
    assert res["n_kept"] == 0 and res["n_reads"] == 200
    out, keep, res = _check(native, empty, data, rows0, 1, (0, 1), FILTER_DROP)
    assert out == data
    empty.close()
    # contexts that cannot filter
    ordered = native.Counter(k=16, prefix=b"ATGAC")
    ordered.count_buffer(data)
    assert _status(native, lambda: ordered.table_filter(data)) == E_STATE
    assert _status(native, lambda: ordered.table_filter_device(buf.data_ptr(), len(data))) == E_STATE
    ordered.close()
    fasta = native.Counter(k=k, prefix=b"", flags=native.FLAG_UNORDERED | native.FLAG_FASTA)
    fasta.count_buffer(b">a\n" + _key_bytes(_synth_digits(data)[:1]) + b"\n")
    assert _status(native, lambda: fasta.table_filter(data)) == E_STATE
    assert _status(native, lambda: fasta.table_filter_device(buf.data_ptr(), len(data))) == E_STATE
    fasta.close()
    # non-ASCII input is refused as in the screen; a lookup and a second filter on the same context succeed
    keys = _key_bytes(_synth_digits(data)[:5, 20:20 + k])
    looked = ctr.table_lookup(keys).tolist()
    bad = bytearray(data)
    bad[5000] = 0x80
    assert _status(native, lambda: ctr.table_filter(bytes(bad))) == E_NONASCII
    assert _status(native, lambda: ctr.table_filter_device(_dev(bytes(bad)).data_ptr(), len(bad))) == E_NONASCII
    assert ctr.table_lookup(keys).tolist() == looked and sum(looked) > 0
    out, keep, res = _check(native, ctr, data, rows, 1, (0, 1), 0, buf=buf)
    assert keep == [True] * 100 + [False] * 100
