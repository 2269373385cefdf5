"""GPU parity of the calls that relate two tables (kmer_table_compare,
kmer_table_setop_device, kmer_table_setop; kmer_setops.hip) and of the
matcher's exclude route.  Every comparison is exact.  Expected values come
from the CPU restatement's Maps (oracle.count_arrays, oracle.count_buffer for
record keys) joined with numpy / Python set operations, never from the
library's own results."""
import math

import numpy as np
import pytest

from oracle import kmerfinder_oracle as ko
from tests import test_table_lookup_gpu as L

pytestmark = pytest.mark.gpu

FIELDS = ("keys_a", "keys_b", "keys_both", "total_a", "total_b", "shared_a", "shared_b", "sum_min")
PAIRS = [(1, 1), (2, 1), (1, 3), (3, 2)]


@pytest.fixture(scope="module")
def native():
    from kmerjs_amd import _native
    return _native


@pytest.fixture(scope="module")
def kf():
    from kmerjs_amd import kmerfinder
    return kmerfinder


def _host_inputs():
    """A = synthetic reads 0..2999, read i repeated i % 5 + 1 times; B = reads
    1500..4499 of the same seed, read i repeated i % 3 + 1 times: 1,500 shared
    reads at different multiplicities."""
    from oracle import oracle
    raw = oracle.synth_fastq(3, 0, 4500)
    read = lambda i: raw[317 * i:317 * (i + 1)]
    a = b"".join(read(i) * (i % 5 + 1) for i in range(0, 3000))
    b = b"".join(read(i) * (i % 3 + 1) for i in range(1500, 4500))
    return a, b


@pytest.fixture(scope="module")
def data():
    """((device buffer, host bytes) of A, the same of B)."""
    import torch
    a, b = _host_inputs()
    assert len(a) == 9000 * 317 and len(b) == 6000 * 317
    dev = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).cuda()
    return (dev(a), a), (dev(b), b)


_MAPS = {}


def _raw_maps(data, prefix, k):
    from oracle import oracle
    if (prefix, k) not in _MAPS:
        out = []
        for _, host in data:
            keys, cnt = oracle.count_arrays(host, prefix, k)
            d = L._LUT[keys]
            assert (d < 4).all()                              # all-A/C/G/T inputs: no record keys
            out.append((d, L._pack(d), cnt.astype(np.uint64)))
        _MAPS.clear()                                         # (one shape at a time)
        _MAPS[(prefix, k)] = out
    return _MAPS[(prefix, k)]


def _omaps(data, prefix, k, canonical):
    """The expected Maps of A and B as (codes ascending, values)."""
    out = []
    for d, code, cnt in _raw_maps(data, prefix, k):
        if canonical:                          # one key per class: the smaller string, counted per forward window
            r = L._pack(L._rc(d))
            keep = code <= r
            cnt = np.where(code == r, cnt // np.uint64(2), cnt)[keep]
            code = code[keep]
        o = np.argsort(code)
        out.append((code[o], cnt[o]))
    return out


def _digits(code, k):
    """Digit rows (A C G T = 0 1 2 3) of 2-bit codes, first base most significant."""
    out = np.empty((len(code), k), dtype=np.uint8)
    for j in range(k):
        out[:, j] = (code >> np.uint64(2 * (k - 1 - j))) & np.uint64(3)
    return out


class Want:
    """The join of two Maps given as (codes ascending, values): the compare struct and the three results."""

    def __init__(self, ma, mb, k):
        self.k = k
        self.code = np.union1d(ma[0], mb[0])
        self.va = L._get(ma[0], ma[1], self.code)
        self.vb = L._get(mb[0], mb[1], self.code)
        self.rows = L._ACGT[_digits(self.code, k)]            # key bytes, row per key, ascending

    def sides(self, min_a, min_b):
        return self.va >= np.uint64(max(min_a, 1)), self.vb >= np.uint64(max(min_b, 1))

    def compare(self, min_a, min_b):
        ia, ib = self.sides(min_a, min_b)
        both = ia & ib
        s = lambda x: int(x.sum(dtype=np.uint64))
        return {"keys_a": s(ia), "keys_b": s(ib), "keys_both": s(both), "total_a": s(self.va[ia]),
                "total_b": s(self.vb[ib]), "shared_a": s(self.va[both]), "shared_b": s(self.vb[both]),
                "sum_min": s(np.minimum(self.va, self.vb)[both])}

    def setop(self, op, min_a, min_b):
        ia, ib = self.sides(min_a, min_b)
        zero = np.uint64(0)
        if op == 0:
            sel, val = ia & ib, np.minimum(self.va, self.vb)
        elif op == 1:
            sel, val = ia & ~ib, self.va
        else:
            sel, val = ia | ib, np.where(ia, self.va, zero) + np.where(ib, self.vb, zero)
        return self.rows[sel].tobytes(), val[sel]


def _device_setop(a, b, op, min_a=1, min_b=1):
    """table_setop_device copied to the host through torch: (key bytes, values)."""
    import torch
    from kmerjs_amd.multi import _CudaArray, device_u64
    d_keys, d_counts, n = a.table_setop_device(b, op, min_a, min_b)
    if n == 0:
        return b"", np.zeros(0, dtype=np.uint64)
    assert d_keys and d_counts
    dev = torch.device("cuda", torch.cuda.current_device())
    keys = torch.as_tensor(_CudaArray(d_keys, n * a.k, "|u1"), device=dev).cpu().numpy().tobytes()
    return keys, device_u64(d_counts, n, dev).cpu().numpy().view(np.uint64).copy()


def _compare(a, b, min_a=1, min_b=1):
    out = a.table_compare(b, min_a, min_b)
    either = out["keys_a"] + out["keys_b"] - out["keys_both"]
    assert out.pop("jaccard") == (out["keys_both"] / either if either else 0.0)
    assert out.pop("containment_a") == (out["keys_both"] / out["keys_a"] if out["keys_a"] else 0.0)
    assert tuple(out) == FIELDS
    return out


def _flags(native, canonical, extra=0):
    return (native.FLAG_CANONICAL if canonical else native.FLAG_UNORDERED) | extra


def _check_pair(native, a, b, want, pairs=PAIRS, host_pair=(2, 1)):
    """compare and the three device results for every threshold pair, the host result for one,
    the identities at (1, 1), and both tables untouched."""
    before = [(c.table_digest(), c.table_stats()) for c in (a, b)]
    k = a.k
    for min_a, min_b in pairs:
        cmp = _compare(a, b, min_a, min_b)
        assert cmp == want.compare(min_a, min_b), (min_a, min_b)
        got = {}
        for op in (native.SETOP_INTERSECT, native.SETOP_SUBTRACT, native.SETOP_UNION):
            wk, wv = want.setop(op, min_a, min_b)
            keys, vals = _device_setop(a, b, op, min_a, min_b)
            assert len(vals) == len(wv) and keys == wk and np.array_equal(vals, wv), (op, min_a, min_b)
            got[op] = vals
            if (min_a, min_b) == host_pair:
                r = a.table_setop(b, op, min_a, min_b)
                assert r.keybuf == wk and np.array_equal(r.counts, wv)
                assert np.array_equal(r.offsets, np.arange(len(wv) + 1, dtype=np.uint64) * np.uint64(k))
        if (min_a, min_b) == (1, 1):
            _, keys_a, total_a = a.table_stats()
            _, keys_b, total_b = b.table_stats()
            assert (cmp["keys_a"], cmp["total_a"], cmp["keys_b"], cmp["total_b"]) == (keys_a, total_a, keys_b, total_b)
            assert cmp["keys_both"] <= min(keys_a, keys_b)
            assert len(got[0]) == cmp["keys_both"] and len(got[1]) == keys_a - cmp["keys_both"]
            assert len(got[2]) == keys_a + keys_b - cmp["keys_both"]
            assert int(got[0].sum(dtype=np.uint64)) == cmp["sum_min"]
    assert [(c.table_digest(), c.table_stats()) for c in (a, b)] == before


def _check_self(native, a, ma, min_v=2):
    """compare and the setops of a table with itself."""
    code, val = ma
    sel = val >= np.uint64(min_v)
    n, tot = int(sel.sum()), int(val[sel].sum(dtype=np.uint64))
    assert _compare(a, a, min_v, min_v) == {"keys_a": n, "keys_b": n, "keys_both": n, "total_a": tot, "total_b": tot,
                                            "shared_a": tot, "shared_b": tot, "sum_min": tot}
    rows = L._ACGT[_digits(code[sel], a.k)].tobytes()
    keys, vals = _device_setop(a, a, native.SETOP_UNION, min_v, min_v)
    assert keys == rows and np.array_equal(vals, val[sel] * np.uint64(2))
    keys, vals = _device_setop(a, a, native.SETOP_INTERSECT, min_v, min_v)
    assert keys == rows and np.array_equal(vals, val[sel])
    assert a.table_setop_device(a, native.SETOP_SUBTRACT, min_v, min_v) == (0, 0, 0)
    keys, vals = _device_setop(a, a, native.SETOP_SUBTRACT, 1, min_v)    # in A, below B's threshold
    low = val < np.uint64(min_v)
    assert keys == L._ACGT[_digits(code[low], a.k)].tobytes() and np.array_equal(vals, val[low])


# (k, prefix): wide and narrow keys, both sides of k = 21 / 22, odd and even k, with and without a prefix;
# k = 6 / 4: a few hundred keys with large values, nearly all of them in both Maps
SHAPES = [(31, b""), (22, b"AC"), (21, b""), (21, b"AC"), (16, b"ATGAC"), (32, b"T"), (6, b""), (4, b"A")]


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,prefix", SHAPES)
def test_compare_and_setops_equal_the_join_of_the_oracle_maps(native, data, k, prefix, canonical):
    (buf_a, host_a), (buf_b, host_b) = data
    ma, mb = _omaps(data, prefix, k, canonical)
    want = Want(ma, mb, k)
    ia, ib = want.sides(1, 1)
    if k >= 16:                                # A-only, B-only and shared keys; the thresholds move keys between them
        assert (ia & ~ib).sum() > 50 and (ib & ~ia).sum() > 50 and (ia & ib).sum() > 50
        for pair in PAIRS[1:]:
            ja, jb = want.sides(*pair)
            assert (ja & jb).sum() < (ia & ib).sum() and not np.array_equal(ja & ~jb, ia & ~ib)
    else:
        assert (ia & ib).any() and len(want.code) <= 4 ** k
    a = L._fed(native, buf_a, len(host_a), k, prefix, _flags(native, canonical))
    b = L._fed(native, buf_b, len(host_b), k, prefix, _flags(native, canonical))
    _check_pair(native, a, b, want)
    _check_self(native, a, ma)
    a.close()
    b.close()


@pytest.mark.parametrize("route", ["chunks", "fixed", "split"])
def test_setops_of_tables_with_different_layouts(native, data, route):
    # one side fed in three chunks, or built by the fixed-capacity route / the general final kernel:
    # the two tables hold the same classes at different places
    (buf_a, host_a), (buf_b, host_b) = data
    k, prefix, canonical = (21, b"AC", True) if route == "split" else (31, b"", False)
    ma, mb = _omaps(data, prefix, k, canonical)
    want = Want(ma, mb, k)
    extra = {"chunks": 0, "fixed": native.FLAG_TABLE_FIXED_TEST, "split": native.FLAG_TABLE_SPLIT_TEST}[route]
    cuts = [0, 317 * 2999, 317 * 3000, len(host_a)] if route == "chunks" else None
    a = L._fed(native, buf_a, len(host_a), k, prefix, _flags(native, canonical, extra), cuts=cuts)
    b = L._fed(native, buf_b, len(host_b), k, prefix, _flags(native, canonical))
    if route == "fixed":
        assert a.table_routes()["p2_fixed"] == 1
    _check_pair(native, a, b, want, pairs=[(1, 1), (3, 2)], host_pair=(3, 2))
    _check_pair(native, b, a, Want(mb, ma, k), pairs=[(2, 1)], host_pair=None)
    a.close()
    b.close()


# ---- small Maps as dicts: key bytes -> value, record keys included ----
def _join_dicts(ma, mb, min_a=1, min_b=1):
    A = {x: v for x, v in ma.items() if v >= max(min_a, 1)}
    B = {x: v for x, v in mb.items() if v >= max(min_b, 1)}
    both = A.keys() & B.keys()
    cmp = {"keys_a": len(A), "keys_b": len(B), "keys_both": len(both), "total_a": sum(A.values()),
           "total_b": sum(B.values()), "shared_a": sum(A[x] for x in both), "shared_b": sum(B[x] for x in both),
           "sum_min": sum(min(A[x], B[x]) for x in both)}
    ops = {0: sorted((x, min(A[x], B[x])) for x in both),
           1: sorted((x, v) for x, v in A.items() if x not in B),
           2: sorted((x, A.get(x, 0) + B.get(x, 0)) for x in A.keys() | B.keys())}
    return cmp, ops


def _acgt(rows):
    return [(x, v) for x, v in rows if not x.translate(None, b"ACGT")]


def _check_dicts(native, a, b, ma, mb, pairs=((1, 1),), host=True):
    for min_a, min_b in pairs:
        cmp, ops = _join_dicts(ma, mb, min_a, min_b)
        assert _compare(a, b, min_a, min_b) == cmp, (min_a, min_b)
        for op, rows in ops.items():
            dev = _acgt(rows)                                 # the device result holds no record keys
            keys, vals = _device_setop(a, b, op, min_a, min_b)
            assert keys == b"".join(x for x, _ in dev) and vals.tolist() == [v for _, v in dev], (op, min_a, min_b)
            if host:
                assert a.table_setop(b, op, min_a, min_b).entries() == rows, (op, min_a, min_b)
    return cmp, ops


def _records(rows, k, mult):
    """FASTQ records of one k-mer each, record i repeated mult(i) times."""
    return b"".join((b"@r%d\n%s\n+\n%s\n" % (i, L._key_bytes(row[None, :]), b"I" * k)) * mult(i)
                    for i, row in enumerate(rows))


def _bucket_lens(ctr):
    import torch
    from kmerjs_amd.multi import _CudaArray
    ln = ctr.table_device()[2]
    return torch.as_tensor(_CudaArray(ln, 1 << 20, "<i4"), device=torch.device("cuda", torch.cuda.current_device()))


def _one_bucket_wide(k, q, rem_bits, need):
    """Canonical k-mers (k = 31) of bucket q with remainders below 2^rem_bits
    (test_lookup_scans_a_long_bucket's construction)."""
    rng = np.random.default_rng(rem_bits)
    rem = np.unique(rng.integers(0, 1 << rem_bits, 24 * need, dtype=np.uint64))
    rem = rem[rng.permutation(len(rem))]
    h = (np.uint64(q) << np.uint64(44)) | rem
    with np.errstate(over="ignore"):
        c = h * np.uint64(L._INV)
    c = c[c < np.uint64(1 << 62)]
    d = L._planar_digits(c, k)
    d = d[c <= L._planar(L._rc(d))][:need]
    assert len(d) == need
    return d


def _one_bucket_narrow(k, q, need):
    """Canonical k-mers (k = 20) of bucket q: the header's narrow-key inverse.  h = f(c) << 23 with
    f(c) = q << 21 | r for 21-bit remainders r; z = f(c) * MUL^-1 mod 2^41, c = z ^ (z >> 21); kept
    when c < 2^40 is the smaller planar code of its class (even k: the table's key code)."""
    rng = np.random.default_rng(k)
    r = rng.permutation(1 << 21)[:16 * need].astype(np.uint64)
    f = (np.uint64(q) << np.uint64(21)) | r
    with np.errstate(over="ignore"):
        z = (f * np.uint64(L._INV)) & np.uint64((1 << 41) - 1)
    c = z ^ (z >> np.uint64(21))
    c = c[c < np.uint64(1 << (2 * k))]
    d = L._planar_digits(c, k)
    d = d[c <= L._planar(L._rc(d))][:need]
    assert len(d) == need
    return d


def _long_pair(native, rows, k, q):
    """A = rows [0, m) with every 97th record tripled, B = rows [m / 2, 3 m / 2) with every 89th doubled,
    m = ceil(2.5 x JOIN_TILE): the tables (one bucket of m entries each) and the oracle's Maps."""
    from oracle import oracle
    m = math.ceil(2.5 * native.JOIN_TILE)
    assert len(rows) >= m // 2 + m and m > 2 * native.JOIN_TILE
    text_a = _records(rows[:m], k, lambda i: 3 if i % 97 == 0 else 1)
    text_b = _records(rows[m // 2:m // 2 + m], k, lambda i: 2 if i % 89 == 0 else 1)
    ctrs, maps = [], []
    for text in (text_a, text_b):
        c = native.Counter(k=k, prefix=b"", flags=native.FLAG_UNORDERED)
        c.count_buffer(text)
        lens = _bucket_lens(c)
        assert int(lens[q]) == m and int(lens.sum()) == m     # the test's point: one long bucket on each side
        ctrs.append(c)
        maps.append(dict(oracle.count_buffer(text, b"", k, 1)))
    return ctrs, maps, m


@pytest.mark.parametrize("rem_bits", [44, 30])
def test_long_buckets_are_joined_in_lds(native, rem_bits):
    # rem_bits 30: the remainders' top 14 bits are equal, so the ranges of the staged side must deepen
    from oracle import oracle
    k, q = 31, 0x5A5A5
    m = math.ceil(2.5 * native.JOIN_TILE)
    rows = _one_bucket_wide(k, q, rem_bits, m // 2 + m + 10)
    (a, b), (ma, mb), m = _long_pair(native, rows, k, q)
    _check_dicts(native, a, b, ma, mb, pairs=((1, 1), (2, 1), (1, 2), (3, 2)), host=False)
    assert _join_dicts(ma, mb)[0]["keys_both"] == 2 * (m - m // 2)     # rows [m / 2, m), both orientations
    _check_dicts(native, b, a, mb, ma, pairs=((1, 1), (2, 3)), host=False)
    _check_dicts(native, a, a, ma, ma, pairs=((1, 1),), host=False)
    # long against empty (a tiny input of another bucket: bucket q of the other table is empty) and
    # long against short (10 of A's k-mers), both argument orders
    tiny = _records(_one_bucket_wide(k, q ^ 1, 44, 10), k, lambda i: 1)
    short = _records(rows[5:15], k, lambda i: 4)
    for text in (tiny, short):
        c = native.Counter(k=k, prefix=b"", flags=native.FLAG_UNORDERED)
        c.count_buffer(text)
        mc = dict(oracle.count_buffer(text, b"", k, 1))
        assert int(_bucket_lens(c)[q]) == (0 if text is tiny else 10) and int(_bucket_lens(c).sum()) == 10
        _check_dicts(native, a, c, ma, mc, pairs=((1, 1), (3, 2)), host=False)
        _check_dicts(native, c, a, mc, ma, pairs=((1, 1), (2, 3)), host=False)
        assert _join_dicts(ma, mc)[0]["keys_both"] == (0 if text is tiny else 20)
        c.close()
    a.close()
    b.close()


def test_long_narrow_bucket_is_joined_in_lds(native):
    k, q = 20, 0x3C3C3
    m = math.ceil(2.5 * native.JOIN_TILE)
    rows = _one_bucket_narrow(k, q, m // 2 + m + 10)
    (a, b), (ma, mb), m = _long_pair(native, rows, k, q)
    _check_dicts(native, a, b, ma, mb, pairs=((1, 1), (2, 1), (3, 2)), host=False)
    _check_dicts(native, b, a, mb, ma, pairs=((1, 2),), host=False)
    a.close()
    b.close()


@pytest.mark.parametrize("k", [15, 16])
def test_palindromes_and_big_counts_through_compare_and_setops(native, k):
    # poly-A reads: one class seen > 2^20 times (its count lies in the big list); AT-repeats: palindromes
    # at even k (doubled in table mode).  9,000 / 4,500 poly-A reads: the big list on A's side only;
    # 18,000 / 9,000: on both sides
    from oracle import oracle
    at = b"".join(b"@s%010d\n%s\n+\n%s\n" % (i, b"AT" * 75, b"I" * 150) for i in range(300))
    polya = lambda n: b"".join(b"@r%010d\n%s\n+\n%s\n" % (i, b"A" * 150, b"I" * 150) for i in range(n))
    texts = {n: polya(n) + at for n in (4500, 9000, 18000)}
    maps = {n: dict(oracle.count_buffer(t, b"", k, 1)) for n, t in texts.items()}
    assert maps[4500][b"A" * k] < (1 << 20) - 1 <= maps[9000][b"A" * k] < maps[18000][b"A" * k]
    for canonical in (False, True):
        ctrs = {}
        for n, t in texts.items():
            ctrs[n] = native.Counter(k=k, prefix=b"", flags=_flags(native, canonical))
            ctrs[n].count_buffer(t)
        for na, nb in ((9000, 4500), (18000, 9000), (9000, 18000)):
            ma, mb = maps[na], maps[nb]
            if canonical:
                ma, mb = L._canonical_from_map(ma), L._canonical_from_map(mb)
            _check_dicts(native, ctrs[na], ctrs[nb], ma, mb, pairs=((1, 1), (1 << 20, 2), (2, 1 << 20)))
            cmp, ops = _join_dicts(ma, mb)
            big = min(na, nb) * (151 - k)
            assert (b"A" * k, big) in ops[0] and (b"A" * k, (na + nb) * (151 - k)) in ops[2] and cmp["sum_min"] > big
            if k == 16:
                pal = b"AT" * 8
                assert dict(ops[0])[pal] == ma[pal] == mb[pal] and dict(ops[2])[pal] == 2 * ma[pal]
                assert canonical or ma[pal] % 2 == 0
        for c in ctrs.values():
            c.close()


@pytest.mark.parametrize("k,prefix,canonical", [(16, b"", False), (21, b"GT", False), (21, b"", True), (16, b"A", True)])
def test_record_keys_in_compare_and_the_host_setop(native, k, prefix, canonical):
    # keys with N / lowercase live on the host: joined there by the same rules, in compare and the
    # host setop, absent from the device setop.  Two seeds over the same reads: shared record keys
    from oracle import oracle
    texts = (L._n_rich(600, 12), L._n_rich(600, 13))
    maps, ctrs = [], []
    for t in texts:
        m = dict(oracle.count_buffer(t, prefix, k, 1))
        maps.append(L._canonical_from_map(m) if canonical else m)
        ctrs.append(native.Counter(k=k, prefix=prefix, flags=_flags(native, canonical)))
        ctrs[-1].count_buffer(t)
    rec = [{x for x in m if any(ch not in b"ACGT" for ch in x)} for m in maps]
    assert rec[0] and rec[1] and rec[0] != rec[1]
    if not prefix:                                            # (a key that starts with N fails a prefix)
        assert len(rec[0] & rec[1]) > 20 and len(rec[0] - rec[1]) > 20 and len(rec[1] - rec[0]) > 20
    _check_dicts(native, ctrs[0], ctrs[1], maps[0], maps[1], pairs=((1, 1), (2, 1), (1, 2)))
    _check_dicts(native, ctrs[1], ctrs[1], maps[1], maps[1], pairs=((1, 1),))
    for c in ctrs:
        c.close()


def test_states_parameters_empty_tables_and_reuse(native):
    import torch
    from kmerjs_amd.multi import _CudaArray
    from oracle import oracle
    raw = oracle.synth_fastq(3, 0, 600)                       # two small inputs that share reads 200..399
    host_a = b"".join(raw[317 * i:317 * (i + 1)] * (i % 3 + 1) for i in range(0, 400))
    host_b = b"".join(raw[317 * i:317 * (i + 1)] * (i % 2 + 1) for i in range(200, 600))
    buf_b = torch.frombuffer(bytearray(host_b), dtype=torch.uint8).cuda()
    k, n = 21, len(host_b)
    mk = lambda kk=k, prefix=b"", flags=native.FLAG_UNORDERED, **kw: native.Counter(k=kk, prefix=prefix, flags=flags, **kw)
    a = mk()
    a.count_buffer(host_a)
    calls = (lambda x, y: x.table_compare(y), lambda x, y: x.table_setop_device(y, 1), lambda x, y: x.table_setop(y, 2))

    def refused(x, y, status):
        for call in calls:
            with pytest.raises(native.KmerError) as e:
                call(x, y)
            assert e.value.status == status, (status, str(e.value))

    for other in (mk(kk=22), mk(flags=native.FLAG_CANONICAL), mk(prefix=b"A")):    # k, mode, prefix: bad parameter
        other.count_buffer(host_b)
        refused(a, other, 2)
        refused(other, a, 2)
        other.close()
    with pytest.raises(native.KmerError) as e:
        a.table_setop_device(a, 3)
    assert e.value.status == 2
    b = mk()
    refused(a, b, 8)                                          # no finish on b yet
    b.reset()
    refused(b, a, 8)
    b.feed_device(buf_b.data_ptr(), n)
    refused(a, b, 8)                                          # fed, not finished
    ordered = native.Counter(k=k, prefix=b"")                 # an ordered-mode context has no table
    ordered.count_buffer(host_b[:317 * 200])
    refused(a, ordered, 8)
    refused(ordered, a, 8)
    ordered.close()
    grp = mk(devices=[0, 0])
    grp.count_buffer(host_b[:317 * 200])
    refused(a, grp, 8)
    refused(grp, a, 8)
    grp.close()
    b.finish(want_result=False)
    ma = dict(oracle.count_buffer(host_a, b"", k, 1))
    mb = dict(oracle.count_buffer(host_b, b"", k, 1))
    before = [(c.table_digest(), c.table_stats()) for c in (a, b)]
    cmp, ops = _check_dicts(native, a, b, ma, mb, pairs=((1, 1), (2, 2)), host=True)
    assert cmp["keys_both"] > 0 and ops[1] and ops[0]
    assert [(c.table_digest(), c.table_stats()) for c in (a, b)] == before
    # the result lives in a: it survives a reset of b, and the next extract on a replaces it
    d_keys, d_counts, cnt = a.table_setop_device(b, native.SETOP_SUBTRACT)
    want = _join_dicts(ma, mb)[1][1]
    b.reset()
    dev = torch.device("cuda", torch.cuda.current_device())
    keys = torch.as_tensor(_CudaArray(d_keys, cnt * k, "|u1"), device=dev).cpu().numpy().tobytes()
    assert cnt == len(want) and keys == b"".join(x for x, _ in want)
    e_keys, _, e_n = a.table_extract_device(1, 0)
    assert e_n == len(ma) and e_n != cnt
    keys = torch.as_tensor(_CudaArray(e_keys, e_n * k, "|u1"), device=dev).cpu().numpy().tobytes()
    assert keys == b"".join(sorted(ma))
    # empty tables: on b's side, on a's side, on both
    b.finish(want_result=False)
    empty = {}
    _check_dicts(native, a, b, ma, empty, pairs=((1, 1), (2, 1)))
    _check_dicts(native, b, a, empty, ma, pairs=((1, 1), (1, 2)))
    _check_dicts(native, b, b, empty, empty)
    c = mk()
    c.reset()
    c.finish(want_result=False)
    _check_dicts(native, b, c, empty, empty)
    assert b.table_setop_device(c, native.SETOP_UNION) == (0, 0, 0)
    assert (a.table_digest(), a.table_stats()) == before[0]
    for x in (a, b, c):
        x.close()


@pytest.mark.parametrize("k,flags_name", [(31, "FLAG_UNORDERED"), (21, "FLAG_CANONICAL")])
def test_compare_and_subtract_on_exchanged_tables(native, data, k, flags_name):
    """World 2 in one process (test_lookup_on_exchanged_tables' construction), for A and for B: rank r's
    two tables hold the same buckets, so the ranks' compare structs add up to the one-table answer and
    their SUBTRACT results are disjoint and together equal it."""
    import torch
    from kmerjs_amd.multi import device_u64
    world = 2
    canonical = flags_name == "FLAG_CANONICAL"
    ma, mb = _omaps(data, b"", k, canonical)
    want = Want(ma, mb, k)
    ranks, keep = [], []
    for (buf, host), n_rec in zip(data, (9000, 6000)):
        cuts = [317 * (n_rec * r // world) for r in range(world + 1)]
        ctrs = [native.Counter(k=k, prefix=b"", flags=getattr(native, flags_name)) for _ in range(world)]
        sends = []
        for r, c in enumerate(ctrs):
            c.reset()
            c.feed_device(buf.data_ptr() + cuts[r], cuts[r + 1] - cuts[r])
            dsend, counts, parts = c.table_exchange_prepare(world)
            sends.append((device_u64(dsend, sum(counts), buf.device).clone(), counts, parts))
        parts_all = np.array([p for _, _, p in sends], dtype=np.uint64)
        for o, c in enumerate(ctrs):
            recv = torch.cat([keys[sum(counts[:o]):sum(counts[:o]) + counts[o]] for keys, counts, _ in sends])
            keep.append(recv)
            c.table_finish_exchanged(recv.data_ptr(), recv.numel(), parts_all, world, o,
                                     stream=torch.cuda.current_stream().cuda_stream)
        ranks.append(ctrs)
    for min_a, min_b in ((1, 1), (2, 1)):
        parts = [_compare(ranks[0][r], ranks[1][r], min_a, min_b) for r in range(world)]
        assert {f: parts[0][f] + parts[1][f] for f in FIELDS} == want.compare(min_a, min_b)
        assert all(p["keys_a"] and p["keys_b"] and p["keys_both"] for p in parts)
        ex = [_device_setop(ranks[0][r], ranks[1][r], native.SETOP_SUBTRACT, min_a, min_b) for r in range(world)]
        rows = [[(kb[i * k:(i + 1) * k], int(v)) for i, v in enumerate(vals)] for kb, vals in ex]
        assert rows[0] == sorted(rows[0]) and rows[1] == sorted(rows[1]) and rows[0] and rows[1]
        assert not set(x for x, _ in rows[0]) & set(x for x, _ in rows[1])
        merged = sorted(rows[0] + rows[1])
        wk, wv = want.setop(native.SETOP_SUBTRACT, min_a, min_b)
        assert b"".join(x for x, _ in merged) == wk and [v for _, v in merged] == wv.tolist()
    for ctrs in ranks:
        for c in ctrs:
            c.close()
    del keep


@pytest.mark.parametrize("k,prefix,canonical", [(21, b"", True), (22, b"AC", False)])
def test_find_matches_table_with_an_excluded_sample(native, kf, data, k, prefix, canonical):
    """find_matches_table(a, exclude=b) = the oracle restatement of kmerFinder over the oracle Map of A
    with B's keys removed (sorted by bytes); without `exclude` the result is the table probe's, as before."""
    from tests import test_match_table_gpu as T
    (buf_a, host_a), (buf_b, host_b) = data
    (code_a, cnt_a), (code_b, cnt_b) = _omaps(data, prefix, k, canonical)
    d = _digits(code_a, k)
    whole = (d, cnt_a, code_a, cnt_a)                         # (the tuple test_table_lookup_gpu._oracle_map returns)
    for min_count, exclude_min in ((1, 1), (2, 2)):
        keep = (cnt_a >= min_count) & ~(L._get(code_b, cnt_b, code_a) >= np.uint64(exclude_min))
        cut = (d[keep], cnt_a[keep], code_a[keep], cnt_a[keep])
        db = T._winner_db(whole, k, np.random.default_rng(k))  # templates hold keys of A, in B or not
        summary = T._summary(db)
        tdb = kf.TemplateDB(db, k, summary)
        a = L._fed(native, buf_a, len(host_a), k, prefix, _flags(native, canonical))
        b = L._fed(native, buf_b, len(host_b), k, prefix, _flags(native, canonical))
        q0 = T._query(cut, db, k)
        full = T._query(whole, db, k)
        assert 0 < len(q0) < len(full)
        size = int(keep.sum())                                # kmerMapSize of the depleted Map
        qo = dict(q0)
        want = ko.winner_scoring(qo, db, summary, size)
        assert len(want) >= 2                                 # the loop is not vacuous
        deleted = sorted(km.encode() for km in q0 if km not in qo)
        assert len(deleted) >= 100
        args = dict(min_count=min_count, exclude=b, exclude_min=exclude_min)
        got, removed = kf.KmerFinder(tdb, "winner").find_matches_table(a, with_removed=True, **args)
        assert got == want and removed == deleted
        assert kf.KmerFinder(tdb, "winner").find_matches_table(a, query_size=size, **args) == want
        assert kf.KmerFinder(tdb, "standard").find_matches_table(a, **args) == ko.standard_scoring(dict(q0), db, summary, size)
        # without exclude: exactly what the table probe returns
        want1 = ko.winner_scoring(dict(full), db, summary, len(cnt_a))
        assert kf.KmerFinder(tdb, "winner").find_matches_table(a) == want1 and want1 != want
        a.close()
        b.close()
        tdb.close()
