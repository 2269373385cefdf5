"""GPU parity of template matching straight from a table-mode count
(kmer_match_open_table, kmer_db_kmers; kmer_probe.hip): the query is the Map
the counter's finished table describes, probed on the device from the DB's
side.  Expected values come from the oracle: the CPU restatement's Map
(canonical counts derived from it as test_table_gpu.py::_canonical_from_map
does), SORTED BY KEY BYTES -- the order of the table's host result and of the
DB's distinct k-mers -- fed to the oracle restatement of kmerFinder
(oracle/kmerfinder_oracle.py).  Keys of that Map which no template holds
contribute nothing to any score, to the order of the rest or to the removals,
so the large Maps are cut down to the DB's k-mers before the Python loops run
over them; kmerMapSize stays the whole Map's."""
import numpy as np
import pytest

from oracle import kmerfinder_oracle as ko
from tests import test_table_lookup_gpu as L

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def native():
    from kmerjs_amd import _native
    return _native


@pytest.fixture(scope="module")
def kf():
    from kmerjs_amd import kmerfinder
    return kmerfinder


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


# ---- helpers ------------------------------------------------------------------
def _strs(d):
    """Digit rows -> list of str."""
    k = d.shape[1]
    raw = L._key_bytes(d).decode("latin-1")
    return [raw[i * k:(i + 1) * k] for i in range(len(d))]


def _digits(kms, k):
    return L._LUT[np.frombuffer("".join(kms).encode("latin-1"), dtype=np.uint8)].reshape(-1, k)


def _template(t, kms):
    return {"sequence": "T%03d" % t, "lengths": 2 * len(kms) + 7, "ulength": max(1, len(set(kms))),
            "species": "sp %d" % t, "kmers": kms}


def _summary(db):
    return {"templates": len(db), "totalLen": sum(t["lengths"] for t in db),
            "uniqueLens": sum(t["ulength"] for t in db)}


def _make_db(m, k, prefix, rng, nt=40, own=200):
    """~nt templates x ~400 k-mers: Map keys from disjoint ranges of the Map (in
    its own order: disjoint reads), reverse complements of such keys, keys
    shared between templates, ~25 % random absent k-mers (half of them with
    the prefix), keys that fail the prefix, duplicates inside a template, and
    one empty template."""
    d = m[0]
    n = len(d)
    pd = L._LUT[np.frombuffer(prefix, dtype=np.uint8)]
    common = d[rng.choice(n, 300, replace=False)]
    db = []
    for t in range(nt):
        if t == 7:
            db.append(_template(t, []))
            continue
        lo, hi = n * t // nt, n * (t + 1) // nt
        mine = d[lo + rng.choice(hi - lo, min(own, (hi - lo) * 3 // 4), replace=False)]
        absent = rng.integers(0, 4, (100, k), dtype=np.uint8)
        absent[:50, :len(pd)] = pd
        parts = [mine, L._rc(d[lo + rng.integers(0, hi - lo, 40)]), common[rng.choice(300, 40, replace=False)], absent]
        if len(pd):
            bad = mine[:30].copy()
            bad[:, 0] = (bad[:, 0] + rng.integers(1, 4, len(bad))) % 4
            parts.append(bad.astype(np.uint8))
        rows = np.concatenate(parts)
        rows = np.concatenate([rows, rows[rng.integers(0, len(rows), 20)]])      # duplicates inside the template
        db.append(_template(t, _strs(rows[rng.permutation(len(rows))])))
    return db


def _query(m, db, k):
    """The oracle Map sorted by key bytes, cut down to the DB's k-mers: str -> count."""
    kms = sorted({km for t in db for km in t["kmers"]})
    if not kms:
        return {}
    vals = L._get(m[2], m[3], L._pack(_digits(kms, k)))
    return {km: int(v) for km, v in zip(kms, vals) if v}


def _round1(kf, tdb, db, ctr, q):
    """Round 1 of a table match against the oracle's; returns what it read."""
    try:
        tpls, hits = ko.first_round(dict(q), db, ko.build_index(db))
    except ko.NoHits:
        tpls, hits = {}, 0
    m = kf.Match(tdb, table=ctr)
    try:
        assert m.n == tdb.info()["distinct"]
        got, gdb, w = m.templates(0), m.templates(1), m.winner()
        assert [db[t]["sequence"] for t, _, _ in got] == list(tpls.keys())                  # first-hit order
        assert [(u, s) for _, u, s in got] == [(v["uScore"], v["tScore"]) for v in tpls.values()]
        assert gdb == sorted(got)                                                            # DB order
        assert w.hits == hits == sum(u for _, u, _ in got)
        if tpls:
            name, best = sorted(tpls.items(), key=lambda kv: -kv[1]["uScore"])[0]
            assert db[w.tmpl]["sequence"] == name
            assert (w.uscore, w.tscore, w.first_uscore, w.first_tscore) == (best["uScore"], best["tScore"]) * 2
            # the winner's k-mers: DB indices, ascending = the oracle's Set in query order
            idx = m.template_kmers(w.tmpl)
            allk = tdb.kmers()
            assert [allk[i].decode() for i in idx] == list(best["kmers"].keys())
        else:
            assert w.tmpl == NONE
        assert not m.removed().any() and len(m.removed()) == m.n
        return got, gdb, (w.tmpl, w.uscore, w.tscore, w.hits)
    finally:
        m.close()


def _flags(native, canonical):
    return native.FLAG_CANONICAL if canonical else native.FLAG_UNORDERED


MODES = [(31, b"", False), (32, b"GT", False), (22, b"", False), (21, b"A", False), (21, b"", True),
         (16, b"ATGAC", False), (16, b"", True), (15, b"T", False)]


@pytest.mark.parametrize("k,prefix,canonical", MODES)
def test_table_match_encodings_and_modes(native, kf, reads, k, prefix, canonical):
    # wide and narrow keys, odd and even narrow k, both modes; fed whole and in chunks
    buf, host = reads
    m = L._oracle_map(host, prefix, k, canonical)
    db = _make_db(m, k, prefix, np.random.default_rng(100 + k))
    q = _query(m, db, k)
    assert len(q) > 39 * 120                             # the join is not vacuous
    tdb = kf.TemplateDB(db, k)
    ctr = L._fed(native, buf, len(host), k, prefix, _flags(native, canonical))
    assert ctr.table_stats()[1] == len(m[2])             # the Map the table stands for
    before = (ctr.table_digest(), ctr.table_stats())
    whole = _round1(kf, tdb, db, ctr, q)
    assert (ctr.table_digest(), ctr.table_stats()) == before
    ctr.close()
    cuts = [0, 317 * 7001, 317 * 7002, 317 * 19000, len(host)]
    ctr = L._fed(native, buf, len(host), k, prefix, _flags(native, canonical), cuts=cuts)
    assert _round1(kf, tdb, db, ctr, q) == whole
    ctr.close()
    tdb.close()


def _winner_db(m, k, rng, present=(2, 9, 17, 25), nt=30):
    """Templates of which `present` hold up to 300 Map keys each (disjoint
    ranges) and the others 3: the winner loop takes the present ones, then
    ends on an insignificant winner."""
    d = m[0]
    n = len(d)
    db = []
    for t in range(nt):
        lo, hi = n * t // nt, n * (t + 1) // nt
        take = min(300, (hi - lo) * 4 // 5) if t in present else 3
        mine = d[lo + rng.choice(hi - lo, take, replace=False)]
        rows = np.concatenate([mine, rng.integers(0, 4, (400 - take, k), dtype=np.uint8)])
        db.append(_template(t, _strs(rows[rng.permutation(len(rows))])))
    return db


@pytest.mark.parametrize("k,prefix,canonical", [(16, b"ATGAC", False), (21, b"", True)])
def test_find_matches_table_matches_oracle(native, kf, reads, k, prefix, canonical):
    buf, host = reads
    m = L._oracle_map(host, prefix, k, canonical)
    db = _winner_db(m, k, np.random.default_rng(k))
    summary = _summary(db)
    size = len(m[2])                                     # kmerMapSize of the whole Map
    tdb = kf.TemplateDB(db, k, summary)
    ctr = L._fed(native, buf, len(host), k, prefix, _flags(native, canonical))
    q0 = _query(m, db, k)
    qo = dict(q0)
    want = ko.winner_scoring(qo, db, summary, size)
    assert len(want) >= 3                                # the loop is not vacuous
    deleted = sorted(km.encode() for km in q0 if km not in qo)
    assert len(deleted) >= 3 * 200
    got, removed = kf.KmerFinder(tdb, "winner").find_matches_table(ctr, with_removed=True)
    assert got == want
    assert removed == deleted
    assert kf.KmerFinder(tdb, "winner").find_matches_table(ctr) == want          # query_size defaults to the Map's
    assert kf.KmerFinder(tdb, "winner").find_matches_table(ctr, query_size=size) == want
    want_s = ko.standard_scoring(dict(q0), db, summary, size)
    assert kf.KmerFinder(tdb, "standard").find_matches_table(ctr) == want_s
    assert want_s[0] is not None
    # find_matches over an open table match, as it is
    mt = kf.Match(tdb, table=ctr)
    assert kf.KmerFinder(tdb, "winner").find_matches(None, size, match=mt) == want
    assert sorted(tdb.kmers()[i] for i in np.nonzero(mt.removed())[0]) == deleted
    mt.close()
    # no hits: a DB of absent k-mers, and an empty table
    rng = np.random.default_rng(9)
    miss = [_template(t, _strs(rng.integers(0, 4, (50, k), dtype=np.uint8))) for t in range(3)]
    assert _query(m, miss, k) == {}
    mdb = kf.TemplateDB(miss, k)
    empty = native.Counter(k=k, prefix=prefix, flags=_flags(native, canonical))
    empty.reset()
    empty.finish(want_result=False)
    for method in ("winner", "standard"):
        with pytest.raises(ko.NoHits, match=r"^No hits were found!$"):
            getattr(ko, method + "_scoring")({}, miss, _summary(miss), size)
        with pytest.raises(kf.NoHits, match=r"^No hits were found!$"):
            kf.KmerFinder(mdb, method).find_matches_table(ctr)
        with pytest.raises(kf.NoHits, match=r"^No hits were found!$"):
            kf.KmerFinder(tdb, method).find_matches_table(empty)
    empty.close()
    ctr.close()


@pytest.mark.parametrize("split", [False, True])
def test_table_match_probes_a_long_bucket(native, kf, split):
    """~5,000 distinct 31-mers in ONE bucket (the construction of
    test_lookup_scans_a_long_bucket), and a DB whose k-mers all fall into it:
    thousands of probes of one bucket, in runs that span waves, with x and
    rc x of one class (the same remainder twice in a run) and absent keys."""
    import torch
    from kmerjs_amd.multi import _CudaArray
    from oracle import oracle
    k, bucket = 31, 0x5A5A5
    rng = np.random.default_rng(31)
    rem = np.unique(rng.integers(0, 1 << 44, 120_000, dtype=np.uint64))
    rem = rem[rng.permutation(len(rem))]
    h = (np.uint64(bucket) << np.uint64(44)) | rem
    with np.errstate(over="ignore"):
        c = h * np.uint64(L._INV)                         # (mod 2^64)
    c = c[c < np.uint64(1 << 62)]                         # a 31-mer's planar code ...
    d = L._planar_digits(c, k)
    d = d[c <= L._planar(L._rc(d))]                       # ... and the class's canonical one
    assert len(d) >= 10_000
    written, absent = d[:5000], d[5000:10_000]
    recs = []
    for i, row in enumerate(written):
        rec = b"@r%d\n%s\n+\n%s\n" % (i, L._key_bytes(row[None, :]), b"I" * k)
        recs.append(rec * (3 if i % 97 == 0 else 1))
    data = b"".join(recs)
    omap = dict(oracle.count_buffer(data, b"", k, 1))
    assert len(omap) == 2 * len(written)
    ctr = native.Counter(k=k, prefix=b"", flags=native.FLAG_UNORDERED | (native.FLAG_TABLE_SPLIT_TEST if split else 0))
    ctr.count_buffer(data)
    _, _, ln, _, _ = ctr.table_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    lens = torch.as_tensor(_CudaArray(ln, 1 << 20, "<i4"), device=dev)
    assert int(lens[bucket]) == len(written) and int(lens.sum()) == len(written)   # the test's point: one long bucket
    both = lambda x: np.concatenate([x, L._rc(x)])                               # noqa: E731
    rows = [both(written[:1000]), both(written[800:1800]), both(absent[:1600]),
            np.concatenate([both(written[1500:2500]), absent[1000:2000]]), both(written[4990:])]
    db = [_template(t, _strs(r[rng.permutation(len(r))])) for t, r in enumerate(rows)]
    in_db = {km for t in db for km in t["kmers"]}
    assert len(in_db & {x.decode() for x in omap}) == 2 * 2510 and len(in_db) == 2 * 2510 + 2 * 1600 + 400
    q = {x.decode(): v for x, v in sorted(omap.items())}
    tdb = kf.TemplateDB(db, k)
    before = (ctr.table_digest(), ctr.table_stats())
    got, _, w = _round1(kf, tdb, db, ctr, q)
    assert sorted(t for t, _, _ in got) == [0, 1, 3, 4]
    assert w[3] == 2000 + 2000 + 2000 + 20 and dict((t, u) for t, u, _ in got)[3] == 2000
    assert (ctr.table_digest(), ctr.table_stats()) == before
    tdb.close()
    ctr.close()


@pytest.mark.parametrize("k", [16, 15])
@pytest.mark.parametrize("prefix", [b"", b"A", b"T"])
def test_table_match_palindromes_and_big_counts(native, kf, k, prefix):
    # test_lookup_palindromes_and_big_counts' input: one class seen > 2^20 times
    # (its count is in the big list) and AT-repeat palindromes at even k
    from oracle import oracle
    polya = b"".join(b"@r%010d\n%s\n+\n%s\n" % (i, b"A" * 150, b"I" * 150) for i in range(9000))
    at = b"".join(b"@s%010d\n%s\n+\n%s\n" % (i, b"AT" * 75, b"I" * 150) for i in range(300))
    data = polya + at
    m = dict(oracle.count_buffer(data, prefix, k, 1))
    every = [x.decode() for x, _ in oracle.count_buffer(data, b"", k, 1)]
    rng = np.random.default_rng(k)
    a, t, pal, lap = "A" * k, "T" * k, ("AT" * k)[:k], ("TA" * k)[:k]
    db = [_template(0, [a, t, pal, lap]),
          _template(1, [a] + every[:3] + _strs(rng.integers(0, 4, (20, k), dtype=np.uint8))),
          _template(2, [t, lap] + [oracle.complement(x.encode()).decode() for x in every[:3]]),
          _template(3, [pal, pal] + _strs(rng.integers(0, 4, (20, k), dtype=np.uint8)))]
    tdb = kf.TemplateDB(db, k)
    for canonical in (False, True):
        want_map = L._canonical_from_map(m) if canonical else m
        q = {x.decode(): v for x, v in sorted(want_map.items())}
        ctr = native.Counter(k=k, prefix=prefix, flags=_flags(native, canonical))
        ctr.count_buffer(data)
        got, _, _ = _round1(kf, tdb, db, ctr, q)
        ts = {tt: s for tt, _, s in got}
        if prefix in (b"", b"A"):                          # poly-A: 136 windows per read, past the 20-bit count field
            big = 9000 * (151 - k)
            assert big > (1 << 20) - 1 and q[a] == big and ts[1] >= big and ts[0] >= big
        if k == 16 and prefix in (b"", b"A"):              # the palindrome: doubled in the Map, not in canonical mode
            full = dict(oracle.count_buffer(data, b"", k, 1))[pal.encode()]
            assert q[pal] == (full // 2 if canonical else full) and full % 2 == 0
            assert ts[3] == q[pal]
        ctr.close()
    tdb.close()


def test_table_match_states_and_lifetimes(native, kf, reads):
    import torch
    from oracle import oracle
    buf, host = reads
    k, prefix = 16, b"ATGAC"
    n1 = 317 * 12000
    m1 = L._oracle_map(host[:n1], prefix, k, False)
    second = oracle.synth_fastq(11, 0, 9000)
    m2 = L._oracle_map(second, prefix, k, False)
    rng = np.random.default_rng(77)
    # a DB over both Maps' keys
    d12 = np.concatenate([m1[0][::3], m2[0][::3]])
    db = []
    for t in range(12):
        rows = d12[rng.choice(len(d12), 250, replace=False)]
        db.append(_template(t, _strs(np.concatenate([rows, rng.integers(0, 4, (50, k), dtype=np.uint8)]))))
    tdb = kf.TemplateDB(db, k)
    q1, q2 = _query(m1, db, k), _query(m2, db, k)
    assert q1 and q2 and q1 != q2
    # kmer_db_kmers: the DB's distinct k-mers, ascending; range errors
    allk = sorted({km.encode() for t in db for km in t["kmers"]})
    dist = tdb.info()["distinct"]
    assert dist == len(allk) and tdb.kmers() == allk
    assert tdb.kmers(5, 7) == allk[5:12] and tdb.kmers(dist, 0) == [] and tdb.kmers(dist - 1) == allk[-1:]
    for first, n in ((0, dist + 1), (dist + 1, 0), (dist, 1)):
        with pytest.raises(native.KmerError) as e:
            tdb.kmers(first, n)
        assert e.value.status == 2
    # states
    ctr = native.Counter(k=k, prefix=prefix, flags=native.FLAG_UNORDERED)
    with pytest.raises(native.KmerError) as e:          # no finish yet
        kf.Match(tdb, table=ctr)
    assert e.value.status == 8
    ctr.reset()
    ctr.feed_device(buf.data_ptr(), n1)
    with pytest.raises(native.KmerError) as e:          # fed, not finished
        kf.Match(tdb, table=ctr)
    assert e.value.status == 8
    ctr.finish(want_result=False)
    ordered = native.Counter(k=k, prefix=prefix)        # an ordered-mode context has no table
    ordered.count_buffer(host[:317 * 2000])
    with pytest.raises(native.KmerError) as e:
        kf.Match(tdb, table=ordered)
    assert e.value.status == 8
    ordered.close()
    grp = native.Counter(k=k, prefix=prefix, flags=native.FLAG_UNORDERED, devices=[0, 0])
    with pytest.raises(native.KmerError) as e:          # a group context
        kf.Match(tdb, table=grp)
    assert e.value.status == 8
    grp.close()
    # k mismatch: strings of different length never compare equal
    c21 = native.Counter(k=21, prefix=b"", flags=native.FLAG_CANONICAL)
    c21.count_buffer(host[:317 * 2000])
    mk = kf.Match(tdb, table=c21)
    assert mk.templates() == [] and mk.winner().hits == 0 and mk.winner().tmpl == NONE and mk.n == dist
    mk.close()
    c21.close()
    # an empty DB
    edb = kf.TemplateDB([], k)
    me = kf.Match(edb, table=ctr)
    assert me.n == 0 and me.templates() == [] and me.winner().hits == 0 and len(me.removed()) == 0
    assert edb.kmers() == []
    me.close()
    edb.close()
    # the answers, the table untouched; two matches open on one DB
    before = (ctr.table_digest(), ctr.table_stats())
    r1 = _round1(kf, tdb, db, ctr, q1)
    ma, mb = kf.Match(tdb, table=ctr), kf.Match(tdb, table=ctr)
    assert ma.templates() == mb.templates() == r1[0]
    wa = ma.winner()
    ma.remove(wa.tmpl)                                  # a removal in one leaves the other as it was
    assert mb.templates() == r1[0] and ma.templates() != r1[0]
    assert (ctr.table_digest(), ctr.table_stats()) == before
    after_remove = (ma.templates(), ma.templates(1), ma.removed().tobytes())
    mb.close()
    # the match outlives the counter: reset, other data, close
    buf2 = torch.frombuffer(bytearray(second), dtype=torch.uint8).cuda()
    ctr.reset()
    ctr.feed_device(buf2.data_ptr(), len(second))
    ctr.finish(want_result=False)
    assert (ma.templates(), ma.templates(1), ma.removed().tobytes()) == after_remove
    r2 = _round1(kf, tdb, db, ctr, q2)                  # open / close against another table: its own answers
    assert r2 != r1
    ctr.close()
    assert (ma.templates(), ma.templates(1), ma.removed().tobytes()) == after_remove
    w2 = ma.winner()
    assert w2.hits == sum(u for _, u, _ in after_remove[0]) and w2.hits < r1[2][3]
    ma.close()
    # ... and back to the first table (the spare-buffer path again)
    ctr = L._fed(native, buf, n1, k, prefix, native.FLAG_UNORDERED)
    assert _round1(kf, tdb, db, ctr, q1) == r1
    # cross-check through the host-array open over the library's own host result
    ctr2 = native.Counter(k=k, prefix=prefix, flags=native.FLAG_UNORDERED)
    ents = ctr2.count_buffer(host[:n1]).entries()
    mh = kf.Match(tdb, [x.decode() for x, _ in ents], [v for _, v in ents])
    assert mh.templates() == r1[0] and mh.templates(1) == r1[1]
    mh.close()
    ctr2.close()
    ctr.close()
    tdb.close()
