"""GPU parity of the template DB built from FASTA genomes on the device
(kmer_db_open_fasta / kmer_db_open_fasta_device, kmer_dbfasta.hip) and of the
per-template readouts (kmer_db_template_stats / _kmers / _name).

Expected values never come from the library: a record's k-mers are the
A/C/G/T keys of oracle.count_buffer(record, prefix, k, 1, fasta=True) over
that record alone; canonical sets are derived from that Map as
tests/test_table_gpu.py::_canonical_from_map does; lengths = the sum of the
values, ulength = their number.  Every case goes through the host call, the
device call and KMER_DB_PIECE_TEST (internal pieces of 4,096 windows); all must
agree with the oracle on kmer_db_info, kmer_db_kmers, template_kmers of every
template, template_stats and the names.

Two things the configurations themselves rule out, asserted below rather than
passed over: no 8-mer that starts with ATGAC is its own reverse complement
(bases 4 and 5 would have to be complements), so the edge FASTA is also run at
k 8 / AT, where its planted ATGCGCAT counts twice; and kmer_open refuses a
canonical context whose prefix is longer than k or not A/C/G/T, so those two
prefixes of the grid run on non-canonical contexts only."""
import ctypes

import numpy as np
import pytest

from oracle import kmerfinder_oracle as ko

pytestmark = pytest.mark.gpu

FLAG_UNORDERED, FLAG_CANONICAL = 16, 64
_TR = bytes.maketrans(b"ACGT", b"TGCA")
_ACGT = frozenset(b"ACGT")
PAD = 0xC3            # around the device call's bytes: a load outside them would be a non-ASCII input


@pytest.fixture(scope="module")
def native():
    from kmerjs_amd import _native
    return _native


@pytest.fixture(scope="module")
def kf():
    from kmerjs_amd import kmerfinder
    return kmerfinder


# ---- inputs ---------------------------------------------------------------------
def _rc(s):
    return s.translate(_TR)[::-1]


def _wrap(seq, width, eol=b"\n"):
    return b"".join(seq[i:i + width] + eol for i in range(0, len(seq), width))


def _rand(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def _join(records):
    """records: [(header line or None, body)] -> (the FASTA, each record's own text, the names)."""
    texts = [(h or b"") + b for h, b in records]
    names = [(h[1:].rstrip(b"\n").removesuffix(b"\r") if h else b"") for h, _ in records]
    return b"".join(texts), texts, names


# ---- expected values --------------------------------------------------------------
_ORACLE = {}


def _maps(texts, prefix, k, canonical):
    """Per record: {key: value} of the record's own Map, A/C/G/T keys only."""
    from oracle import oracle
    out = []
    for text in texts:
        ck = (text, prefix, k)
        if ck not in _ORACLE:
            _ORACLE[ck] = {key: v for key, v in oracle.count_buffer(text, prefix, k, 1, fasta=True)
                           if _ACGT.issuperset(key)}
        m = _ORACLE[ck]
        if canonical:
            c = {}
            for key, v in m.items():
                r = _rc(key)
                if key <= r:
                    c[key] = v // 2 if key == r else v
            m = c
        out.append(m)
    return out


def _check(tdb, maps, names, what=""):
    distinct = sorted(set().union(*maps)) if maps else []
    info = tdb.info()
    assert (info["templates"], info["distinct"], info["entries"]) == \
        (len(maps), len(distinct), sum(len(m) for m in maps)), what
    assert tdb.kmers() == distinct, what
    lengths, ulengths = tdb.template_stats()
    assert lengths.tolist() == [sum(m.values()) for m in maps], what
    assert ulengths.tolist() == [len(m) for m in maps], what
    pos = {km: i for i, km in enumerate(distinct)}
    for t, m in enumerate(maps):
        assert tdb.template_kmers(t).tolist() == sorted(pos[km] for km in m), (what, t)
    assert [tdb.template_name(t) for t in range(len(maps))] == names, what
    assert [(t["lengths"], t["ulength"]) for t in tdb.templates] == \
        [(sum(m.values()), len(m)) for m in maps], what


def _device_copy(data, off):
    import torch
    t = torch.full((len(data) + off + 8,), PAD, dtype=torch.uint8, device="cuda")
    t[off:off + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def _routes(kf, native, ctr, data, offsets=(1,)):
    """(name, DB) for the host call, the device call and KMER_DB_PIECE_TEST on both."""
    yield "host", kf.TemplateDB.from_fasta(ctr, data)
    yield "host, test pieces", kf.TemplateDB.from_fasta(ctr, data, flags=native.DB_PIECE_TEST)
    if not data:
        return
    for off in offsets:
        t = _device_copy(data, off)
        yield "device + %d" % off, kf.TemplateDB.from_fasta_device(ctr, t.data_ptr() + off, len(data))
    t = _device_copy(data, offsets[-1])
    yield "device, test pieces", kf.TemplateDB.from_fasta_device(ctr, t.data_ptr() + offsets[-1], len(data),
                                                                 flags=native.DB_PIECE_TEST)


def _all_routes(kf, native, ctr, data, maps, names, offsets=(1,), what=""):
    for name, tdb in _routes(kf, native, ctr, data, offsets):
        _check(tdb, maps, names, "%s %s" % (what, name))
        tdb.close()


# ---- 1. hand-written edge FASTA ---------------------------------------------------
def _edge_records():
    return [
        (None, _wrap(b"ATGACGTACGTTAGCATGACCC", 7)),                                  # headerless first record
        (b">r1 lines of one base\n", _wrap(b"GGATGACGTTTACCATGACAAAAGTCAT", 1)),
        (b">r2 CRLF lines\r\n", _wrap(b"ATGACGTACGTTAGCATGACCCGGTCATAA", 7, b"\r\n")),
        (b">r3 a blank line inside\n", b"ATGACGT\n\nACGTTAG\n\n"),
        (b">r4 N and lowercase runs\n", _wrap(b"ATGACGTNNATGACatgacgtaATGACGGTTNATGACGGTCATCGTCAT", 7)),
        (b">r5 empty\n", b""),
        (b">r6 one base\n", b"A\n"),
        (b">r7 k - 1 bases\n", b"ATGACGT\n"),
        (b">r8 exactly k bases\n", b"ATGACGTA\n"),
        (b">r9 self-complementary ATGCGCAT\n", _wrap(b"CCATGCGCATGGATGACTTTT", 7)),
        (b">r10 shares k-mers with r8 and r0\n", _wrap(b"TTATGACGTATTATGACGTACGTT", 7)),
        (b">r11 a k-mer twice\n", _wrap(b"ATGACGTACGGATGACGTACTT", 7)),
        (b">\n", b"ATGACTTTTGG\n"),                                                  # a header without a name
        (b">r13 no trailing newline\n", b"ATGACCCGGTCAT"),
    ]


@pytest.mark.parametrize("flags", [0, FLAG_UNORDERED, FLAG_CANONICAL], ids=["ordered", "unordered", "canonical"])
@pytest.mark.parametrize("prefix", [b"ATGAC", b"AT"])
def test_edge_fasta(kf, native, flags, prefix):
    k = 8
    data, texts, names = _join(_edge_records())
    canonical = bool(flags & FLAG_CANONICAL)
    maps = _maps(texts, prefix, k, canonical)
    # the cases are what they claim to be (by the oracle)
    assert maps[5] == {} and maps[6] == {} and maps[7] == {}
    if prefix == b"ATGAC":
        assert maps[8] == {b"ATGACGTA": 1}
        assert not any(km == _rc(km) for m in maps for km in m)                  # (no such 8-mer exists)
    else:
        assert maps[9][b"ATGCGCAT"] == (1 if canonical else 2)                    # counted for both strands
    assert set(maps[8]) & set(maps[10]) and set(maps[0]) & set(maps[10])          # shared between records
    assert sum(maps[11].values()) > len(maps[11])                                 # repeated inside one record
    ctr = native.Counter(k=k, prefix=prefix, flags=flags)
    try:
        _all_routes(kf, native, ctr, data, maps, names, offsets=(0, 1, 2, 3))
        # an unterminated last header: a last record without a sequence
        data2, texts2, names2 = _join(_edge_records()[:4] + [(b">last header, no newline", b"")])
        assert names2[-1] == b"last header, no newline"
        _all_routes(kf, native, ctr, data2, _maps(texts2, prefix, k, canonical), names2, what="open header")
        # ... and one that ends with '\r'
        data3, texts3, _ = _join(_edge_records()[:2] + [(b">cr at the end\r", b"")])
        _all_routes(kf, native, ctr, data3, _maps(texts3, prefix, k, canonical), [b"", names[1], b"cr at the end"],
                    what="open header, CR")
    finally:
        ctr.close()


# ---- 2. grid ------------------------------------------------------------------------
def _grid_records(seed):
    rng = np.random.default_rng(seed)
    recs = []
    for r in range(40):
        n = int(rng.integers(0, 601)) if r % 9 else int(rng.integers(0, 3))
        seq = bytearray(_rand(rng, n))
        if r % 5 == 0 and n > 40:
            for p in rng.integers(0, n, 3):
                seq[p] = rng.choice(list(b"NnXa"))
        if r % 4 == 1 and n > 64:                          # a repeat and a reverse-complement repeat inside the record
            seq[n - 32:n] = seq[:32]
            seq[n // 2:n // 2 + 24] = _rc(bytes(seq[:24]))
        width = (1, 7, 60, 61)[r % 4]
        eol = b"\r\n" if r % 7 == 3 else b"\n"
        recs.append((b">g%d sp %d" % (r, r * r) + eol, _wrap(bytes(seq), width, eol)))
    return recs


@pytest.mark.parametrize("canonical", [False, True], ids=["map", "canonical"])
@pytest.mark.parametrize("k", [1, 2, 5, 16, 21, 31, 32])
def test_grid(kf, native, k, canonical):
    data, texts, names = _join(_grid_records(k))
    # a prefix of length k that occurs: a window of the longest record
    seq = max((b"".join(tx.replace(b"\r", b"").split(b"\n")[1:]) for tx in texts), key=len)
    whole = next(seq[i:i + k] for i in range(100, len(seq)) if _ACGT.issuperset(seq[i:i + k]))
    for prefix in (b"", b"A", b"ATGAC", whole, b"ATGAC" * 7, b"ATNAC"):
        if prefix == b"ATGAC" * 7:
            prefix = prefix[:k + 1]                        # one longer than k
        if prefix == b"ATGAC" and k < 5:
            prefix = prefix[:k]
        flags = FLAG_CANONICAL if canonical else (FLAG_UNORDERED if k % 2 else 0)
        if canonical and (len(prefix) > k or not _ACGT.issuperset(prefix)):
            with pytest.raises(native.KmerError) as e:     # (no such canonical context exists)
                native.Counter(k=k, prefix=prefix, flags=flags)
            assert e.value.status == 2
            continue
        maps = _maps(texts, prefix, k, canonical)
        if len(prefix) > k or not _ACGT.issuperset(prefix):
            assert not any(maps)                           # a valid DB whose templates all have ulength 0
        elif not canonical:
            assert any(maps)
        ctr = native.Counter(k=k, prefix=prefix, flags=flags)
        try:
            _all_routes(kf, native, ctr, data, maps, names, what="prefix %r" % prefix)
        finally:
            ctr.close()


# ---- 3. boundaries --------------------------------------------------------------------
def _boundary_records():
    rng = np.random.default_rng(3)
    n = 70_000
    seq = bytearray(_rand(rng, n))
    motif = b"ATGAC" + _rand(rng, 43)
    for j in range(1, n // 4096 + 1):                      # windows that straddle every 4,096-window boundary
        seq[4096 * j - 8:4096 * j + 40] = motif            # (record 0 has no window at k 16 and 21: window p starts at byte p)
        seq[4096 * j - 300:4096 * j - 252] = _rc(motif)
    return [(b">tiny three bases\n", b"ACG\n"), (b">big 70 kb\n", _wrap(bytes(seq), 60)),
            (b">after\n", _wrap(_rand(rng, 500), 60))]


@pytest.mark.parametrize("k,prefix,flags", [(21, b"", FLAG_UNORDERED), (16, b"ATGAC", 0)], ids=["k21", "k16-ATGAC"])
def test_boundaries(kf, native, k, prefix, flags):
    data, texts, names = _join(_boundary_records())
    maps = _maps(texts, prefix, k, False)
    assert sum(maps[1].values()) > len(maps[1]) > 0 and maps[0] == {}
    ctr = native.Counter(k=k, prefix=prefix, flags=flags)
    try:
        _all_routes(kf, native, ctr, data, maps, names, offsets=(0, 1, 2, 3))
    finally:
        ctr.close()


# ---- 4. host pieces -----------------------------------------------------------------------
def test_host_pieces(kf, native):
    rng = np.random.default_rng(4)
    recs = []
    for r in range(61):
        n = 20_000 if r == 37 else int(rng.integers(1000, 3001))
        recs.append((b">p%d piece test\n" % r, _wrap(_rand(rng, n), 70)))
    data, texts, names = _join(recs)
    maps = _maps(texts, b"ATGAC", 16, False)
    small = native.Counter(k=16, prefix=b"ATGAC", batch_bytes=4096)
    whole = native.Counter(k=16, prefix=b"ATGAC")
    try:
        a = kf.TemplateDB.from_fasta(small, data)
        b = kf.TemplateDB.from_fasta(whole, data)
        _check(a, maps, names, "pieces of 4 KiB")
        _check(b, maps, names, "one piece")
        assert a.kmers() == b.kmers() and [t for t in a.templates] == [t for t in b.templates]
        assert [t["sequence"] for t in a.templates] == ["p%d" % r for r in range(61)]
        assert all(t["species"] == "piece test" for t in a.templates)
        a.close(), b.close()
    finally:
        small.close(), whole.close()


# ---- 5. the same DB as the existing route ------------------------------------------------------
def _genomes(seed, n, length, related=()):
    rng = np.random.default_rng(seed)
    seqs = [_rand(rng, length) for _ in range(n)]
    for a, b in related:                                   # b shares a third of a
        seqs[b] = seqs[a][:length // 3] + seqs[b][length // 3:]
    return seqs


def _fastq(rng, seqs, picks, rlen=150):
    out = []
    for t, n in picks:
        for i in range(n):
            p = int(rng.integers(0, len(seqs[t]) - rlen))
            out.append(b"@r%d_%d\n" % (t, i) + seqs[t][p:p + rlen] + b"\n+\n" + b"I" * rlen + b"\n")
    return b"".join(out)


def _templates(names, maps):
    out = []
    for name, m in zip(names, maps):
        parts = name.decode("latin-1").split(None, 1)
        out.append({"sequence": parts[0], "species": parts[1] if len(parts) > 1 else "",
                    "lengths": sum(m.values()), "ulength": len(m), "kmers": [km.decode("latin-1") for km in m]})
    return out


def _trace(m):
    """Everything a winner loop sees: both orders, every winner, the hits after every remove."""
    out = [m.templates(0), m.templates(1)]
    for _ in range(1000):
        w = m.winner()
        out.append((w.tmpl, w.uscore, w.tscore, w.hits, w.first_uscore, w.first_tscore))
        if w.hits == 0:
            return out
        out.append(m.remove(w.tmpl))
        out.append(m.templates(1))
    raise AssertionError("the winner loop did not end")


def test_same_db_as_the_kmer_list_route(kf, native):
    from oracle import oracle
    k, prefix = 16, b"AT"
    seqs = _genomes(5, 12, 4000, related=[(2, 7), (2, 9), (4, 5)])
    data, texts, names = _join([(b">t%d genus species %d\n" % (i, i), _wrap(s, 60)) for i, s in enumerate(seqs)])
    maps = _maps(texts, prefix, k, False)
    old = kf.TemplateDB(_templates(names, maps), k)
    fq = _fastq(np.random.default_rng(6), seqs, [(2, 60), (4, 30), (7, 10), (11, 5)])
    ctr = native.Counter(k=k, prefix=prefix, flags=FLAG_UNORDERED)
    try:
        new = kf.TemplateDB.from_fasta(ctr, data)
        assert new.info() == old.info() and new.kmers() == old.kmers()
        assert [{**t, "kmers": None} for t in old.templates] == [{**t, "kmers": None} for t in new.templates]
        assert new.summary == old.summary
        q = oracle.count_buffer(fq, prefix, k, 1)
        keys, counts = [key for key, _ in q], [v for _, v in q]
        traces = []
        for db in (old, new):
            m = kf.Match(db, keys, counts)
            traces.append(_trace(m))
            m.close()
        assert traces[0] == traces[1] and len(traces[0]) > 8 and traces[0][2][3] > 0
        ctr.count_buffer(fq)                                               # the table-mode count as the query
        traces = []
        for db in (old, new):
            m = kf.Match(db, table=ctr)
            traces.append(_trace(m))
            m.close()
        assert traces[0] == traces[1] and len(traces[0]) > 8 and traces[0][2][3] > 0
        old.close(), new.close()
    finally:
        ctr.close()


# ---- 6. end to end ---------------------------------------------------------------------------------
def test_end_to_end_reads_find_their_genome(kf, native):
    from oracle import oracle
    k, prefix = 16, b"A"
    seqs = _genomes(8, 8, 5000)
    data, texts, names = _join([(b">NC_%06d Genus species strain %d\n" % (i, i), _wrap(s, 60))
                                for i, s in enumerate(seqs)])
    fq = _fastq(np.random.default_rng(9), seqs, [(3, 200), (6, 40)] + [(t, 1) for t in range(8)])
    tpl = _templates(names, _maps(texts, prefix, k, False))
    summary = {"templates": len(tpl), "totalLen": sum(t["lengths"] for t in tpl),
               "uniqueLens": sum(t["ulength"] for t in tpl)}
    qo = {key.decode("latin-1"): v for key, v in oracle.count_buffer(fq, prefix, k, 1)}
    want = ko.winner_scoring(dict(qo), tpl, summary, len(qo))
    ctr = native.Counter(k=k, prefix=prefix)
    try:
        db = kf.TemplateDB.from_fasta(ctr, data)
        assert db.summary == summary
        q = {key.decode("latin-1"): v for key, v in ctr.count_buffer(fq).entries()}
        assert q == qo
        got = kf.KmerFinder(db).find_matches(q)
        assert got == want
        assert len(want) == 2                              # (ended by an insignificant third winner, not by NoHits)
        assert got[0][0] == ("template", "NC_000003") and got[0][-1] == ("species", "Genus species strain 3")
        db.close()
    finally:
        ctr.close()


# ---- 7. state and errors ----------------------------------------------------------------------------
def _status(native, f):
    with pytest.raises(native.KmerError) as e:
        f()
    return e.value.status


def test_state_and_parameter_errors(kf, native):
    import torch
    from kmerjs_amd import synth_fastq_device
    data, texts, names = _join(_edge_records())
    maps = _maps(texts, b"ATGAC", 8, False)
    grp = native.Counter(k=8, prefix=b"ATGAC", devices=[0, 0])
    assert _status(native, lambda: kf.TemplateDB.from_fasta(grp, data)) == 8
    grp.close()
    for kw in ({"k": 33}, {"k": 16, "step": 2}):
        c = native.Counter(prefix=b"ATGAC", **kw)
        assert _status(native, lambda: kf.TemplateDB.from_fasta(c, data)) == 2
        t = _device_copy(data, 0)
        assert _status(native, lambda: kf.TemplateDB.from_fasta_device(c, t.data_ptr(), len(data))) == 2
        c.close()
    ctr = native.Counter(k=8, prefix=b"ATGAC")
    try:
        buf = torch.empty(200 * 317, dtype=torch.uint8, device="cuda")
        synth_fastq_device(buf.data_ptr(), 2, 0, 200)
        torch.cuda.synchronize()
        ctr.reset()
        db = kf.TemplateDB.from_fasta(ctr, data)           # a session without a chunk yet: allowed
        _check(db, maps, names, "after a reset")
        db.close()
        ctr.feed_device(buf.data_ptr(), 200 * 317)
        assert _status(native, lambda: kf.TemplateDB.from_fasta(ctr, data)) == 8      # fed, not finished
        n_keys = len(ctr.finish())
        bad = data[:40] + b"\xc3" + data[40:]
        assert _status(native, lambda: kf.TemplateDB.from_fasta(ctr, bad)) == 6
        t = _device_copy(bad, 1)
        assert _status(native, lambda: kf.TemplateDB.from_fasta_device(ctr, t.data_ptr() + 1, len(bad))) == 6
        db = kf.TemplateDB.from_fasta(ctr, data)           # the same context afterwards
        _check(db, maps, names, "after a non-ASCII input")
        assert ctr.result_device()[3] == n_keys            # the finished result is still the context's
        db.close()
    finally:
        ctr.close()


def test_empty_input_gives_an_empty_db(kf, native):
    ctr = native.Counter(k=16, prefix=b"ATGAC")
    try:
        for db in (kf.TemplateDB.from_fasta(ctr, b""), kf.TemplateDB.from_fasta_device(ctr, 0, 0)):
            assert db.info() == {"k": 16, "templates": 0, "distinct": 0, "entries": 0}
            assert db.templates == [] and db.kmers() == []
            m = kf.Match(db, ["ATGACGTACGTTAGCA"], [3])
            assert m.winner().hits == 0 and m.templates(0) == [] and m.templates(1) == []
            m.close()
            db.close()
    finally:
        ctr.close()


def test_db_between_table_reads_leaves_the_table_alone(kf, native):
    from oracle import oracle
    fq = oracle.synth_fastq(5, 0, 300)
    data, texts, names = _join(_grid_records(16))
    maps = _maps(texts, b"ATGAC", 16, False)
    ctr = native.Counter(k=16, prefix=b"ATGAC", flags=FLAG_UNORDERED)
    try:
        res = ctr.count_buffer(fq)
        keys = b"".join(res.keys()[:50]) + b"ATGACAAAAAAAAAAA"
        before = (ctr.table_stats(), ctr.table_digest(), ctr.table_lookup(keys).tolist(),
                  ctr.table_screen(fq[:317 * 20]).tolist(), ctr.lines())
        db = kf.TemplateDB.from_fasta(ctr, data)
        after = (ctr.table_stats(), ctr.table_digest(), ctr.table_lookup(keys).tolist(),
                 ctr.table_screen(fq[:317 * 20]).tolist(), ctr.lines())
        assert before == after and sum(before[2]) > 0
        _check(db, maps, names)
        ctr.close()                                        # the DB outlives the context
        _check(db, maps, names, "after the context's close")
        t = next(t for t, m in enumerate(maps) if len(m) >= 3)
        n = len(maps[t])
        assert db.template_kmers(t, cap=2).tolist() == db.template_kmers(t).tolist()[:2]
        idx = (ctypes.c_uint32 * 4)(7, 7, 7, 7)
        got = ctypes.c_uint64()
        assert native.LIB.kmer_db_template_kmers(db.handle, t, 2, idx, ctypes.byref(got)) == 0
        assert got.value == n and list(idx)[2:] == [7, 7] and list(idx)[:2] == db.template_kmers(t).tolist()[:2]
        db.close()
    finally:
        ctr.close()


def test_readouts_on_a_kmer_list_db(kf):
    tpl = [{"sequence": "a", "species": "s", "lengths": 9, "ulength": 2, "kmers": ["ATGACGTA", "ATGACGTA", "CCGTACGT"]},
           {"sequence": "b", "species": "s", "lengths": 9, "ulength": 0, "kmers": []},
           {"sequence": "c", "species": "s", "lengths": 9, "ulength": 1, "kmers": ["ATGACGTA"]}]
    db = kf.TemplateDB(tpl, 8)
    lengths, ulengths = db.template_stats()
    assert lengths.tolist() == [3, 0, 1] and ulengths.tolist() == [2, 0, 1]      # keys passed / entries after dedup
    assert db.kmers() == [b"ATGACGTA", b"CCGTACGT"]
    assert [db.template_kmers(t).tolist() for t in range(3)] == [[0, 1], [], [0]]
    assert [db.template_name(t) for t in range(3)] == [b"", b"", b""]
    db.close()
