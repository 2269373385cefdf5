"""The plane scan's candidate -> hit-record pass (scan_planes_kernel): the
fixed k = 16 / ATGAC instantiation and the run-time ones, bytes that alias on
the planes, window and line-start positions, and candidate densities that take
the queue's other routes.  Every case is a few tiles (TILE = 16384 bytes) of
seeded text, and every result equals the oracle's entry for entry, in order.

`scan_model` restates what the kernel sees per tile (plane candidates, queue
entries, verified hits, where each hit's line starts), so that a CPU test can
check that each case holds what it is about."""
import functools

import numpy as np
import pytest

from tests.util import first_diff

TILE = 16384
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rc(s):
    return s.translate(COMP)[::-1]


def _acgt(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def _mix(rng, pieces, n):
    """n bytes drawn piece by piece."""
    out = b""
    while len(out) < n:
        out += pieces[int(rng.integers(0, len(pieces)))]
    return out[:n]


def _plant(rng, seq, pieces, at=None):
    """seq with each piece written over it, at random places (or at `at`)."""
    seq = bytearray(seq)
    for i, p in enumerate(pieces):
        o = at[i] if at is not None else int(rng.integers(0, len(seq) - len(p) + 1))
        seq[o:o + len(p)] = p
    return bytes(seq)


class Text:
    """A FASTQ text built read by read; the header is padded so that a
    sequence line starts where a case needs it."""

    def __init__(self):
        self.b = bytearray()
        self.n = 0

    def read(self, seq, qual=None, seq_at=None):
        name = b"@r%d" % self.n
        self.n += 1
        if seq_at is not None:
            pad = seq_at - (len(self.b) + len(name) + 1)
            assert pad >= 0, "sequence start already passed"
            name += b"x" * pad
        self.b += name + b"\n"
        assert seq_at is None or len(self.b) == seq_at
        self.b += seq + b"\n+\n" + (qual if qual is not None else b"I" * len(seq)) + b"\n"
        return self

    def fill(self, rng, upto, pieces=()):
        """150-base reads, each with `pieces` planted, until `upto` bytes."""
        while len(self.b) < upto:
            self.read(_plant(rng, _acgt(rng, 150), pieces))
        return self

    def bytes(self, cut=None):
        return bytes(self.b if cut is None else self.b[:cut])


# ---------------------------------------------------------------------------
# what the kernel sees
# ---------------------------------------------------------------------------
def scan_model(data, prefix, k):
    """Per tile t (candidates belong to the tile of their prefix match at q):
    cand[s], entries, hits[s] for strand s, far[s] = set of line-start classes
    of the verified hits, plus the candidates dropped for an aliasing byte
    (`alias[s]`) or for a prefix byte past the fifth (`late[s]`)."""
    plen, pb = len(prefix), min(len(prefix), 5)
    a = np.frombuffer(data + b"\n" * 96, dtype=np.uint8)
    n = len(data)
    code = (a >> 1) & 3
    nl = np.flatnonzero(a[:n] == 10)
    tiles = {}
    for s, pat in enumerate((prefix, rc(prefix))):
        p = np.frombuffer(pat, dtype=np.uint8)
        cand = np.ones(n, bool)
        exact5 = np.ones(n, bool)
        exact = np.ones(n, bool)
        for i in range(plen):
            if i < pb:
                cand &= code[i:n + i] == ((p[i] >> 1) & 3)
                exact5 &= a[i:n + i] == p[i]
            exact &= a[i:n + i] == p[i]
        for q in np.flatnonzero(cand):
            q = int(q)
            t = tiles.setdefault(q // TILE, {"cand": [0, 0], "ent": set(), "hits": [0, 0], "far": [set(), set()],
                                             "alias": [0, 0], "late": [0, 0], "halo": [set(), set()]})
            t["cand"][s] += 1
            t["ent"].add(((q % TILE) // 32, s))
            s0 = q + plen - k if s else q
            if not exact5[q]:
                t["alias"][s] += 1
                continue
            if not exact[q]:
                t["late"][s] += 1
                continue
            if s0 < 0 or s0 + k > n or (a[s0:s0 + k] == 10).any():
                continue
            t["hits"][s] += 1
            r0 = s0 - (q // TILE) * TILE            # window start, tile-relative
            if r0 < 0:
                t["halo"][s].add("front")
            if r0 + k > TILE:
                t["halo"][s].add("back")
            i = int(np.searchsorted(nl, s0)) - 1   # last '\n' before s0
            ls = int(nl[i]) - (q // TILE) * TILE if i >= 0 else -1
            if r0 <= 0:
                continue
            if ls < 0:
                t["far"][s].add("none")
            else:
                d = (r0 - 1) // 64 - ls // 64
                t["far"][s].add("chunk" if (r0 - 1) // 16 == ls // 16 else "region" if d == 0 else
                                "previous" if d == 1 else "beyond64" if d > 64 else "beyond32" if d > 32 else "near")
    return tiles


def both(x):
    return x[0] > 0 and x[1] > 0


# ---------------------------------------------------------------------------
# cases: name -> (data, k, prefix, check(model, oracle entries))
# ---------------------------------------------------------------------------
LONG7, LONG8 = b"ATGACGT", b"ATGACGTA"


def _inst_text():
    """Motif-rich FASTQ over three tiles: the prefixes of every instantiation
    case, their reverse complements, and near-misses of the long prefixes in
    base 6 or 7."""
    rng = np.random.default_rng(411)
    near = [b"ATGACCT", b"ATGACGA", b"ATGACCTA", b"ATGACGAA", b"ATGACGTC"]
    pieces = [b"ATGAC", b"GTCAT", b"ATGA", b"TCAT", b"CTGAC", b"GTCAG", LONG7, rc(LONG7), LONG8, rc(LONG8)]
    pieces += near + [rc(x) for x in near] + [b"A", b"C", b"G", b"T", b"AC", b"GT", b"TA", b"CG"]
    t = Text()
    while len(t.b) < 3 * TILE + 200:
        t.read(_mix(rng, pieces, 150), qual=_mix(rng, [b"I", b"F", b"ATGAC", b"GTCAT", b"5", b"#"], 150))
    return t.bytes(3 * TILE + 150)


INST = [(16, b"ATGAC"), (15, b"ATGAC"), (17, b"ATGAC"), (32, b"ATGAC"), (16, b"ATGA"), (16, b"CTGAC"),
        (16, LONG7), (20, LONG8)]


def _chk_inst(k, prefix):
    def chk(m, want):
        assert all(both(m[t]["hits"]) for t in (0, 1, 2))
        if len(prefix) > 5:
            assert both([sum(t["late"][s] for t in m.values()) for s in (0, 1)]), "no near-miss past base 5"
    return chk


def _same_planes(b, rng):
    """A printable byte other than b that the planes cannot tell from it."""
    c = [x for x in range(33, 127) if (x >> 1) & 3 == (b >> 1) & 3 and x != b]
    return c[int(rng.integers(0, len(c)))]


def _alias_text():
    rng = np.random.default_rng(412)
    named = [b"atgac", b"gtcat", b"ATNAC", b"@TGAC", b"ADGAC", b"ATFAC", b"ATGAB",
             b"ftcat", b"GTKAT", b"GDCAT", b"GTCQT", b"GTC@T", b"GTCAD", b"FTCAT"]
    for x in named:                          # each aliases one of the two motifs, byte for byte
        assert any(x != mo and all((p >> 1) & 3 == (y >> 1) & 3 for p, y in zip(mo, x)) for mo in (b"ATGAC", b"GTCAT")), x
    keep = [b"ATGACGTNACGTACGT", b"ATGACgtacgtacgta", b"ATGACGTACGTACGTn",      # exact prefix, exotic suffix
            b"NCGTACGTACGGTCAT", b"acgtacgtacgGTCAT", b"ACGTACGTACNGTCAT"]      # ... and the mirror image
    t = Text()
    r = 0
    while len(t.b) < 2 * TILE + 300:
        ps = [named[(r + j) % len(named)] for j in range(3)] + [keep[r % len(keep)]]
        for motif in (b"ATGAC", b"GTCAT"):                                     # one random aliasing byte each
            x = bytearray(motif)
            i = int(rng.integers(0, 5))
            x[i] = _same_planes(x[i], rng)
            ps.append(bytes(x))
        at = [8 + 24 * j for j in range(len(ps))]                              # (apart: no piece overwrites another)
        seq = _plant(rng, _acgt(rng, 160), ps, at)
        qual = _plant(rng, bytes(rng.integers(33, 127, 160, dtype=np.uint8)), ps[:3] + [(b"ATGAC", b"GTCAT")[r % 2]] + ps[4:],
                      at)
        if r % 3 == 0:
            seq = seq[:-4] + b"ATGA"         # ATGA\n: the line end aliases C
            qual = qual[:-2] + b"GT"         # GT\n@r: '\n' aliases C, '@' aliases A (four of GTCAT's five)
        if r % 3 == 1:
            seq = seq[:-2] + b"GT"           # GT\n+\n: no candidate ('+' aliases C), a window across the line end
            qual = qual[:-4] + b"ATGA"
        t.read(seq, qual=qual)
        r += 1
    return t.bytes()


def _chk_alias(m, want):
    assert all(t["alias"][s] >= 20 for t in list(m.values())[:2] for s in (0, 1)), "too few aliasing candidates"
    exo = [key for key, _ in want if set(key) - set(b"ACGT")]
    assert sum(b"N" in key or b"n" in key for key in exo) >= 4 and any(key[5:].islower() for key in exo)
    assert all(key.startswith(b"ATGAC") for key, _ in want)


def _pos_front_halo():
    """Tile 1 begins in mid-line with GTCAT inside its first 11 bytes (the
    window starts in the front halo); ATGAC 8 bytes before the end of tile 1
    (the window ends in the back halo); a sequence line begins at byte 0 of
    tile 3."""
    rng = np.random.default_rng(413)
    t = Text().fill(rng, TILE - 700, [b"ATGAC"])
    t.read(_plant(rng, _acgt(rng, 150), [b"GTCAT", b"GTCAT", b"ATGAC"], [63, 69, 80]), seq_at=TILE - 60)
    t.fill(rng, 2 * TILE - 700, [b"GTCAT"])
    t.read(_plant(rng, _acgt(rng, 150), [b"ATGAC", b"GTCAT", b"ATGAC"], [92, 98, 103]), seq_at=2 * TILE - 100)
    t.fill(rng, 3 * TILE - 700, [b"ATGAC"])
    t.read(_plant(rng, _acgt(rng, 150), [b"ATGAC", b"GTCAT"], [0, 11]), seq_at=3 * TILE)
    t.fill(rng, 3 * TILE + 900, [b"GTCAT", b"ATGAC"])
    return t.bytes()


def _chk_front_halo(m, want):
    assert "front" in m[1]["halo"][1] and "back" in m[1]["halo"][0]
    assert m[3]["hits"][0] and m[3]["hits"][1]


def _pos_line_starts():
    """Hits whose line begins in the same 16-byte chunk, the same 64-byte
    region, the region before, and more than 32 / more than 64 regions back
    (a 6000-base read: whole bitmap words without a line end)."""
    rng = np.random.default_rng(414)
    t = Text()
    long_seq = bytearray(_acgt(rng, 6000))
    for o in range(40, 5980, 97):
        long_seq[o:o + 5] = (b"ATGAC", b"GTCAT")[(o // 97) % 2]
    t.read(bytes(long_seq))
    for i in range(40):
        at = [(i * 7) % 11, 17 + (i * 5) % 30, 60 + (i * 3) % 40, 110 + i % 20]
        t.read(_plant(rng, _acgt(rng, 150), [b"ATGAC", b"GTCAT", b"ATGAC", b"GTCAT"][i % 2:] +
                      [b"ATGAC", b"GTCAT"][:i % 2], at))
    t.fill(rng, len(t.b) + 1500, [b"ATGAC", b"GTCAT"])
    return t.bytes()


def _chk_line_starts(m, want):
    for s in (0, 1):
        seen = set().union(*(t["far"][s] for t in m.values()))
        assert {"chunk", "region", "previous", "beyond32", "beyond64"} <= seen, (s, seen)


def _pos_no_newline_tile():
    """A 34000-base read: tile 1 lies inside the line and holds no '\\n'."""
    rng = np.random.default_rng(415)
    t = Text().fill(rng, 3000, [b"ATGAC", b"GTCAT"])
    seq = bytearray(_acgt(rng, 34000))
    for o in range(10, 33980, 211):
        seq[o:o + 5] = (b"ATGAC", b"GTCAT")[(o // 211) % 2]
    t.read(bytes(seq))
    return t.bytes()


def _chk_no_newline_tile(m, want):
    assert m[1]["far"][0] == {"none"} and m[1]["far"][1] == {"none"} and both(m[1]["hits"])


def _pos_last_line():
    """The input ends inside a sequence line, right after a window."""
    rng = np.random.default_rng(416)
    t = Text().fill(rng, TILE + 500, [b"ATGAC"])
    t.read(_plant(rng, _acgt(rng, 150), [b"GTCAT", b"ATGAC"], [100, 110]))
    seq_start = len(t.b) - (150 + 3 + 150 + 1)
    data = t.bytes(seq_start + 110 + 16)
    assert data[-16:-11] == b"ATGAC" and data[-26:-21] == b"GTCAT" and b"\n" not in data[-126:]
    return data


def _chk_last_line(m, want):
    assert both(m[max(m)]["hits"])


def _dense(seed, exact, alias, upto=TILE - 200):
    """One tile of reads with `exact` exact and `alias` aliasing motifs each
    (alternating strands), at least 32 bytes apart: one queue entry each."""
    rng = np.random.default_rng(seed)
    t = Text()
    r = 0
    while len(t.b) < upto - 320:
        ps = [(b"ATGAC", b"GTCAT")[(r + j) % 2] for j in range(exact)] + \
             [(b"ATNAC", b"GTCQT")[(r + j) % 2] for j in range(alias)]
        seq = bytearray(b"A" * 150)          # (poly-A between the motifs: no chance candidates)
        for j, p in enumerate(ps):
            o = 14 + 33 * j
            seq[o:o + 5] = p
        t.read(bytes(seq))
        r += 1
    return t.bytes()


def _chk_dense(ent, hits):
    def chk(m, want):
        t = m[0]
        assert ent[0] < len(t["ent"]) <= ent[1], len(t["ent"])
        assert hits[0] < sum(t["hits"]) <= hits[1] and both(t["hits"]), t["hits"]
    return chk


@functools.lru_cache(maxsize=None)
def cases():
    inst = _inst_text()
    out = {"inst-%d-%s" % (k, p.decode()): (inst, k, p, _chk_inst(k, p)) for k, p in INST}
    out["alias"] = (_alias_text(), 16, b"ATGAC", _chk_alias)
    out["pos-halo"] = (_pos_front_halo(), 16, b"ATGAC", _chk_front_halo)
    out["pos-line-starts"] = (_pos_line_starts(), 16, b"ATGAC", _chk_line_starts)
    out["pos-no-newline-tile"] = (_pos_no_newline_tile(), 16, b"ATGAC", _chk_no_newline_tile)
    out["pos-last-line"] = (_pos_last_line(), 16, b"ATGAC", _chk_last_line)
    # more than 64 candidates (second wave of the drain, final barrier), at most 64 hits
    out["dense-cand65"] = (_dense(417, 1, 1), 16, b"ATGAC", _chk_dense((64, 128), (0, 64)))
    # more than 128 queue entries: the queue is drained in rounds
    out["dense-queue-rounds"] = (_dense(418, 2, 2), 16, b"ATGAC", _chk_dense((128, 1024), (64, 9999)))
    # more than 64 verified hits: the overflow list
    out["dense-hits65"] = (_dense(419, 2, 0), 16, b"ATGAC", _chk_dense((64, 128), (64, 9999)))
    return out


NAMES = ["inst-%d-%s" % (k, p.decode()) for k, p in INST] + [
    "alias", "pos-halo", "pos-line-starts", "pos-no-newline-tile", "pos-last-line",
    "dense-cand65", "dense-queue-rounds", "dense-hits65"]


@functools.lru_cache(maxsize=None)
def expected(name):
    from oracle import oracle
    data, k, prefix, _ = cases()[name]
    return oracle.count_buffer(data, prefix, k, 1)


@pytest.mark.parametrize("name", NAMES)
def test_case_holds_what_it_is_about(name):
    data, k, prefix, check = cases()[name]
    assert len(data) <= 5 * TILE
    want = expected(name)
    assert want, "empty oracle result"
    check(scan_model(data, prefix, k), want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_hit_pass_vs_oracle(name):
    from kmerjs_amd import _native
    data, k, prefix, _ = cases()[name]
    want = expected(name)
    ctr = _native.Counter(k=k, prefix=prefix)
    got = ctr.count_buffer(data).entries()
    ctr.close()
    assert len(got) == len(want), name
    assert first_diff(got, want) is None, name
