"""The plane scan's line context, carried with the candidate from the thread
that found it: hand-made inputs of a few 16 KiB tiles that put '\\n' bytes,
line starts and hits of both strands at the edges of the 64-byte thread
regions, of the waves (4 KiB) and of the tile.  Every case compares the whole
ordered result (keys, counts, first-occurrence order, line count) with the
oracle on the same bytes, three times on one context; a test without the GPU
mark checks that the oracle's result of every case is non-empty."""
import functools

import numpy as np
import pytest

from tests.util import first_diff

TILE = 16384
REGION = 64                # bytes per thread of the scan
WAVE = 64 * REGION
FLAG_LONG_LINES = 128      # KMER_FLAG_LONG_LINES (kmer_api.h)
FWD, REV = b"ATGACA", b"TGTCAT"   # ATGA / ATGAC / ATGACA, and the reverse complements behind a T
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


class Build:
    """A FASTQ text built record by record, with the bytes that matter at
    chosen offsets.  Motif positions of a sequence line are line-relative; a
    reverse motif is given by the position of its GTCAT."""

    def __init__(self, seed, eol=b"\n"):
        self.b = bytearray()
        self.rng = np.random.default_rng(seed)
        self.eol = eol

    def bases(self, n, fwd=(), rev=(), raw=()):
        s = bytearray(ACGT[self.rng.integers(0, 4, n)].tobytes())
        for p in fwd:
            s[p:p + 6] = FWD[:max(0, min(6, n - p))]
        for p in rev:
            if p >= 1:
                s[p - 1:p + 5] = REV
            else:
                s[p:p + 5] = REV[1:]
        for p, x in raw:
            s[p:p + len(x)] = x
        assert len(s) == n
        return bytes(s)

    def record(self, seq, header_len=8):
        """header of header_len bytes (without its line end), the sequence line, '+', quality"""
        assert header_len >= 1
        e = self.eol
        self.b += b"@" + b"h" * (header_len - 1) + e + seq + e + b"+" + e + b"I" * len(seq) + e

    def filler(self, n=100):
        """An ordinary read: hits of both strands inside the line, at its start
        and at its end, and motifs whose window would cross a line end (a
        GTCAT in the first 11 bases, an ATGAC in the last 15): no hit."""
        self.record(self.bases(n, fwd=(0, 30, n - 16), rev=(6, 11, 50), raw=((n - 10, b"ATGACGTCAT"),)))

    def fill_to(self, off, slack=320):
        while off - len(self.b) > slack:
            self.filler()

    def line_at(self, start, seq):
        """a record whose sequence line starts at byte `start` (its header's '\\n' at start - 1)"""
        self.fill_to(start - len(self.eol), 330)
        hl = start - len(self.eol) - len(self.b)
        assert hl >= 1, (start, len(self.b))
        self.record(seq, hl)
        assert self.b[start - 1] == 10 and self.b[start:start + len(seq)] == seq

    def line_ending_at(self, off, seq):
        """a record whose sequence line's '\\n' is byte `off`"""
        self.line_at(off - len(seq) - (len(self.eol) - 1), seq)
        assert self.b[off] == 10

    def done(self, fillers=3):
        for _ in range(fillers):
            self.filler()
        return bytes(self.b)


EDGE_OFFS = [0, 63, 64, 65, 4095, 4096, 16383]


def edge_input(off, kind):
    """A '\\n' at tile offset `off` of tile 1: the end of a sequence line whose
    last window is a hit on both strands, or the end of a header, so that the
    sequence line behind it starts with a hit (forward at its first byte,
    reverse with the window start at its first byte)."""
    b = Build(100 + off)
    at = TILE + off
    if kind == "seq-end":
        b.line_ending_at(at, b.bases(100, fwd=(0, 84), rev=(40, 95)))
    else:
        b.line_at(at + 1, b.bases(100, fwd=(0, 50), rev=(11, 12 + 64, 95)))
    assert b.b[at] == 10
    return b.done()


def back_input(d):
    """A sequence line that starts in region 2 (d = 130: region 60) of tile 1
    and has its hits d regions further on: no '\\n' in the hits' region, in
    the d - 1 regions before it (d = 65: across a wave edge; d = 130: the
    whole of wave 1 lies inside the line)."""
    b = Build(200 + d)
    r0 = 60 if d == 130 else 2
    start = TILE + REGION * r0 + 10
    hit = REGION * d                      # line-relative: region r0 + d, offset 10
    b.line_at(start, b.bases(hit + 60, fwd=(0, hit, hit + 40), rev=(11, hit + 20, hit + 55)))
    return b.done()


def shift_input(sh):
    """GTCAT GTCAT GTCAT from offset sh (0..4) of the tile, of a region and of
    a wave: reverse hits with q at offsets 0..14 there, their window starts in
    the front halo, the previous region and the previous wave.  ATGAC at offset
    59 + sh of a region, of a wave's last region and of the tile's: forward
    hits that start in the last five bytes."""
    b = Build(300 + sh)
    rev3 = (40 + sh, 45 + sh, 50 + sh)
    b.line_at(TILE - 40, b.bases(100, rev=rev3))                           # tile 1, offset sh
    b.line_at(TILE + REGION * 10 - 40, b.bases(100, rev=rev3))            # region 10
    b.line_at(TILE + REGION * 20 + 19 + sh, b.bases(100, fwd=(40,)))      # region 20, offset 59 + sh
    b.line_at(TILE + WAVE - 40, b.bases(100, rev=rev3))                   # wave 1
    b.line_at(TILE + 2 * WAVE - 45 + sh, b.bases(100, fwd=(40,)))         # wave 1's last five bytes
    b.line_at(TILE + 3 * WAVE - 40, b.bases(100, rev=rev3))               # wave 3
    b.line_at(2 * TILE - 45 + sh, b.bases(100, fwd=(40,)))                # the tile's last five bytes
    d = b.done()
    for o in (TILE, TILE + REGION * 10, TILE + WAVE, TILE + 3 * WAVE):
        assert d[o + sh:o + sh + 15] == b"GTCAT" * 3
    for o in (TILE + REGION * 21, TILE + 2 * WAVE, 2 * TILE):
        assert d[o - 5 + sh:o + sh] == b"ATGAC"
    return d


def blank_crlf_input():
    """CRLF line ends and groups of four blank lines (the sequence lines keep
    their place in the count of four): several '\\n' per region."""
    b = Build(400, eol=b"\r\n")
    for i in range(150):
        b.filler(60 + i % 7)
        b.b += (b"\n\n\n\n", b"\r\n\r\n\r\n\r\n", b"\n\r\n\n\n")[i % 3]
    return bytes(b.b)


def tail_input():
    """No trailing newline, a length that is no multiple of 16, hits in the last line."""
    b = Build(500)
    for _ in range(40):
        b.filler()
    b.b += b"@last\n"
    m = 100 + (15 - (len(b.b) + 100)) % 16
    b.b += b.bases(m, fwd=(0, 50), rev=(11, 70, m - 5))   # the last window ends with the input
    n = len(b.b)
    assert n % 16 == 15
    return bytes(b.b)


def dense_input():
    """Reads of ATGAC x 30 over more than two tiles: some 250 queue entries
    and 1,400 hits per tile (rounds of the queue, the overflow list)."""
    b = Build(600)
    for _ in range(20):
        b.filler()
    for _ in range(2 * TILE // 311 + 10):
        b.record(b"ATGAC" * 30)
    return b.done()


def long_input():
    """One 20,000-base sequence line (longer than a tile, so tile 1 holds no
    '\\n' at all) with a motif every 97 bases."""
    b = Build(700)
    at = list(range(40, 19980, 97))
    b.line_at(TILE - 100, b.bases(20000, fwd=at[0::2], rev=at[1::2]))
    assert b"\n" not in b.b[TILE:2 * TILE]
    return b.done()


INPUTS = {}
for _off in EDGE_OFFS:
    for _kind in ("seq-end", "header-end"):
        INPUTS["nl%d-%s" % (_off, _kind)] = functools.partial(edge_input, _off, _kind)
for _d in (1, 2, 63, 65, 130):
    INPUTS["back%d" % _d] = functools.partial(back_input, _d)
for _sh in range(5):
    INPUTS["shift%d" % _sh] = functools.partial(shift_input, _sh)
INPUTS["blank-crlf"] = blank_crlf_input
INPUTS["tail"] = tail_input
INPUTS["dense"] = dense_input
INPUTS["long"] = long_input

# the other instantiations of the kernel: run-time k, wide keys, four plane-tested
# bytes, prefix bytes past the fifth, window = prefix
OTHER = [(17, b"ATGAC"), (40, b"ATGAC"), (16, b"ATGA"), (16, b"ATGACA"), (5, b"ATGAC")]
OTHER_INPUTS = ["shift2", "back65", "nl4096-header-end", "dense"]
CASES = [(name, 16, b"ATGAC") for name in INPUTS] + \
        [(name, k, prefix) for k, prefix in OTHER for name in OTHER_INPUTS]


@functools.lru_cache(maxsize=None)
def data(name):
    return INPUTS[name]()


@functools.lru_cache(maxsize=None)
def expected(name, k, prefix):
    from oracle import oracle
    return oracle.count_buffer(data(name), prefix, k, 1, stats=True)


def case_id(c):
    return "%s-k%d-%s" % (c[0], c[1], c[2].decode())


def test_inputs_are_small_and_no_case_is_vacuous():
    for name in INPUTS:
        assert len(data(name)) <= 5 * TILE, name
    for c in CASES:
        entries, st = expected(*c)
        assert entries and st["lines"] > 8, case_id(c)
    # the dense input's tiles overflow their 64 hit slots and need a second round of the queue
    assert data("dense")[TILE:2 * TILE].count(b"ATGAC") > 1000
    assert sum(v for _, v in expected("dense", 16, b"ATGAC")[0]) > 3000


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_whole_result_matches_the_oracle(case):
    import torch
    from kmerjs_amd import _native
    name, k, prefix = case
    want, st = expected(*case)
    buf = data(name)
    c = _native.Counter(k=k, prefix=prefix, flags=FLAG_LONG_LINES if name == "long" else 0)
    t = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    for rep in range(3):
        c.reset()
        c.feed_device(t.data_ptr(), len(buf))
        r = c.finish()
        got = r.entries()
        assert len(got) == len(want), (case_id(case), rep)
        assert first_diff(got, want) is None, (case_id(case), rep, first_diff(got, want))
        assert r.lines == st["lines"], (case_id(case), rep)
    c.close()
