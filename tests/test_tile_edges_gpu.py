"""Inputs that end at, just before and just after a tile edge (TILE = 16384
bytes: one workgroup stages one tile plus its halos in LDS), through every
route that stages tiles: the plane scan, the byte scan, the general path's
plane-candidate kernel and FASTA mode.  A sequence line straddles each tile
edge and carries the prefix and its reverse complement densely there, so
windows start in one tile and end in the next, and the cuts fall in mid-line
(legal input: the last line is unterminated).  Every result equals the
oracle's entry for entry, in order."""
import numpy as np
import pytest

from tests.util import first_diff

pytestmark = pytest.mark.gpu

TILE = 16384
CUTS = [TILE - 1, TILE, TILE + 1, TILE + 15, 2 * TILE + 1]
ROUTES = ["planes", "bytes", "gen_cand", "fasta"]


def _motif_rich(rng, n):
    """n bases in which ATGAC and GTCAT turn up every few positions."""
    pieces = [b"ATGAC", b"GTCAT", b"A", b"C", b"G", b"T"]
    out = b""
    while len(out) < n:
        out += pieces[int(rng.integers(0, len(pieces)))]
    return out[:n]


def _header(mark, name, at):
    """Header line at offset `at`, padded when its record reaches a tile edge
    so that the sequence line starts 70 bytes before the edge."""
    edge = (at // TILE + 1) * TILE
    pad = edge - 70 - (at + 1 + len(name) + 1)
    return mark + name + b"x" * (pad if 0 <= pad < 400 else 0) + b"\n"


def make_texts(seed=20, total=2 * TILE + 400):
    """(fastq, fasta): the same seeded reads in both shapes.  A sequence line
    straddles each tile edge, and the sequence bytes within 48 bytes of an edge
    are motif-rich."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    fq, fa = bytearray(), bytearray()
    fq_seq, fa_seq = [], []                 # (start, length) of every sequence line
    r = 0
    while len(fq) < total or len(fa) < total:
        name = b"read%d/%d" % (r, int(rng.integers(0, 1 << 20)))
        seq = acgt[rng.integers(0, 4, 150)].tobytes()
        fq += _header(b"@", name, len(fq))
        fq_seq.append((len(fq), len(seq)))
        fq += seq + b"\n+\n" + b"I" * len(seq) + b"\n"
        fa += _header(b">", name, len(fa))
        fa_seq.append((len(fa), len(seq)))
        fa += seq + b"\n"
        r += 1
    for text, lines in ((fq, fq_seq), (fa, fa_seq)):
        for edge in (TILE, 2 * TILE):
            hit = [(s, n) for s, n in lines if s < edge - 16 and s + n > edge + 16]
            assert hit, "no sequence line straddles the tile edge"
            s, n = hit[0]
            a, b = max(s, edge - 48), min(s + n, edge + 48)
            text[a:b] = _motif_rich(rng, b - a)
    return bytes(fq), bytes(fa)


def route_args(native, route):
    """(k, prefix, counter flags, input is FASTA) of a route."""
    return {"planes": (16, b"ATGAC", 0, False),
            "bytes": (16, b"ATGAC", native.FLAG_BYTE_SCAN, False),
            "gen_cand": (70, b"ATGAC", 0, False),
            "fasta": (16, b"ATGAC", native.FLAG_FASTA, True)}[route]


@pytest.fixture(scope="module")
def native():
    from kmerjs_amd import _native
    return _native


@pytest.fixture(scope="module")
def expected(native):
    """{(route, cut): (input, oracle entries)}, computed once."""
    from oracle import oracle
    fq, fa = make_texts()
    out = {}
    for route in ROUTES:
        k, prefix, _, fasta = route_args(native, route)
        for cut in CUTS:
            data = (fa if fasta else fq)[:cut]
            out[route, cut] = (data, oracle.count_buffer(data, prefix, k, 1, fasta=fasta))
    return out


@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("route", ROUTES)
def test_tile_edge_cut_vs_oracle(native, expected, route, cut):
    k, prefix, flags, _ = route_args(native, route)
    data, want = expected[route, cut]
    assert len(data) == cut and want
    ctr = native.Counter(k=k, prefix=prefix, flags=flags)
    got = ctr.count_buffer(data).entries()
    ctr.close()
    assert len(got) == len(want), (route, cut)
    assert first_diff(got, want) is None, (route, cut)
