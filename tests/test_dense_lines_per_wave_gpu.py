"""The dense-hit ordered path (kmer_dense.hip, dense_windows_kernel) with waves
that take several sequence lines.  A wave's share is ceil(lines / 2^17) lines,
so below 131,072 lines per chunk every wave has one line and most of the
kernel's state machine does not run: lanes dealt over up to 16 lines, a line
partly taken in a round that is not the wave's first, counts carried into a
round that also opens new lines, the advance when lane 63 ends at a line end,
the refetch inside a share, the last wave's clipped share.
KMER_FLAG_DENSE_LPW_TEST gives every wave 19 lines at any size;
kmer_dense_routes proves it.  Every case compares the whole ordered result
(keys, counts, order of entries, line count) with the oracle on the same
bytes.  W = line length - k + 1; a line takes ceil(W / 16) lanes; share w of a
chunk is its sequence ordinals [19 w, 19 w + 19).  One case takes the natural
route (262,221 lines in one chunk: 3 lines per wave without the flag)."""
import functools
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN_DIR
from tests.util import first_diff

pytestmark = pytest.mark.gpu

LPW = 19                      # lines per wave under KMER_FLAG_DENSE_LPW_TEST (kmer_api.h)
N_LINES = LPW * 40 + 7        # 40 whole shares and a clipped one
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def fastq(seqs):
    """Records with short other lines: '@r', the sequence, '+', an empty quality line."""
    return b"".join(b"@r\n" + s + b"\n+\n\n" for s in seqs)


def bases(rng, n):
    return ACGT[rng.integers(0, 4, size=int(n))].tobytes()


def lines_of(rng, lengths):
    lengths = [int(x) for x in lengths]
    pool = bases(rng, sum(lengths))
    out, o = [], 0
    for n in lengths:
        out.append(pool[o:o + n])
        o += n
    return out


# ---------------------------------------------------------------------------
# length patterns
# ---------------------------------------------------------------------------
def _reads(k, prefix, n=N_LINES):
    # k 16: 135 windows, 9 lanes per line; 16 lines want 144 lanes and lane 63 sits in line 7
    return lines_of(np.random.default_rng(100 + k), [150] * n)


def _tiny(k, prefix):
    # at most 2 lanes per line: 16 lines per round, then a refetch for the share's last 3;
    # lines without windows between lines with windows
    cyc = [k - 1, k, k + 1, k + 14, k + 15, k + 16, 0, 1, k + 31]
    return lines_of(np.random.default_rng(200 + k), [cyc[i % len(cyc)] for i in range(N_LINES)])


def _exact256(k, prefix):
    # W = 256, 16 lanes: four lines fill the wave exactly
    return lines_of(np.random.default_rng(300 + k), [k + 255] * N_LINES)


def _exact1024(k, prefix):
    # W = 1,024, 64 lanes: one line fills the round
    return lines_of(np.random.default_rng(400 + k), [k + 1023] * (LPW * 6 + 5))


LONG_POS = (0, 7, 15, 16, 18)           # share positions of the long lines: first, inside the first
LONG_W = (1025, 2500, 5000)             # fetch, its last, the refetch's first, the share's last


def _long(k, prefix):
    # one long line per share: entered behind other lines, continued from lane 0 over several
    # rounds with its counts carried, then followed by new lines in the same round
    lengths = [60] * N_LINES
    for w in range((N_LINES + LPW - 1) // LPW):
        o = LPW * w + LONG_POS[w % len(LONG_POS)]
        if o < N_LINES:
            lengths[o] = LONG_W[w % len(LONG_W)] + k - 1
    return lines_of(np.random.default_rng(500 + k), lengths)


def _exotic(k, prefix):
    # reads with about 1 % N, a few lower-case bases, and N / lower case placed inside and right
    # next to occurrences of the prefix and of its reverse complement (N and 'a' have A's code
    # bits: the planes alias them, the bytes decide)
    rng = np.random.default_rng(600 + k)
    rp = prefix.translate(COMP)[::-1]
    out = []
    for i, s in enumerate(lines_of(rng, [150] * N_LINES)):
        a = bytearray(s)
        for o in rng.integers(0, len(a), size=rng.integers(0, 4)):
            a[o] = ord("N")
        if i % 7 == 0:
            o = int(rng.integers(0, len(a)))
            a[o] = a[o] | 0x20
        if i % 3 == 0:
            for j, (pat, side) in enumerate(((prefix, 1), (rp, -1))):
                o = bytes(a).find(pat, int(rng.integers(0, 100)))
                if o < 0:
                    continue
                how = (i // 3 + j) % 3
                if how == 0:                                   # inside the occurrence
                    a[o + (i // 9) % len(pat)] = ord("N")
                elif how == 1:                                 # right behind it (in front of rc(P))
                    t = o + len(pat) if side > 0 else o - 1
                    if 0 <= t < len(a):
                        a[t] = ord("N")
                else:                                          # the occurrence in lower case
                    a[o:o + len(pat)] = pat.lower()
        out.append(bytes(a))
    return out


def _mixed(k, prefix):
    rng = np.random.default_rng(700 + k)
    choice = np.array([0, 1, k - 1, k, 30, 150, 151, 300, 1100])
    return lines_of(rng, choice[rng.integers(0, len(choice), size=N_LINES)])


PATTERNS = {"reads": _reads, "tiny": _tiny, "exact256": _exact256, "exact1024": _exact1024, "long": _long,
            "exotic": _exotic, "mixed": _mixed}
for _n in (1, LPW - 1, LPW, LPW + 1, LPW * 40):
    PATTERNS["reads%d" % _n] = functools.partial(_reads, n=_n)


@functools.lru_cache(maxsize=None)
def pattern(name, k, prefix):
    return fastq(PATTERNS[name](k, prefix))


@functools.lru_cache(maxsize=None)
def expected(data, k, prefix, fasta=False):
    from oracle import oracle
    return oracle.count_buffer(data, prefix, k, 1, stats=True, fasta=fasta)


# ---------------------------------------------------------------------------
# running and comparing
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    from kmerjs_amd import _native
    return _native


@pytest.fixture(scope="module")
def counters(native):
    """One context per configuration, shared by the cases (sessions on a used context)."""
    made = {}

    def get(k, prefix, flags, **kw):
        key = (k, prefix, flags, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = native.Counter(k=k, prefix=prefix, flags=flags, **kw)
        return made[key]
    yield get
    for c in made.values():
        c.close()


def feed(native, ctr, chunks, pos=None, what=""):
    """One session: reset, position, one device feed per chunk, finish.  A refused rank slot
    (ERR_DENSE_RANK) fails with the library's message: line, strand, rank, lines per wave."""
    import torch
    try:
        ctr.reset()
        if pos is not None:
            ctr.set_position(*pos)
        keep = []
        for ch in chunks:
            t = torch.frombuffer(bytearray(ch), dtype=torch.uint8).cuda()
            keep.append(t)
            ctr.feed_device(t.data_ptr(), len(ch))
        return ctr.finish()
    except native.KmerError as e:
        pytest.fail("%s: %s" % (what, e))


def where(data, k, diff):
    """The first sequence line that holds the differing key (or its reverse complement): its
    ordinal, its place in its share and its W name the kernel's branch."""
    key = diff[2][0] if diff[2] is not None else diff[1][0]
    rc = key.translate(COMP)[::-1]
    for o, s in enumerate(data.split(b"\n")[1::4]):
        if key in s or rc in s:
            return "first in sequence line %d (share position %d, W %d)" % (o, o % LPW, max(len(s) - k + 1, 0))
    return "in no sequence line"


def check(r, want, data, k, what):
    entries, st = want
    got = r.entries()
    d = first_diff(got, entries)
    assert d is None, (what, d, where(data, k, d))
    assert len(got) == len(entries), what
    assert r.lines == st["lines"], what


def same_arrays(a, b):
    return (a.keybuf == b.keybuf and np.array_equal(a.offsets, b.offsets) and np.array_equal(a.counts, b.counts) and
            np.array_equal(a.firsts, b.firsts) and a.lines == b.lines)


# ---------------------------------------------------------------------------
# every pattern, every key layout
# ---------------------------------------------------------------------------
CONFIGS = [(12, b"G"),       # 22 key bits: bucket finish
           (16, b"AT"),      # 28 bits: 32-bit sort
           (21, b"ACG"),     # 36 bits: 64-bit keys
           (32, b"AT"),      # the longest k of the narrow kernel
           (33, b"A"),       # the shortest k of the WIDE kernel, keys of exactly 64 bits
           (40, b"AT"),
           (64, b"ACG")]
CONFIG_IDS = ["k%d-%s" % (k, p.decode()) for k, p in CONFIGS]


def test_patterns_are_what_they_claim():
    """The shapes the cases rely on (no GPU work)."""
    assert N_LINES % LPW == 7 and (LPW * 6 + 5) % LPW == 5
    k = 16
    seqs = _long(k, b"AT")
    longs = [(o % LPW, len(s) - k + 1) for o, s in enumerate(seqs) if len(s) != 60]
    assert len(longs) == 41 and {p for p, _ in longs} == set(LONG_POS) and {w for _, w in longs} == set(LONG_W)
    assert all(sum(len(s) != 60 for s in seqs[o:o + LPW]) == 1 for o in range(0, N_LINES, LPW))
    assert {len(s) for s in _mixed(k, b"AT")} == {0, 1, 15, 16, 30, 150, 151, 300, 1100}
    ex = b"\n".join(_exotic(k, b"AT"))
    assert 0.005 < ex.count(b"N") / len(ex) < 0.02 and b"at" in ex and b"NT" in ex and b"ATN" in ex
    assert all(len(pattern(name, 64, b"ACG")) < 1 << 20 for name in PATTERNS)


@pytest.mark.parametrize("name", list(PATTERNS))
@pytest.mark.parametrize("k,prefix", CONFIGS, ids=CONFIG_IDS)
def test_pattern_vs_oracle(native, counters, k, prefix, name):
    data = pattern(name, k, prefix)
    want = expected(data, k, prefix)
    assert want[0] or name == "reads1"
    ctr = counters(k, prefix, native.FLAG_DENSE_LPW_TEST)
    check(feed(native, ctr, [data], what=name), want, data, k, name)
    assert ctr.dense_routes() == {"chunks": 1, "lines_per_wave": LPW}


MORE = [(16, b"AT"), (40, b"AT")]
MORE_IDS = ["k16-AT", "k40-AT"]


@pytest.mark.parametrize("name", ["reads", "long", "mixed"])
@pytest.mark.parametrize("k,prefix", MORE, ids=MORE_IDS)
def test_long_line_mode_sort_finish_and_default_share(native, counters, k, prefix, name):
    data = pattern(name, k, prefix)
    want = expected(data, k, prefix)
    flagged = feed(native, counters(k, prefix, native.FLAG_DENSE_LPW_TEST), [data], what=name)
    for extra in (native.FLAG_LONG_LINES, native.FLAG_SORT_FINISH):
        ctr = counters(k, prefix, native.FLAG_DENSE_LPW_TEST | extra)
        check(feed(native, ctr, [data], what=(name, extra)), want, data, k, (name, extra))
        assert ctr.dense_routes()["lines_per_wave"] == LPW
    # without the flag: one line per wave, and the same result array for array
    ctr = counters(k, prefix, 0)
    plain = feed(native, ctr, [data], what=(name, "default"))
    assert ctr.dense_routes() == {"chunks": 1, "lines_per_wave": 1}
    check(plain, want, data, k, (name, "default"))
    assert same_arrays(plain, flagged), name


# ---------------------------------------------------------------------------
# sessions: several chunks (shares restart per chunk, out_base > 0), a position, host batches
# ---------------------------------------------------------------------------
def session_chunks(k, prefix):
    return [pattern(name, k, prefix) for name in ("reads", "long", "tiny")]


@pytest.mark.parametrize("k,prefix", MORE, ids=MORE_IDS)
def test_three_feeds_twice(native, counters, k, prefix):
    chunks = session_chunks(k, prefix)
    ends = np.cumsum([ch.count(b"\n") // 4 for ch in chunks])
    assert all(e % LPW for e in ends[:-1])         # (the cuts are no share boundaries of the whole input)
    data = b"".join(chunks)
    want = expected(data, k, prefix)
    ctr = counters(k, prefix, native.FLAG_DENSE_LPW_TEST)
    for rep in range(2):
        check(feed(native, ctr, chunks, what=rep), want, data, k, rep)
        assert ctr.dense_routes() == {"chunks": 3, "lines_per_wave": LPW}


@pytest.mark.parametrize("k,prefix", MORE, ids=MORE_IDS)
def test_three_feeds_positioned(native, counters, k, prefix):
    """The session starts at the first sequence line, as line 5 of a stream (five empty lines in
    front for the oracle)."""
    chunks = session_chunks(k, prefix)
    lo = chunks[0].index(b"\n") + 1
    chunks[0] = chunks[0][lo:]
    data = b"\n" * 5 + b"".join(chunks)
    want = expected(data, k, prefix)
    assert want[0] == expected(b"@r\n" + data[5:], k, prefix)[0]
    ctr = counters(k, prefix, native.FLAG_DENSE_LPW_TEST)
    check(feed(native, ctr, chunks, pos=(5, 5), what="positioned"), want, data, k, "positioned")
    assert ctr.dense_routes() == {"chunks": 3, "lines_per_wave": LPW}


@pytest.mark.parametrize("k,prefix", MORE, ids=MORE_IDS)
def test_host_batches(native, counters, k, prefix):
    """kmer_count_buffer in batches of 64 KiB (cut at any line end), and the reads in batches of
    2 KiB: a dozen lines per chunk, fewer than one share."""
    data = b"".join(session_chunks(k, prefix))
    assert 2048 // len(fastq([b"A" * 150])) < LPW
    for batch, buf in ((65536, data), (2048, pattern("reads", k, prefix)[:40000])):
        ctr = counters(k, prefix, native.FLAG_DENSE_LPW_TEST, batch_bytes=batch)
        try:
            r = ctr.count_buffer(buf)
        except native.KmerError as e:
            pytest.fail("batches of %d: %s" % (batch, e))
        check(r, expected(buf, k, prefix), buf, k, batch)
        routes = ctr.dense_routes()
        assert routes["lines_per_wave"] == LPW and routes["chunks"] >= len(buf) // batch, routes


# ---------------------------------------------------------------------------
# FASTA records (rewritten into sequence lines on the device)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fasta_records():
    rng = np.random.default_rng(800)
    out = bytearray()
    for i in range(100):
        out += b">s%d\n" % i
        for _ in range(int(rng.integers(1, 41))):
            out += bases(rng, rng.integers(0, 81)) + b"\n"
    return bytes(out)


@pytest.mark.parametrize("which", ["edge_contigs", "records"])
def test_fasta(native, counters, which):
    k, prefix = 16, b"AT"
    if which == "records":
        data = fasta_records()
    else:
        with open(os.path.join(GOLDEN_DIR, "inputs", "edge_contigs.fsa"), "rb") as f:
            data = f.read()
    want = expected(data, k, prefix, fasta=True)
    assert want[0]
    ctr = counters(k, prefix, native.FLAG_FASTA | native.FLAG_DENSE_LPW_TEST)
    try:
        r = ctr.count_buffer(data)
    except native.KmerError as e:
        pytest.fail("%s: %s" % (which, e))
    d = first_diff(r.entries(), want[0])
    assert d is None, (which, d)
    assert r.lines == want[1]["lines"]
    assert ctr.dense_routes()["lines_per_wave"] == LPW


# ---------------------------------------------------------------------------
# the natural route: more than 2 * 2^17 lines in one chunk, no flag
# ---------------------------------------------------------------------------
N_NATURAL = 2 * (1 << 17) + 77


@functools.lru_cache(maxsize=None)
def natural_input():
    rng = np.random.default_rng(900)
    n = N_NATURAL
    lengths = rng.integers(14, 41, size=n)
    lengths[::997] = 400
    lengths[5::1500] = 1300
    lengths[3::211] = rng.integers(0, 13, size=len(lengths[3::211]))
    return b"".join(b"@\n" + s + b"\n+\n\n" for s in lines_of(rng, lengths))


@pytest.mark.parametrize("k,prefix", [(12, b"AC"), (40, b"AT")], ids=["k12-AC", "k40-AT"])
def test_natural_three_lines_per_wave(native, counters, k, prefix):
    data = natural_input()
    assert 8_000_000 < len(data) < 10_000_000
    want = expected(data, k, prefix)
    assert len(want[0]) > 10_000
    ctr = counters(k, prefix, 0)
    check(feed(native, ctr, [data], what="natural"), want, data, k, "natural")
    # (if the share's divisor changes: resize the input so that this still holds)
    assert ctr.dense_routes() == {"chunks": 1, "lines_per_wave": 3}
