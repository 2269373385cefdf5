"""Head marks on the bucket route of the ordered finish: a rank's head count is
kept as one byte, min(count, 255), and in full in the 4-byte array only where
the byte is 255 (that array is no longer cleared on this route).  Counts on
both sides of the escape, next to counts of 1, and a context whose ranks held
large counts in the session before.  Every case compares the whole ordered
result (keys, counts, first-occurrence order, line count) with the oracle on
the same bytes, and checks that the oracle counted what the input was built to
hold.  The sort route (KMER_FLAG_SORT_FINISH) keeps 4-byte counts and must
agree; the counted bucket route is covered by test_bucket_onepass_gpu.py."""
import functools

import pytest

from tests.util import first_diff

pytestmark = pytest.mark.gpu

TILE = 16384
REC = 317                  # bytes per read, as the synthetic reads
SEQ = 150                  # bases per read
FLAG_SORT_FINISH = 8       # KMER_FLAG_SORT_FINISH (kmer_api.h)
FULL = 255                 # the mark that sends the reader to the 4-byte count
REPEATS = [FULL - 1, FULL, FULL + 1, 1000]


def counter(k=16, prefix=b"ATGAC", flags=0):
    from kmerjs_amd import _native
    return _native.Counter(k=k, prefix=prefix, flags=flags)


def run(ctr, chunks):
    """One session: reset, one device feed per chunk, finish."""
    import torch
    ctr.reset()
    keep = []
    for ch in chunks:
        t = torch.frombuffer(bytearray(ch), dtype=torch.uint8).cuda()
        keep.append(t)
        ctr.feed_device(t.data_ptr(), len(ch))
    return ctr.finish()


def oracle_count(data, prefix=b"ATGAC", k=16):
    from oracle import oracle
    return oracle.count_buffer(data, prefix, k, 1, stats=True)


def check(r, want, what):
    entries, st = want
    got = r.entries()
    assert len(got) == len(entries), what
    assert first_diff(got, entries) is None, what
    assert r.lines == st["lines"], what


def _read(i, seq):
    assert len(seq) == SEQ
    rec = b"@r%010d\n" % i + seq + b"\n+\n" + b"I" * SEQ + b"\n"
    assert len(rec) == REC
    return rec


def _suffix(index):
    """11 bases over {C, G} that spell `index`, low bit first."""
    assert index < 1 << 11
    return bytes(b"CG"[(index >> b) & 1] for b in range(11))


def _planted_read(i, indices):
    """A read of C with ATGAC + _suffix(index) at every 16th base: one forward
    hit with its own key per index, and no GTCAT (a T is always followed by G)."""
    assert 16 * len(indices) <= SEQ
    seq = bytearray(b"C" * SEQ)
    for c, index in enumerate(indices):
        seq[16 * c:16 * (c + 1)] = b"ATGAC" + _suffix(index)
    return _read(i, bytes(seq))


@functools.lru_cache(maxsize=None)
def repeated(n):
    """One read with three planted hits, n times: three keys of count n, whose
    first occurrences are the first three ranks."""
    data = _planted_read(0, (2000, 2001, 2002)) * n
    assert len(data) <= 320_000 and data.count(b"ATGAC") == 3 * n and b"GTCAT" not in data
    return data


@functools.lru_cache(maxsize=None)
def singles(m):
    """m hits with m different keys (none of repeated()'s), nine per read."""
    data = b"".join(_planted_read(i, range(9 * i, min(9 * i + 9, m))) for i in range((m + 8) // 9))
    assert data.count(b"ATGAC") == m and b"GTCAT" not in data
    return data


@pytest.mark.parametrize("flags", [0, FLAG_SORT_FINISH], ids=["bucket", "sort"])
@pytest.mark.parametrize("n", REPEATS)
def test_counts_around_the_full_mark(n, flags):
    data = repeated(n)
    want = oracle_count(data)
    assert [c for _, c in want[0]] == [n, n, n]                  # 3 n accepted windows, three keys
    c = counter(flags=flags)
    for rep in range(2):
        check(run(c, [data]), want, (n, flags, rep))
    c.close()


@pytest.mark.parametrize("flags", [0, FLAG_SORT_FINISH], ids=["bucket", "sort"])
def test_full_marks_next_to_small_counts(flags):
    """Counts of 1,000 and of 1 in one session (the large ones first, last and
    split by the small ones), then sessions of small counts only on the ranks
    that held the large ones: a stale 4-byte count is never read."""
    small = singles(200)
    c = counter(flags=flags)
    for what, data in [("large first", repeated(1000) + small), ("large last", small + repeated(1000)),
                       ("split", repeated(FULL) + small + repeated(1000 - FULL))]:
        want = oracle_count(data)
        assert sorted(n for _, n in want[0]) == [1] * 200 + [1000] * 3, what
        check(run(c, [data]), want, (what, flags))
        want = oracle_count(small)
        assert [n for _, n in want[0]] == [1] * 200
        check(run(c, [small]), want, (what, "small after", flags))
    c.close()


def test_two_chunks_cross_the_full_mark():
    """200 + 55 repeats in two chunks: the count reaches 255 only at the finish."""
    data = repeated(FULL)
    at = REC * 200
    want = oracle_count(data)
    assert [c for _, c in want[0]] == [FULL] * 3
    c = counter()
    check(run(c, [data[:at], data[at:]]), want, "two chunks")
    c.close()
