"""The bucket finish behind a plain session (k = 16, ATGAC: 22 key bits, 256
buckets of 2^14 keys) around the one-pass partition's block of 8,192 hits: a
block loads its 16 keys per thread before it uses the first, claims a run in
every bucket it has keys for, and the region rule gives a bucket 1.5 times the
mean and one such block.  Every case builds an input whose sequence lines hold
exactly n ATGAC windows with chosen keys, runs one session and compares the
whole ordered result with the oracle on the same bytes."""
import functools
import itertools

import pytest

from tests.hit_path_util import SEQ, check, counter, oracle_count, read, run, total, windows

pytestmark = pytest.mark.gpu

E = 8192                   # hits per one-pass partition block (BKT_OP_EPB, kmer_kernels.hip)
E_OLD = 4096               # ... of the counted route's kernels, and of the one-pass route before
NB = 256                   # buckets: 22 key bits, 14 of them inside a bucket
WPR = 8                    # windows per read: ATGAC + 11 bases + a G, every 17th base

X4 = ["".join(p).encode() for p in itertools.product("ACGT", repeat=4)]


def bucket_cap(n, nb=NB):
    # the region rule (kmer_internal.hpp): cap = ceil(n / nb) * 3 / 2 + one one-pass block
    return (n + nb - 1) // nb * 3 // 2 + E


def spread_key(i):
    """Key i of 65,536: the first four and the last four bases each take every
    value, so the keys spread over every bucket whichever end the bucket is
    taken from.  (A G after the first four, a C before the last four and the G
    behind every window keep ATGAC and GTCAT from forming anywhere else.)"""
    return X4[i % 256] + b"GCC" + X4[(i // 256) % 256]


def one_bucket_key(i):
    """Eight keys that share their first and their last four bases: one bucket."""
    return b"CCCC" + bytes(b"CG"[(i >> b) & 1] for b in range(3)) + b"CCCC"


def hits_input(keys):
    """Reads whose sequence lines hold exactly one forward window per key, in order."""
    keys = list(keys)
    out = []
    for j in range(0, max(len(keys), 1), WPR):
        seq = bytearray(b"G" * SEQ)
        for c, key in enumerate(keys[j:j + WPR]):
            assert len(key) == 11
            seq[17 * c:17 * c + 16] = b"ATGAC" + key
        out.append(read(j // WPR, bytes(seq)))
    return b"".join(out)


def checked(data, n):
    want = oracle_count(data)
    assert total(want) == n == windows(data, b"ATGAC", 16)
    return want


@functools.lru_cache(maxsize=None)
def sized(n):
    data = hits_input(spread_key(i) for i in range(n))
    return data, checked(data, n)


SIZES = sorted({0, 1, E - 1, E, E + 1, 2 * E, 3 * E + 7, E_OLD - 1, E_OLD, E_OLD + 1, 2 * E_OLD, 3 * E_OLD + 7})


@pytest.mark.parametrize("n", SIZES)
def test_hits_around_the_block_sizes(n):
    data, want = sized(n)
    assert len(want[0]) == n                     # (every hit its own key)
    c = counter()
    check(run(c, [data]), want, n)
    c.close()


def test_one_key_in_every_bucket():
    data = hits_input(X4[i] + b"GCC" + X4[i] for i in range(NB))
    want = checked(data, NB)
    assert len(want[0]) == NB
    c = counter()
    check(run(c, [data]), want, "every bucket")
    c.close()


def test_bucket_at_and_past_its_region():
    """cap = ceil(n / 256) * 3 / 2 + 8,192.  With all n hits in one bucket,
    n = cap(n) fills the region exactly; one more (the rule gives the same cap)
    is past it: ERR_BKT_CAP, the counted kernels redo the finish, and the
    result is still exact.  (Which route a finish took is not visible through
    the API: both sides of the edge are checked by their result.)"""
    m = next(n for n in range(E, 2 * E) if bucket_cap(n) == n)
    assert bucket_cap(m + 1) == m
    c = counter()
    for n in (m, m + 1):
        data = hits_input(one_bucket_key(i) for i in range(n))
        check(run(c, [data]), checked(data, n), n)
    # (the context stays on the counted route from here on)
    data, want = sized(E + 1)
    check(run(c, [data]), want, "after the redo")
    c.close()


@pytest.mark.parametrize("n", [16384, 16385])
def test_first_round_of_a_bucket_table(n):
    """All hits in one bucket: 16,384 fill the first round of
    bucket_heads_kernel (16 entries per thread), one more takes a second.  So
    few hits cannot put 16,384 into one of 256 regions (cap = 8,288 and 8,289
    here; it would take about 1.4 M hits), so the edge is met through
    ERR_BKT_CAP and the counted redo, whose bucket bounds the same loop walks."""
    assert bucket_cap(n) < n
    data = hits_input(one_bucket_key(i) for i in range(n))
    want = checked(data, n)
    assert len(want[0]) == 8
    c = counter()
    check(run(c, [data]), want, n)
    c.close()


@pytest.mark.parametrize("count", [254, 255, 256])
def test_counts_around_the_full_mark(count):
    keys = [spread_key(i) for i in range(200)] + [spread_key(7000)] * count + [spread_key(300 + i) for i in range(50)]
    data = hits_input(keys)
    want = checked(data, 250 + count)
    assert sorted(c for _, c in want[0]) == [1] * 250 + [count]
    c = counter()
    check(run(c, [data]), want, count)
    c.close()


def test_smaller_finish_after_a_larger_one():
    """reset() between finishes on one context: the cursors are back at 0, and
    what an earlier finish left in the regions and the marks is never read."""
    c = counter()
    for n in (2 * E, 1, E_OLD + 1, 2 * E, 0, E - 1):
        data, want = sized(n)
        check(run(c, [data]), want, n)
    c.close()
