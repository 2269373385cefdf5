"""Hit resolution and the ordered emit, in the instantiation compiled for the
default shape (k = 16, ATGAC, narrow keys, default order-key layout) and in
the run-time one that every other shape takes.  Every case runs one session on
the device and compares the whole ordered result (keys, counts,
first-occurrence order, line count) with the oracle on the same bytes, and
checks that the oracle counted what the input was built to hold.

The session flag INFO_LONGSEG of an overflowed tile is not visible through
the API; the overflow case is checked by its result."""
import functools

import pytest

from tests.hit_path_util import (EMIT_RPB, FLAG_LONG_LINES, FLAG_SORT_FINISH, HMAX, REC, SEQ, TILE, check, counter,
                                 oracle_count, pad, planted_read, planted_reads, random_reads, read, record, run,
                                 suffix, tile_of, total, windows)

pytestmark = pytest.mark.gpu

SHAPES = [(16, b"ATGAC"), (16, b"ATGAA"), (15, b"ATGAC"), (17, b"ATGAC"), (16, b"ATGA"), (16, b"ATGACA"),
          (32, b"ATGAC"), (33, b"ATGAC"), (40, b"ATGAC")]
FLAGS = [0, FLAG_SORT_FINISH, FLAG_LONG_LINES]


@functools.lru_cache(maxsize=None)
def shape_input(k, prefix):
    """Three tiles of random reads with planted prefixes, and the oracle's answer."""
    data = random_reads(3 * TILE // REC, prefix, seed=k * 131 + len(prefix))
    want = oracle_count(data, prefix, k)
    assert total(want) == windows(data, prefix, k) >= 80
    return data, want


@pytest.mark.parametrize("flags", FLAGS, ids=["bucket", "sort", "long_lines"])
@pytest.mark.parametrize("k,prefix", SHAPES, ids=["%d-%s" % (k, p.decode()) for k, p in SHAPES])
def test_shapes_next_to_the_default(k, prefix, flags):
    data, want = shape_input(k, prefix)
    c = counter(k=k, prefix=prefix, flags=flags)
    check(run(c, [data]), want, (k, prefix, flags))
    c.close()


@pytest.mark.parametrize("tiles", [1, 3, 4, 5, 16, 17])
def test_tiles_per_wave_and_workgroup(tiles):
    """The last wave with fewer than four tiles, the last workgroup with fewer
    than four waves."""
    data = random_reads(tiles * TILE // REC, b"ATGAC", seed=tiles)
    assert (tiles - 1) * TILE < len(data) <= tiles * TILE
    want = oracle_count(data)
    assert total(want) == windows(data, b"ATGAC", 16) > 0
    c = counter()
    check(run(c, [data]), want, tiles)
    c.close()


def test_hit_counts_per_tile():
    """The four tiles of a wave with {0, 1, 63, 64} and {65, 0, 64, 2} hits; 65
    is past the tile's hit slots (all of its hits go the cross route)."""
    per_tile = [0, 1, HMAX - 1, HMAX, HMAX + 1, 0, HMAX, 2]
    data, first = b"", 0
    for t, n in enumerate(per_tile):
        data += tile_of(n, first, first_read=1000 * t)
        first += n
    assert len(data) == 8 * TILE
    want = oracle_count(data)
    assert [c for _, c in want[0]] == [1] * sum(per_tile)        # every hit its own key
    for flags in (0, FLAG_SORT_FINISH):
        c = counter(flags=flags)
        check(run(c, [data]), want, flags)
        c.close()


def test_order_inside_a_line():
    """Forward (ATGAC...) and reverse (...GTCAT) hits interleaved in one line:
    the reverse strand's rank by descending position, behind the forward ones."""
    reads = []
    for i in range(60):
        seq = bytearray(b"C" * SEQ)
        for c in range(9):
            s = suffix(9 * i + c)
            seq[16 * c:16 * c + 16] = b"ATGAC" + s if c % 2 == 0 else s + b"GTCAT"
        reads.append(read(i, bytes(seq)))
    data = b"".join(reads)
    assert data.count(b"ATGAC") == 60 * 5 and data.count(b"GTCAT") == 60 * 4
    want = oracle_count(data)
    assert total(want) == 60 * 9 == windows(data, b"ATGAC", 16)
    c = counter()
    check(run(c, [data]), want, "interleaved")
    c.close()


@functools.lru_cache(maxsize=None)
def line_structure_input():
    """A sequence line across the first tile edge with hits on both sides; a
    header and a quality line that hold ATGAC windows; a window with N in its
    suffix."""
    per = TILE // REC
    data = planted_reads(0, 9 * per)                             # 51 reads
    data += pad(129)                                             # the next read's bases begin 75 bytes before the edge
    assert len(data) + 13 == TILE - 75
    data += planted_read(900, range(600, 609))
    data += record(b"@ATGACCGCGCGCGCGCGCGCG", b"C" * 40 + b"ATGAC" + suffix(700) + b"C" * 20,
                   b"I" * 10 + b"ATGACGCGCGCGCGCGCGCG" + b"I" * 46)
    data += record(b"@n", b"C" * 8 + b"ATGACNCGCGCGCGCG" + b"C" * 8 + b"ATGAC" + suffix(701))
    data += planted_reads(800, 90, first_read=2000)
    return data


def test_line_structure():
    data = line_structure_input()
    want = oracle_count(data)
    # 51 + 1 + 10 planted reads of nine, the two records' three sequence-line windows; not the header's or the quality's
    assert total(want) == 9 * 51 + 9 + 3 + 90 == windows(data, b"ATGAC", 16)
    assert data.count(b"ATGAC") == total(want) + 2
    assert any(b"N" in key for key, _ in want[0])
    for flags in (0, FLAG_SORT_FINISH):
        c = counter(flags=flags)
        check(run(c, [data]), want, flags)
        c.close()


@pytest.mark.parametrize("skip", [0, 1, 2, 3, 6])
def test_set_position(skip):
    """A session that begins at line `skip` of the input: the line-index rule
    runs on lines_before + the lines fed."""
    data = line_structure_input()
    at = 0
    for _ in range(skip):
        at = data.index(b"\n", at) + 1
    part = data[at:]
    model = b"\n" * skip + part                  # (empty lines hold no window)
    want = oracle_count(model)
    assert total(want) == windows(model, b"ATGAC", 16) > 500
    c = counter()
    check(run(c, [part], position=(skip, at)), want, skip)
    c.close()


def test_two_chunks():
    """The second chunk's hits are placed behind the first's (rank and cross bases)."""
    data = line_structure_input()
    at = REC * 40
    want = oracle_count(data)
    for flags in (0, FLAG_SORT_FINISH):
        c = counter(flags=flags)
        check(run(c, [data[:at], data[at:]]), want, flags)
        c.close()


@pytest.mark.parametrize("last_repeat", [False, True], ids=["last_head", "last_repeat"])
@pytest.mark.parametrize("n", [100, EMIT_RPB, EMIT_RPB + 1, EMIT_RPB + 255, EMIT_RPB + 256, EMIT_RPB + 257,
                               2 * EMIT_RPB - 1])
def test_emit_totals(n, last_repeat):
    """n ranks around the emit workgroup's and its rounds' sizes; the last rank
    a key's first occurrence, or a repeat of the first key."""
    if last_repeat:
        data = planted_reads(0, n - 1) + planted_read(5000, [0])
    else:
        data = planted_reads(0, n)
    assert data.count(b"ATGAC") == n
    want = oracle_count(data)
    assert total(want) == n and len(want[0]) == n - last_repeat
    c = counter()
    check(run(c, [data]), want, (n, last_repeat))
    c.close()


@pytest.mark.parametrize("flags", [0, FLAG_SORT_FINISH], ids=["bucket", "sort"])
@pytest.mark.parametrize("count", [254, 255, 256])
def test_emit_counts_around_the_full_mark(count, flags):
    """One key counted 254, 255 or 256 times beside keys of count 1."""
    data = planted_reads(0, 200) + planted_read(7000, [2040]) * count + planted_reads(300, 50, first_read=8000)
    want = oracle_count(data)
    assert sorted(c for _, c in want[0]) == [1] * 250 + [count]
    c = counter(flags=flags)
    check(run(c, [data]), want, (count, flags))
    c.close()
