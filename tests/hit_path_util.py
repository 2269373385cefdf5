"""Helpers of the hit-path tests (test_hit_path_shapes_gpu.py): one session on
the device against the oracle on the same bytes, and small FASTQ inputs built
read by read so that a test knows what its input holds."""
import random

from tests.util import first_diff

TILE = 16384
REC = 317                  # bytes per read, as the synthetic reads
SEQ = 150                  # bases per read
FLAG_SORT_FINISH = 8       # KMER_FLAG_SORT_FINISH (kmer_api.h)
FLAG_LONG_LINES = 128      # KMER_FLAG_LONG_LINES
EMIT_RPB = 1024            # ranks per emit workgroup (kmer_kernels.hip)
HMAX = 64                  # hit slots per tile (kmer_internal.hpp)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def counter(k=16, prefix=b"ATGAC", flags=0):
    from kmerjs_amd import _native
    return _native.Counter(k=k, prefix=prefix, flags=flags)


def run(ctr, chunks, position=None):
    """One session: reset, (set_position,) one device feed per chunk, finish."""
    import torch
    ctr.reset()
    if position is not None:
        ctr.set_position(*position)
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


def total(want):
    return sum(c for _, c in want[0])


def revcomp(s):
    return s.translate(COMP)[::-1]


def record(header, seq, qual=None):
    """One four-line record: 2 |seq| + |header| + 5 bytes."""
    qual = b"I" * len(seq) if qual is None else qual
    assert len(qual) == len(seq) and header.startswith(b"@")
    return header + b"\n" + seq + b"\n+\n" + qual + b"\n"


def read(i, seq):
    assert len(seq) == SEQ
    rec = record(b"@r%010d" % i, seq)
    assert len(rec) == REC
    return rec


def pad(nbytes):
    """A record of nbytes bytes without a hit (nbytes odd, >= 9)."""
    assert nbytes >= 9 and nbytes % 2 == 1
    rec = record(b"@p", b"C" * ((nbytes - 7) // 2))
    assert len(rec) == nbytes
    return rec


def suffix(index):
    """11 bases over {C, G} that spell `index`, low bit first."""
    assert 0 <= index < 1 << 11
    return bytes(b"CG"[(index >> b) & 1] for b in range(11))


def planted_read(i, indices):
    """A read of C with ATGAC + suffix(index) at every 16th base: one forward
    hit with its own key per index, and no GTCAT (a T is always followed by G)."""
    indices = list(indices)
    assert 16 * len(indices) <= SEQ
    seq = bytearray(b"C" * SEQ)
    for c, index in enumerate(indices):
        seq[16 * c:16 * (c + 1)] = b"ATGAC" + suffix(index)
    return read(i, bytes(seq))


def planted_reads(first_index, n_hits, first_read=0):
    """n_hits hits with the keys first_index, first_index + 1, ..., nine per read."""
    return b"".join(planted_read(first_read + j, range(first_index + 9 * j, first_index + min(9 * j + 9, n_hits)))
                    for j in range((n_hits + 8) // 9))


def tile_of(n_hits, first_index, first_read=0):
    """Exactly one tile (16 KiB, whole records) that holds n_hits planted hits."""
    per = TILE // REC                            # 51 reads and a pad record of 217 bytes
    body = planted_reads(first_index, n_hits, first_read)
    body += b"".join(read(first_read + 100 + j, b"C" * SEQ) for j in range(per - len(body) // REC))
    t = body + pad(TILE - len(body))
    assert len(t) == TILE and t.count(b"ATGAC") == n_hits
    return t


def random_reads(n, prefix, seed):
    """n reads of random bases; every third has the prefix planted at base 20
    and every fourth its reverse complement at base 90 (more occur by chance)."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        seq = bytearray(rng.choice(b"ACGT") for _ in range(SEQ))
        if i % 3 == 0:
            seq[20:20 + len(prefix)] = prefix
        if i % 4 == 0:
            seq[90:90 + len(prefix)] = revcomp(prefix)
        out.append(read(i, bytes(seq)))
    return b"".join(out)


def windows(data, prefix, k):
    """Windows that the line-index rule accepts, by a plain model: on every
    line with index 1 mod 4, the prefix at s with s + k <= |line|, and its
    reverse complement ending at e with e >= k."""
    rc, n = revcomp(prefix), 0
    for li, line in enumerate(data.split(b"\n")):
        if li % 4 != 1:
            continue
        for s in range(len(line) - len(prefix) + 1):
            if line.startswith(prefix, s) and s + k <= len(line):
                n += 1
            if line.startswith(rc, s) and s + len(prefix) >= k:
                n += 1
    return n
