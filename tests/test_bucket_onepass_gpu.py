"""The bucket finish's one-pass partition (bucket_onepass_kernel: fixed bucket
regions, runs claimed with one atomicAdd per bucket and block) and its exact
fallback (a bucket past its region -> ERR_BKT_CAP -> the finish redone with
the counted kernels, where the result is first observed), and the packed
path's phase times from device clock stamps.  Every count is compared with the
oracle: exact entries in Map order (lib/kmers.js:76,95)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BKT_EPB = 4096          # ranks per partition block (kmer_kernels.hip)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def native():
    from kmerjs_amd import _native
    return _native


def _fastq(seqs):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))


def _one_hit_read(rng, suffix=None):
    """A read with exactly one window that starts with ATGAC, on either strand
    (none that starts with GTCAT read forward): one hit of k = 16."""
    while True:
        suf = suffix if suffix is not None else ACGT[rng.integers(0, 4, 11)].tobytes()
        s = b"CC" + ACGT[rng.integers(0, 4, 18)].tobytes() + b"ATGAC" + suf + b"CCCCCCCC"
        if s.count(b"ATGAC") == 1 and b"GTCAT" not in s:
            return s


def _one_hit_reads(seed, n):
    rng = np.random.default_rng(seed)
    return [_one_hit_read(rng) for _ in range(n)]


def _check(ctr, data, want, tag):
    from tests.util import first_diff
    got = ctr.count_buffer(data).entries()
    assert got == want, (tag, len(got), len(want), first_diff(got, want))


@pytest.mark.parametrize("n", [0, 1, BKT_EPB - 1, BKT_EPB, BKT_EPB + 1, 3 * BKT_EPB + 7])
def test_block_edges(native, n):
    """n hits exactly (one per read): an empty finish, one rank, a full block
    less one, a full block, one rank into the second block, several blocks."""
    from oracle import oracle
    seqs = _one_hit_reads(100 + n % 97, n) if n else [b"C" * 60] * 50
    data = _fastq(seqs)
    want = oracle.count_buffer(data, b"ATGAC", 16, 1)
    assert sum(c for _, c in want) == n
    ctr = native.Counter(k=16, prefix=b"ATGAC")
    try:
        _check(ctr, data, want, n)
        _check(ctr, data, want, (n, "again"))
    finally:
        ctr.close()


@pytest.fixture(scope="module")
def reads3000():
    from oracle import oracle
    return oracle.synth_fastq(5, 0, 3000)


@pytest.mark.parametrize("prefix,k", [(b"ATGAC", 6), (b"ATGAC", 12), (b"ATGAC", 13), (b"ATGAC", 16), (b"ATGAC", 17),
                                      (b"A", 8), (b"", 3)])
def test_bucket_counts(native, reads3000, prefix, k):
    """1 bucket (k 6, 12), 4 (k 13), 256 (k 16), 1024 (k 17: the widest bucket
    key); 'A' / k 8 and k 3 without a prefix reach the same finish from the
    dense path."""
    from oracle import oracle
    want = oracle.count_buffer(reads3000, prefix, k, 1)
    assert want
    ctr = native.Counter(k=k, prefix=prefix)
    try:
        _check(ctr, reads3000, want, (prefix, k))
    finally:
        ctr.close()


def _skewed(kind):
    rng = np.random.default_rng(17)
    one = _one_hit_read(rng)
    if kind == "identical":
        seqs = [one] * 20_000
    else:                                    # half the hits carry one key, half are random
        seqs = [one] * 10_000 + _one_hit_reads(18, 10_000)
        order = np.random.default_rng(19).permutation(len(seqs))
        seqs = [seqs[i] for i in order]
    return _fastq(seqs)


@pytest.fixture(scope="module", params=["identical", "half"])
def skewed(request):
    from oracle import oracle
    data = _skewed(request.param)
    want = oracle.count_buffer(data, b"ATGAC", 16, 1)
    n = sum(c for _, c in want)
    # one bucket holds at least half of the n hits: far past the region of the
    # one-pass route (1.5 x the mean of 256 buckets + one block)
    assert n == 20_000 and max(c for _, c in want) >= 10_000 > math.ceil(n / 256) * 3 // 2 + BKT_EPB
    return data, want


def test_skew_takes_the_fallback_and_stays_exact(native, skewed):
    """A bucket past its region: the first count is redone on the counted
    route, the context stays on it; six counts on one Counter, each exact."""
    data, want = skewed
    ctr = native.Counter(k=16, prefix=b"ATGAC")
    try:
        for rep in range(6):
            _check(ctr, data, want, rep)
    finally:
        ctr.close()


def test_skew_fallback_at_observation(native, skewed):
    """The asynchronous finish (no host result): the overflow is seen, and the
    finish redone, when result_device() first observes the result."""
    import torch
    from kmerjs_amd.multi import device_u64
    data, want = skewed
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    ctr = native.Counter(k=16, prefix=b"ATGAC")
    try:
        ctr.reset()
        ctr.feed_device(buf.data_ptr(), buf.numel())
        ctr.finish(want_result=False)
        d_keys, d_counts, _, n = ctr.result_device()
        assert n == len(want)
        keys = device_u64(d_keys, 2 * n, buf.device).cpu().numpy().tobytes()     # (k = 16: two words per key)
        counts = device_u64(d_counts, n, buf.device).cpu().numpy().tolist()
        assert keys == b"".join(k for k, _ in want) and counts == [c for _, c in want]
    finally:
        ctr.close()


def test_uniform_count_after_a_skewed_one(native, skewed, reads3000):
    """No cursor or error bit of a fallback leaks: a uniform count on a fresh
    Counter in the same process, and on the Counter that fell back, is exact."""
    from oracle import oracle
    data, _ = skewed
    want = oracle.count_buffer(reads3000, b"ATGAC", 16, 1)
    old = native.Counter(k=16, prefix=b"ATGAC")
    try:
        old.count_buffer(data)
        fresh = native.Counter(k=16, prefix=b"ATGAC")
        try:
            _check(fresh, reads3000, want, "fresh")
            _check(fresh, reads3000, want, "fresh again")
        finally:
            fresh.close()
        _check(old, reads3000, want, "old")
    finally:
        old.close()


@pytest.mark.parametrize("batch", [4096, 1 << 20])
def test_multi_chunk_sessions(native, batch):
    """Chunks whose ranks start past 0 (out_base > 0), and tiles that overflow
    their hit slots (reads of ATGAC repeats: the long-segment and overflow
    paths), into the same finish."""
    from oracle import oracle
    rng = np.random.default_rng(23)
    dense = [(b"ATGAC" * 30)[:150]] * 600 + [(b"ATGAC" * 15 + b"GTCAT" * 15)[:150]] * 600
    inputs = [oracle.synth_fastq(9, 0, 6000),
              _fastq(dense + [ACGT[rng.integers(0, 4, 150)].tobytes() for _ in range(2000)])]
    ctr = native.Counter(k=16, prefix=b"ATGAC", batch_bytes=batch)
    try:
        for i, data in enumerate(inputs):
            _check(ctr, data, oracle.count_buffer(data, b"ATGAC", 16, 1), (batch, i))
    finally:
        ctr.close()


def test_phase_times_from_stamps(native):
    """scan <= feed (the scan is a part of the chunk), every time finite and
    positive, after one count of 100,000 synthetic reads."""
    import torch
    from kmerjs_amd import synth_fastq_device
    n = 100_000
    buf = torch.empty(n * 317, dtype=torch.uint8, device="cuda:0")
    synth_fastq_device(buf.data_ptr(), 1, 0, n)
    torch.cuda.synchronize()
    ctr = native.Counter(k=16, prefix=b"ATGAC")
    try:
        ctr.reset()
        ctr.feed_device(buf.data_ptr(), buf.numel())
        ctr.finish(want_result=False)
        scan, feed, fin = ctr.last_timing()
    finally:
        ctr.close()
    print("scan %.4f ms feed %.4f ms finish %.4f ms" % (scan, feed, fin))
    assert all(math.isfinite(x) for x in (scan, feed, fin))
    assert 0 < scan <= feed
    assert fin > 0
    assert feed < 1000 and fin < 1000          # (milliseconds of a 32 MB input, not clock ticks)
