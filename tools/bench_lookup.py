"""Benchmark of the batched table lookup (kmer_table_lookup_device,
kmer_lookup.hip) on one MI355X.  Not part of bench.py.

Tables: C5 (single-line FASTA contigs, --contig-bytes of them, k = 21,
canonical k-mers: buckets of ~480 entries at 1 GB) and the C3 configuration
(synthetic 150-bp reads, k = 31, no prefix) at --c3-reads reads (2 M: buckets
of ~230 entries; --c3-reads 100000000 is C3 itself, buckets of ~11.4 K, when
the box has the memory free).
Queries: 2^20 and 2^24 per table; half are present keys, sampled from the
input's own counted windows, half are random k-mers (absent: a full scan of
their bucket); in canonical mode both halves are turned to the smaller string
of their class, so that every query reaches its bucket.
Timing: the device call between two HIP events on the caller's stream (the
call ends in a synchronise of the context's stream, so the events enclose the
kernel, its launch and the 8-byte error read-back); one warm-up call per
shape, then --repeats calls, median and min-max reported.  Numbers from one
box; DESIGN.md §8 records a few percent box-to-box spread for this project.
Bytes: what the scan must read -- 8 nd[q] per query (its whole bucket) plus
the query's own 8 + k bytes -- and that over 8 TB/s.  A present key's scan
stops at its match, so it reads about half of this.
Prints one JSON line per (table, query size) and writes them to --out.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MUL = np.uint64(0x9E3779B97F4A7C15)
HBM_BPS = 8e12


def planar(keys):
    """Planar codes (include/kmer_api.h, kmer_table_device) of an (n, k) array of A/C/G/T bytes."""
    k = keys.shape[1]
    lo = np.zeros(len(keys), dtype=np.uint64)
    hi = np.zeros(len(keys), dtype=np.uint64)
    for j in range(k):
        ch = keys[:, j].astype(np.uint64)
        lo |= (((ch >> np.uint64(1)) ^ (ch >> np.uint64(2))) & np.uint64(1)) << np.uint64(j)
        hi |= ((ch >> np.uint64(2)) & np.uint64(1)) << np.uint64(j)
    return (hi << np.uint64(k)) | lo


def revcomp(keys):
    lut = np.arange(256, dtype=np.uint8)
    for a, b in (b"AT", b"TA", b"CG", b"GC"):
        lut[a] = b
    return lut[keys[:, ::-1]]


def buckets(keys):
    """Bucket q of every key's class (the header's two encodings: k >= 22 and k <= 21)."""
    k = keys.shape[1]
    cf, cr = planar(keys), planar(revcomp(keys))
    with np.errstate(over="ignore"):
        if k >= 22:
            h = np.minimum(cf, cr) * MUL
        else:
            if k % 2 == 0:
                c = np.minimum(cf, cr)
            else:
                pos = np.uint64(k + (k - 1) // 2)
                c = np.where((cf >> pos) & np.uint64(1), cr, cf)
                c = ((c >> (pos + np.uint64(1))) << pos) | (c & ((np.uint64(1) << pos) - np.uint64(1)))
            h = ((c ^ (c >> np.uint64(21))) * MUL) << np.uint64(23)
    return (h >> np.uint64(44)).astype(np.int64)


def smaller_string(keys):
    """Each key or its reverse complement, whichever is the smaller string."""
    r = revcomp(keys)
    d = keys != r
    first = np.argmax(d, axis=1)
    rows = np.arange(len(keys))
    take_r = d.any(axis=1) & (r[rows, first] < keys[rows, first])
    out = keys.copy()
    out[take_r] = r[take_r]
    return out


def sample_windows(host, starts, lens, k, n, rng):
    """n windows of k bytes from the counted lines (start, length) of the input."""
    ok = lens >= k
    starts, lens = starts[ok], lens[ok]
    w = (lens - k + 1).astype(np.float64)
    line = rng.choice(len(starts), size=n, p=w / w.sum())
    pos = starts[line] + (rng.random(n) * (lens[line] - k + 1)).astype(np.int64)
    out = np.empty((n, k), dtype=np.uint8)
    for j in range(k):                                  # (column by column: no n x k 64-bit index)
        out[:, j] = host[pos + j]
    return out


def run_table(name, ctr, native, host, starts, lens, k, canonical, sizes, repeats, rng, rows):
    import torch
    from kmerjs_amd.multi import _CudaArray
    dev = torch.device("cuda", torch.cuda.current_device())
    canon_n, keys_n, total = ctr.table_stats()
    _, _, ln, _, n_big = ctr.table_device()
    nd = torch.as_tensor(_CudaArray(ln, 1 << 20, "<i4"), device=dev).cpu().numpy().astype(np.int64)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for n in sizes:
        present = sample_windows(host, starts, lens, k, n // 2, rng)
        absent = acgt[rng.integers(0, 4, (n - n // 2, k))]
        q = np.concatenate([present, absent])
        if canonical:
            q = smaller_string(q)
        q = q[rng.permutation(n)]
        scan_bytes = int(8 * nd[buckets(q)].sum()) + n * (8 + k)
        d_keys = torch.from_numpy(q.reshape(-1)).to(dev)
        d_cnt = torch.zeros(n, dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        ctr.table_lookup_device(d_keys.data_ptr(), n, d_cnt.data_ptr(), stream)      # warm-up
        ms = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ctr.table_lookup_device(d_keys.data_ptr(), n, d_cnt.data_ptr(), stream)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        found = int((d_cnt != 0).sum().item())
        med = float(np.median(ms))
        row = {"table": name, "k": k, "canonical": bool(canonical), "table_entries": int(canon_n), "n_big": int(n_big),
               "bucket_mean": float(nd.mean()), "bucket_max": int(nd.max()), "queries": n, "found": found,
               "ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)), "repeats": repeats,
               "queries_per_s": n / (med / 1e3), "scan_bytes": scan_bytes,
               "scan_bytes_per_s": scan_bytes / (med / 1e3), "fraction_of_8TBps": scan_bytes / (med / 1e3) / HBM_BPS}
        assert found >= n // 2, "sampled windows must be present"
        print(json.dumps(row), flush=True)
        rows.append(row)
        del d_keys, d_cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contig-bytes", type=int, default=1_000_000_000)
    ap.add_argument("--c3-reads", type=int, nargs="*", default=[2_000_000])
    ap.add_argument("--sizes", type=int, nargs="*", default=[1 << 20, 1 << 24])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-c5", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()

    import torch
    from bench import make_contigs
    from kmerjs_amd import _native as native
    from kmerjs_amd import synth_fastq_device

    assert torch.cuda.is_available(), "bench_lookup needs a GPU"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    rows = []
    if not args.skip_c5:
        k = 21
        data, lens = make_contigs(5, args.contig_bytes, k)
        host = np.frombuffer(data, dtype=np.uint8)
        ll = np.array(lens, dtype=np.int64)
        st = np.concatenate([[0], np.cumsum(ll + 1)[:-1]])
        counted = np.arange(len(ll)) % 4 == 1           # (the reference counts lines with index % 4 == 1)
        buf = torch.from_numpy(host.copy()).to(dev)
        ctr = native.Counter(k=k, prefix=b"", flags=native.FLAG_CANONICAL)
        ctr.reset()
        ctr.feed_device(buf.data_ptr(), buf.numel())
        ctr.finish(want_result=False)
        del buf
        run_table("C5 contigs %.2f GB" % (len(data) / 1e9), ctr, native, host, st[counted], ll[counted], k, True,
                  args.sizes, args.repeats, rng, rows)
        ctr.close()
        del data, host
    for reads in args.c3_reads:
        k = 31
        buf = torch.empty(reads * 317, dtype=torch.uint8, device=dev)
        synth_fastq_device(buf.data_ptr(), 3, 0, reads)
        torch.cuda.synchronize()
        ctr = native.Counter(k=k, prefix=b"", flags=native.FLAG_UNORDERED)
        ctr.reset()
        ctr.feed_device(buf.data_ptr(), buf.numel())
        ctr.finish(want_result=False)
        n_host = min(reads, 4_000_000)                  # windows are sampled from the first reads
        host = buf[:n_host * 317].cpu().numpy()
        del buf
        st = np.arange(n_host, dtype=np.int64) * 317 + 13
        run_table("C3 configuration, %d reads" % reads, ctr, native, host, st, np.full(n_host, 150, dtype=np.int64), k,
                  False, args.sizes, args.repeats, rng, rows)
        ctr.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
