"""Benchmark of the table's by-value readers (kmer_table_spectrum,
kmer_table_extract_device; kmer_abundance.hip) on one MI355X.  Not part of
bench.py.

Spectrum.  The comparison is kmer_table_digest on the same table in the same
process: existing code that streams the same entries once and does more
arithmetic per entry.  Tables: C5 (single-line FASTA contigs, --contig-bytes of
them, k = 21, canonical k-mers) and the C3 configuration (synthetic 150-bp
reads, k = 31, no prefix) at --c3-reads reads -- on both the spectrum takes its
no-decode path, and the target is spectrum <= 1.10 x digest.  Beside them,
without a target, the decode path: the C3 configuration at the first
--c3-reads size with the prefix "A" and with k = 30 (an even k has palindromes).
Extract.  kmer_table_extract_device(lo=2) and (lo=1) at the first --c3-reads
size, whole calls; and at --baseline-reads reads next to the only route there
was before: kmer_finish_device(.., out) -- the whole Map to the host as sorted
strings -- plus a host filter of its counts.
Timing: each call between two HIP events on the caller's stream; every call
ends in a synchronise of the context's stream, so the events enclose the whole
call (kernels, launches, read-backs).  One warm-up call, then --repeats calls,
median and min-max reported.  Each spectrum is checked against
kmer_table_stats (sum hist = keys, sum v hist[v] + top_sum = total).
Prints one JSON line per measurement and writes them to --out.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, repeats):
    """ms of `repeats` calls of fn after one warm-up call, and the last call's value."""
    import torch
    out = fn()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms, out


def stat(ms):
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "repeats": len(ms)}


def emit(rows, row):
    print(json.dumps(row), flush=True)
    rows.append(row)


def bucket_lengths(ctr):
    import torch
    from kmerjs_amd.multi import _CudaArray
    dev = torch.device("cuda", torch.cuda.current_device())
    _, _, ln, _, n_big = ctr.table_device()
    nd = torch.as_tensor(_CudaArray(ln, 1 << 20, "<i4"), device=dev).cpu().numpy().astype(np.int64)
    return nd, n_big


def run_spectrum(name, ctr, path, nbins, repeats, rows):
    canon, keys, total = ctr.table_stats()
    nd, n_big = bucket_lengths(ctr)
    base = {"table": name, "k": ctr.k, "path": path, "table_entries": int(canon), "map_keys": int(keys), "n_big": int(n_big),
            "bucket_mean": float(nd.mean()), "bucket_max": int(nd.max()), "table_bytes": int(8 * canon)}
    dms, _ = timed(ctr.table_digest, repeats)
    sms, (hist, top) = timed(lambda: ctr.table_spectrum(nbins), repeats)
    assert int(hist.sum()) == keys, "sum of the spectrum != distinct Map keys"
    v = np.arange(nbins - 1, dtype=np.uint64)
    assert int((v * hist[:-1]).sum(dtype=np.uint64)) + top == total, "sum of v hist[v] != sum of the Map's counts"
    d, s = stat(dms), stat(sms)
    ratio = s["ms_median"] / d["ms_median"]
    emit(rows, dict(base, call="kmer_table_digest", **d, bytes_per_s=8 * canon / (d["ms_median"] / 1e3)))
    emit(rows, dict(base, call="kmer_table_spectrum", nbins=nbins, **s, bytes_per_s=8 * canon / (s["ms_median"] / 1e3),
                    spectrum_over_digest=ratio, target=1.10 if path == "no decode" else None,
                    met=bool(ratio <= 1.10) if path == "no decode" else None,
                    spectrum_head=[int(x) for x in hist[:8]]))


def run_extract(name, ctr, repeats, rows):
    canon, keys, total = ctr.table_stats()
    for lo in (2, 1):
        ms, (_, _, n) = timed(lambda: ctr.table_extract_device(lo, 0), repeats)
        emit(rows, dict(table=name, k=ctr.k, call="kmer_table_extract_device", lo=lo, keys_out=int(n), map_keys=int(keys),
                        table_entries=int(canon), **stat(ms)))


def c3_table(native, reads, k=31, prefix=b""):
    import torch
    from kmerjs_amd import synth_fastq_device
    dev = torch.device("cuda", 0)
    buf = torch.empty(reads * 317, dtype=torch.uint8, device=dev)
    synth_fastq_device(buf.data_ptr(), 3, 0, reads)
    torch.cuda.synchronize()
    ctr = native.Counter(k=k, prefix=prefix, flags=native.FLAG_UNORDERED)
    ctr.reset()
    ctr.feed_device(buf.data_ptr(), buf.numel())
    ctr.finish(want_result=False)
    return ctr, buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contig-bytes", type=int, default=1_000_000_000)
    ap.add_argument("--c3-reads", type=int, nargs="*", default=[2_000_000, 20_000_000])
    ap.add_argument("--baseline-reads", type=int, default=100_000,
                    help="reads of the table whose extract is timed next to finish(out) + a host filter (0: skip)")
    ap.add_argument("--nbins", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-c5", action="store_true")
    ap.add_argument("--skip-decode", action="store_true")
    ap.add_argument("--skip-extract", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()

    import torch
    from bench import make_contigs
    from kmerjs_amd import _native as native

    assert torch.cuda.is_available(), "bench_table_abundance needs a GPU"
    dev = torch.device("cuda", 0)
    rows = []
    if not args.skip_c5:
        k = 21
        data, _ = make_contigs(5, args.contig_bytes, k)
        buf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
        ctr = native.Counter(k=k, prefix=b"", flags=native.FLAG_CANONICAL)
        ctr.reset()
        ctr.feed_device(buf.data_ptr(), buf.numel())
        ctr.finish(want_result=False)
        del buf
        run_spectrum("C5 contigs %.2f GB, canonical" % (len(data) / 1e9), ctr, "no decode", args.nbins, args.repeats, rows)
        ctr.close()
        del data
    for i, reads in enumerate(args.c3_reads):
        ctr, buf = c3_table(native, reads)
        del buf
        name = "C3 configuration, %d reads" % reads
        run_spectrum(name, ctr, "no decode", args.nbins, args.repeats, rows)
        if i == 0 and not args.skip_extract:
            run_extract(name, ctr, args.repeats, rows)
        ctr.close()
    if args.c3_reads and not args.skip_decode:
        reads = args.c3_reads[0]
        for k, prefix, what in ((31, b"A", "decode (prefix A)"), (30, b"", "decode (even k)")):
            ctr, buf = c3_table(native, reads, k, prefix)
            del buf
            run_spectrum("C3 configuration, %d reads, k %d, prefix '%s'" % (reads, k, prefix.decode()), ctr, what,
                         args.nbins, args.repeats, rows)
            ctr.close()
    if args.baseline_reads and not args.skip_extract:
        reads = args.baseline_reads
        name = "C3 configuration, %d reads" % reads
        ctr, buf = c3_table(native, reads)
        run_extract(name, ctr, args.repeats, rows)
        ctr.close()

        def whole_map():
            c = native.Counter(k=31, prefix=b"", flags=native.FLAG_UNORDERED)
            c.reset()
            c.feed_device(buf.data_ptr(), buf.numel())
            c.sync()
            return c
        ms = []
        for _ in range(3):                                      # the finish alone, to take off the rows below
            c = whole_map()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c.finish(want_result=False)
            c.table_stats()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
            c.close()
        emit(rows, dict(table=name, k=31, call="kmer_finish_device(NULL)", **stat(ms[1:])))
        for lo in (2, 1):
            ms = []
            kept = 0
            for _ in range(2):                                  # (one warm-up, one timed: the call takes seconds)
                c = whole_map()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                res = c.finish()                                # the count's finish included: it is part of the call
                sel = res.counts >= lo
                kept = int(sel.sum())
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
                c.close()
                del res
            emit(rows, dict(table=name, k=31, call="kmer_finish_device(out) + host filter", lo=lo, keys_out=kept,
                            ms_median=float(ms[-1]), ms_min=float(ms[-1]), ms_max=float(ms[-1]), repeats=1,
                            note="includes the table finish (pass 2 + final) of the count"))
        del buf
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
