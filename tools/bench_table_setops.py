"""Benchmark of the calls that relate two tables (kmer_table_compare,
kmer_table_setop_device; kmer_setops.hip) on one MI355X.  Not part of bench.py.

Tables: the C3 configuration (synthetic 150-bp reads, k = 31, no prefix) at
--reads reads; A = reads [0, n), B = reads [n / 2, 3 n / 2) of one seed, so half
of each table's classes are in the other.
Per size, in one process:
  floor     kmer_table_digest(a) + kmer_table_digest(b): each one full read of
            a table (the streaming floor)
  route     kmer_table_extract_device(a, 1, 0) followed by
            kmer_table_lookup_device(b, ..) over its keys: what a caller could
            do before (sorts and decodes all of A, then scans B's bucket once
            per key)
  compare   kmer_table_compare(a, b, 1, 1)
  subtract  kmer_table_setop_device(a, b, SUBTRACT, 1, 1), and UNION likewise
  into      kmer_table_setop_into(a, b, SUBTRACT / UNION, 1, 1, dst): the same
            operations with a table as their result, checked against compare
            (keys, totals) and, for UNION, digest(dst) = digest(a) + digest(b)
Required: compare faster than route.  compare / floor is reported, not gated;
so is into against the device setop of the same operation (expected: clearly
below it) and against the floor.
A step that does not fit device memory is reported as such and skipped.
Timing: each call between two HIP events on the caller's stream; every call
ends in a synchronise of the context's stream, so the events enclose the whole
call.  One warm-up call, then --repeats calls, median and min-max reported.
compare is checked against kmer_table_stats (keys_a, total_a, keys_b, total_b)
and against the route's own answer (keys_both = the keys of A that B answers).
Prints one JSON line per measurement and writes them to --out.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.bench_table_abundance import bucket_lengths, emit, stat, timed  # noqa: E402


def table(native, first, reads, k=31):
    import torch
    from kmerjs_amd import synth_fastq_device
    buf = torch.empty(reads * 317, dtype=torch.uint8, device=torch.device("cuda", 0))
    synth_fastq_device(buf.data_ptr(), 3, first, reads)
    torch.cuda.synchronize()
    ctr = native.Counter(k=k, prefix=b"", flags=native.FLAG_UNORDERED)
    ctr.reset()
    ctr.feed_device(buf.data_ptr(), buf.numel())
    ctr.finish(want_result=False)
    del buf
    torch.cuda.empty_cache()
    return ctr


def run(native, reads, repeats, rows, skip_route=False, into_only=False):
    import torch
    a, b = table(native, 0, reads), table(native, reads // 2, reads)
    ca, ka, ta = a.table_stats()
    cb, kb, tb = b.table_stats()
    nd, _ = bucket_lengths(a)
    base = {"table": "C3 configuration, %d reads each, half shared" % reads, "k": a.k, "entries_a": int(ca),
            "entries_b": int(cb), "bucket_mean": float(nd.mean()), "bucket_max": int(nd.max()),
            "join_tile": native.JOIN_TILE}
    fms, _ = timed(lambda: (a.table_digest(), b.table_digest()), repeats)
    floor = stat(fms)
    emit(rows, dict(base, call="kmer_table_digest(a) + kmer_table_digest(b)", **floor,
                    bytes_per_s=8 * (ca + cb) / (floor["ms_median"] / 1e3)))
    cms, cmp = timed(lambda: a.table_compare(b), repeats)
    assert (cmp["keys_a"], cmp["total_a"], cmp["keys_b"], cmp["total_b"]) == (ka, ta, kb, tb), "compare != table_stats"
    c = stat(cms)
    route = None
    if not skip_route and not into_only:
        try:
            def existing():
                d_keys, _, n = a.table_extract_device(1, 0)
                out = torch.empty(n, dtype=torch.int64, device=torch.device("cuda", 0))
                b.table_lookup_device(d_keys, n, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
                return out
            rms, out = timed(existing, repeats)
            assert int((out != 0).sum()) == cmp["keys_both"], "the route's shared keys != compare's keys_both"
            del out
            route = stat(rms)
            emit(rows, dict(base, call="kmer_table_extract_device(a, 1, 0) + kmer_table_lookup_device(b)", **route))
        except (native.KmerError, torch.OutOfMemoryError) as e:
            emit(rows, dict(base, call="kmer_table_extract_device(a, 1, 0) + kmer_table_lookup_device(b)",
                            skipped="does not fit: %s" % str(e)[:120]))
        torch.cuda.empty_cache()
    emit(rows, dict(base, call="kmer_table_compare", **c, bytes_per_s=8 * (ca + cb) / (c["ms_median"] / 1e3),
                    compare_over_floor=c["ms_median"] / floor["ms_median"],
                    route_over_compare=route["ms_median"] / c["ms_median"] if route else None,
                    required="compare faster than the route", met=bool(c["ms_median"] < route["ms_median"]) if route else None,
                    jaccard=cmp["jaccard"], keys_both=cmp["keys_both"]))
    # the device setops (sorted key bytes with counts), then the same operations with a table as their
    # result (no sort, no decode) on the same tables: the device setop of the operation is the baseline
    base_ms = {}
    sizes = {"SUBTRACT": ka - cmp["keys_both"], "UNION": ka + kb - cmp["keys_both"]}
    ops = (("SUBTRACT", native.SETOP_SUBTRACT), ("UNION", native.SETOP_UNION))
    for name, op in ops:
        call = "kmer_table_setop_device(%s)" % name
        if into_only:
            continue
        try:
            sms, (_, _, n) = timed(lambda: a.table_setop_device(b, op), repeats)
            assert n == sizes[name], "|%s| != what compare gives" % name
            s = stat(sms)
            base_ms[name] = s["ms_median"]
            emit(rows, dict(base, call=call, keys_out=int(n), **s,
                            route_over_subtract=route["ms_median"] / s["ms_median"] if route and name == "SUBTRACT" else None))
        except native.KmerError as e:
            emit(rows, dict(base, call=call, skipped="does not fit: %s" % str(e)[:120]))
    dst = native.Counter(k=a.k, prefix=b"", flags=native.FLAG_UNORDERED)
    digest_ab = (a.table_digest() + b.table_digest()) & ((1 << 64) - 1)
    for name, op in ops:
        call = "kmer_table_setop_into(%s)" % name
        try:
            ims, (cd, kd, td) = timed(lambda: a.table_setop_into(b, op, dst), repeats)
        except native.KmerError as e:
            emit(rows, dict(base, call=call, skipped="does not fit: %s" % str(e)[:120]))
            continue
        assert kd == sizes[name], "keys of %s into != what compare gives" % name
        if name == "SUBTRACT":
            assert td == ta - cmp["shared_a"], "total of SUBTRACT into != total_a - shared_a"
        else:
            assert td == ta + tb, "total of UNION into != total_a + total_b"
            assert dst.table_digest() == digest_ab, "digest(UNION) != digest(a) + digest(b)"
        i = stat(ims)
        emit(rows, dict(base, call=call, entries_out=int(cd), keys_out=int(kd), **i,
                        into_over_floor=i["ms_median"] / floor["ms_median"],
                        setop_device_over_into=base_ms[name] / i["ms_median"] if name in base_ms else None,
                        expected="clearly below the device setop of the same operation",
                        met=bool(i["ms_median"] < base_ms[name]) if name in base_ms else None))
    dst.close()
    a.close()
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, nargs="*", default=[2_000_000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-route", action="store_true", help="leave out the extract + lookup route (memory)")
    ap.add_argument("--into-only", action="store_true",
                    help="floor, compare and kmer_table_setop_into only: no route, no device setops (memory)")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()

    import torch
    from kmerjs_amd import _native as native

    assert torch.cuda.is_available(), "bench_table_setops needs a GPU"
    rows = []
    for reads in args.reads:
        run(native, reads, args.repeats, rows, args.skip_route, args.into_only)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
