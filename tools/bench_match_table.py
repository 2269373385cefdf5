"""Benchmark of template matching straight from a table-mode count
(kmer_match_open_table, kmer_probe.hip) on one MI355X.  Not part of bench.py.

Round 1 only (the winner loop is the same machinery for every open).  Routes,
interleaved per repeat on one box:
  table    kmer_match_open_table: the bucket-ordered probe + the shared tail
  simple   the composition the feature could have been, from the public
           calls: kmer_table_lookup_device over the DB's distinct k-mers in U
           order (their bytes decoded once, outside the timing), a compaction
           of the keys with a count > 0 (torch), kmer_match_open_device over
           them.  `simple_lookup_ms` is the lookup call alone: a lower bound
           of any route that scans one bucket per DB k-mer.
  ordered  shape (a) only: kmer_match_open_device over the ORDERED count of
           the same input (the query the matcher was built for)
Shapes:
  (a) the C2 input (10 M reads, k 16, ATGAC) counted in table mode against
      tools/bench_match.py's DB (5,030 x 3,285 k-mers).  The DB-order scores
      must equal those of the ordered route: asserted.
  (b) the C3 configuration (k 31, no prefix) at 2 M reads, (c) at 20 M reads:
      a DB of the same shape, half of each template windows sampled from the
      input, half random (absent) k-mers.
Timing: each call between two HIP events on the caller's stream (every call
ends in a synchronise of the stream it worked on, so the events enclose it);
one warm-up per route, then --repeats rounds, median and min-max reported.
Prints one JSON line per shape and writes them to --out.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def codes_to_bytes(codes, k):
    mat = np.empty((codes.size, k), dtype=np.uint8)
    for j in range(k):                                  # (column by column: no n x k 64-bit temporaries)
        mat[:, j] = ACGT[((codes >> np.uint64(2 * (k - 1 - j))) & np.uint64(3)).astype(np.uint8)]
    return mat


def bench_match_db(qc, k, nt, per, present):
    """The DB of tools/bench_match.py (same generator, same seed): key bytes (n, k)."""
    from tests.match_util import kmer_codes
    rng = np.random.default_rng(7)
    codes = kmer_codes(rng, nt * per * 2, k)
    allc = np.empty(nt * per, dtype=np.uint64)
    for t in range(nt):
        c = np.unique(codes[t * per * 2:(t + 1) * per * 2])[:per]
        if t < present:
            take = int(per * 0.6)
            c = np.unique(np.concatenate([rng.choice(qc, size=take, replace=False), c]))[:per]
        allc[t * per:(t + 1) * per] = c
    return codes_to_bytes(allc, k)


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def run_shape(name, ctr, k, keys, nt, per, repeats, ordered=None):
    """keys: the DB's k-mers (nt * per, k) uint8.  ordered: (d_keys, d_cnt, n) of the ordered count, shape (a)."""
    import torch
    from kmerjs_amd import kmerfinder as kf
    from kmerjs_amd.multi import _CudaArray
    dev = torch.device("cuda", torch.cuda.current_device())
    starts = np.arange(nt + 1, dtype=np.uint64) * np.uint64(per)
    meta = [{"sequence": "NC_%06d" % t, "lengths": 2 * per, "ulength": per, "species": "synthetic"} for t in range(nt)]
    db = kf.TemplateDB.from_arrays(k, keys.tobytes(), starts, meta,
                                   {"templates": nt, "totalLen": 2 * per * nt, "uniqueLens": per * nt})
    info = db.info()
    m = info["distinct"]
    _, _, ln, _, _ = ctr.table_device()
    nd = torch.as_tensor(_CudaArray(ln, 1 << 20, "<i4"), device=dev).cpu().numpy().astype(np.int64)
    stream = torch.cuda.current_stream().cuda_stream
    # the simple composition's inputs: U decoded to bytes, once
    ub = np.empty(max(m * k, 1), dtype=np.uint8)
    kf._check(kf.LIB.kmer_db_kmers(db.handle, 0, m, ub.ctypes.data_as(ctypes.c_void_p)), "kmer_db_kmers")
    ukeys = torch.from_numpy(ub[:m * k]).to(dev)
    del ub
    ucnt = torch.zeros(m, dtype=torch.int64, device=dev)

    def table_route():
        return kf.Match(db, table=ctr)

    def simple_route():
        t_lk, _ = timed(lambda: ctr.table_lookup_device(ukeys.data_ptr(), m, ucnt.data_ptr(), stream))
        keep = ucnt != 0
        qk = ukeys.view(m, k)[keep].contiguous()
        qn = ucnt[keep].contiguous()
        torch.cuda.synchronize()
        mt = kf.Match(db, device_result=(qk.data_ptr(), k, qn.data_ptr(), int(qk.shape[0])), stream=stream)
        return t_lk, mt

    def ordered_route():
        return kf.Match(db, device_result=(ordered[0], k, ordered[1], ordered[2]))

    table_route().close()                                # warm-ups
    simple_route()[1].close()
    if ordered:
        ordered_route().close()
    t_tab, t_simple, t_lookup, t_ord = [], [], [], []
    scores = {}
    for _ in range(repeats):                             # interleaved
        ms, mt = timed(table_route)
        t_tab.append(ms)
        scores["table"] = (mt.templates(1), int(mt.winner().hits))
        mt.close()
        ms, (lk, mt) = timed(simple_route)
        t_simple.append(ms)
        t_lookup.append(lk)
        scores["simple"] = (mt.templates(1), int(mt.winner().hits))
        mt.close()
        if ordered:
            ms, mt = timed(ordered_route)
            t_ord.append(ms)
            scores["ordered"] = (mt.templates(1), int(mt.winner().hits))
            mt.close()
    assert scores["table"] == scores["simple"], "the two table routes disagree"
    if ordered:
        assert scores["table"] == scores["ordered"], "table route and ordered route disagree on the DB-order scores"
    canon_n, keys_n, _ = ctr.table_stats()
    row = {"shape": name, "k": k, "table_entries": int(canon_n), "map_keys": int(keys_n),
           "bucket_mean": float(nd.mean()), "bucket_max": int(nd.max()),
           "db_templates": nt, "db_distinct": int(m), "db_entries": int(info["entries"]),
           "hits": scores["table"][1], "templates_hit": len(scores["table"][0]), "repeats": repeats,
           "table_ms": stats(t_tab), "simple_ms": stats(t_simple), "simple_lookup_ms": stats(t_lookup),
           "scores_equal_table_vs_simple": True}
    if ordered:
        row["ordered_ms"] = stats(t_ord)
        row["scores_equal_table_vs_ordered"] = True
    print(json.dumps(row), flush=True)
    db.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c2-reads", type=int, default=10_000_000, help="0: skip shape (a)")
    ap.add_argument("--c3-reads", type=int, nargs="*", default=[2_000_000, 20_000_000])
    ap.add_argument("--templates", type=int, default=5030)
    ap.add_argument("--per", type=int, default=3285)
    ap.add_argument("--present", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()

    import torch
    from bench_lookup import sample_windows
    from kmerjs_amd import _native as native
    from kmerjs_amd import synth_fastq_device
    from kmerjs_amd.multi import _CudaArray

    assert torch.cuda.is_available(), "bench_match_table needs a GPU"
    dev = torch.device("cuda", 0)
    nt, per = args.templates, args.per
    rows = []
    if args.c2_reads:
        k = 16
        buf = torch.empty(args.c2_reads * 317, dtype=torch.uint8, device=dev)
        synth_fastq_device(buf.data_ptr(), 1, 0, args.c2_reads)
        torch.cuda.synchronize()
        octr = native.Counter(k=k, prefix=b"ATGAC")
        octr.reset()
        octr.feed_device(buf.data_ptr(), buf.numel())
        octr.finish(want_result=False)
        d_keys, d_cnt, _, nq = octr.result_device()
        kt = torch.as_tensor(_CudaArray(d_keys, nq * k, "|u1"), device=dev).cpu().numpy().reshape(nq, k)
        lut = np.zeros(256, dtype=np.uint64)
        lut[ACGT] = np.arange(4, dtype=np.uint64)
        qc = np.zeros(nq, dtype=np.uint64)
        for i in range(k):
            qc = (qc << np.uint64(2)) | lut[kt[:, i]]
        keys = bench_match_db(qc, k, nt, per, args.present)
        tctr = native.Counter(k=k, prefix=b"ATGAC", flags=native.FLAG_UNORDERED)
        tctr.reset()
        tctr.feed_device(buf.data_ptr(), buf.numel())
        tctr.finish(want_result=False)
        del buf
        assert tctr.table_stats()[1] == nq
        rows.append(run_shape("(a) C2, %d reads, k 16 ATGAC" % args.c2_reads, tctr, k, keys, nt, per, args.repeats,
                              ordered=(d_keys, d_cnt, nq)))
        tctr.close()
        octr.close()
        del keys
    for reads in args.c3_reads:
        k = 31
        rng = np.random.default_rng(reads)
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
        half = per // 2
        keys = ACGT[rng.integers(0, 4, (nt * per, k), dtype=np.uint8)]
        win = sample_windows(host, st, np.full(n_host, 150, dtype=np.int64), k, nt * half, rng)
        keys.reshape(nt, per, k)[:, :half, :] = win.reshape(nt, half, k)
        del win, host
        rows.append(run_shape("C3 configuration, %d reads, k 31" % reads, ctr, k, keys, nt, per, args.repeats))
        ctr.close()
        del keys
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
