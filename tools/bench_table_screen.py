"""Benchmark of the read screen (kmer_table_screen_device, kmer_screen.hip) on
one MI355X.  Run by hand; not part of bench.py.

Tables: the C3 configuration (synthetic 150-bp reads, k = 31, no prefix,
KMER_FLAG_UNORDERED) built from reads [0, n) for each n of --table-reads
(20 K, 200 K, 2 M: mean buckets ~2.3, ~23, ~229; more sizes place the
DIRECT / SORTED crossover behind KMER_SCREEN_DIRECT_MAX).
Screened: --screen-reads reads [n / 2, n / 2 + 1 M).
Variants: the screen with KMER_SCREEN_DIRECT, KMER_SCREEN_SORTED and auto (0),
and the only earlier route, built from what the library offered before the
screen: torch `unfold` of the sequence lines into n k key bytes,
kmer_table_lookup_device, a torch segment sum -- timed with the key
materialisation included, and run in pieces of --route-piece reads so that
the key bytes fit (31 x the sequence bytes).
Timing: HIP events on the caller's stream around each whole call; one warm-up,
then --repeats calls, median with min-max.  Numbers from one box.
Floor: one read of the input, its bytes over the 8 TB/s HBM peak.
Required: rows equal between every variant at the timed sizes (asserted).
Writes a markdown table and the JSON rows to --out (profiles/table_screen.md).
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_BPS = 8e12
K = 31
REC, SEQ0, SEQ = 317, 13, 150                 # bytes per synthetic record, offset and length of its sequence line


def timed(f, repeats):
    import torch
    out = f()                                 # warm-up
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = f()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table-reads", type=int, nargs="*", default=[20_000, 200_000, 2_000_000])
    ap.add_argument("--screen-reads", type=int, default=1_000_000)
    ap.add_argument("--route-piece", type=int, default=250_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-count", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "table_screen.md"))
    args = ap.parse_args()

    import torch
    from kmerjs_amd import _native as native
    from kmerjs_amd import synth_fastq_device
    from kmerjs_amd.multi import _CudaArray, device_u64

    assert torch.cuda.is_available(), "bench_table_screen needs a GPU"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    m, mc = args.screen_reads, args.min_count
    W = SEQ - K + 1
    rows, slower = [], []
    for n in args.table_reads:
        tab = torch.empty(n * REC, dtype=torch.uint8, device=dev)
        synth_fastq_device(tab.data_ptr(), 3, 0, n)
        torch.cuda.synchronize()
        ctr = native.Counter(k=K, prefix=b"", flags=native.FLAG_UNORDERED)
        ctr.reset()
        ctr.feed_device(tab.data_ptr(), tab.numel())
        ctr.finish(want_result=False)
        del tab
        entries = ctr.table_stats()[0]
        _, _, ln, _, _ = ctr.table_device()
        nd = torch.as_tensor(_CudaArray(ln, 1 << 20, "<i4"), device=dev)
        bucket_mean, bucket_max = float(nd.float().mean().item()), int(nd.max().item())
        buf = torch.empty(m * REC, dtype=torch.uint8, device=dev)
        synth_fastq_device(buf.data_ptr(), 3, n // 2, m)
        torch.cuda.synchronize()

        def screen(flags):
            ptr, nr = ctr.table_screen_device(buf.data_ptr(), buf.numel(), mc, flags, stream)
            assert nr == m
            return device_u64(ptr, 4 * nr, dev).view(nr, 4).clone()

        def route():
            # table mode, no prefix, odd k: both orientations of every window are keys (weight 2), none is its own rc
            out = torch.empty((m, 4), dtype=torch.int64, device=dev)
            seq = buf.view(m, REC)[:, SEQ0:SEQ0 + SEQ]
            for r0 in range(0, m, args.route_piece):
                r1 = min(m, r0 + args.route_piece)
                keys = seq[r0:r1].unfold(1, K, 1).contiguous()                   # (reads, W, K): n k key bytes
                cnt = torch.empty((r1 - r0) * W, dtype=torch.int64, device=dev)
                ctr.table_lookup_device(keys.data_ptr(), cnt.numel(), cnt.data_ptr(), stream)
                cnt = cnt.view(r1 - r0, W)
                hit = cnt >= mc
                out[r0:r1, 0] = 2 * W
                out[r0:r1, 1] = 2 * hit.sum(dim=1)
                out[r0:r1, 2] = 0
                out[r0:r1, 3] = 2 * (cnt * hit).sum(dim=1)
            return out

        res = {}
        for name, f in (("direct", lambda: screen(native.SCREEN_DIRECT)), ("sorted", lambda: screen(native.SCREEN_SORTED)),
                        ("auto", lambda: screen(0)), ("unfold+lookup", route)):
            res[name] = timed(f, args.repeats)
            print("table %d reads: %s %.2f ms" % (n, name, res[name][1]), flush=True)
        ref = res["direct"][0]
        for name in res:
            assert torch.equal(res[name][0], ref), "rows differ: %s" % name
        floor_ms = buf.numel() / HBM_BPS * 1e3
        auto_route = "sorted" if entries > native.SCREEN_DIRECT_MAX * (1 << 20) else "direct"
        for name in res:
            _, med, lo, hi = res[name]
            row = {"table_reads": n, "table_entries": int(entries), "bucket_mean": bucket_mean, "bucket_max": bucket_max,
                   "screened_reads": m, "windows": m * W, "input_bytes": int(buf.numel()), "variant": name,
                   "auto_route": auto_route, "ms_median": med, "ms_min": lo, "ms_max": hi, "repeats": args.repeats,
                   "reads_per_s": m / (med / 1e3), "windows_per_s": m * W / (med / 1e3),
                   "route_over_this": res["unfold+lookup"][1] / med, "this_over_floor": med / floor_ms,
                   "floor_ms": floor_ms, "hit_reads": int((ref[:, 1] > 0).sum().item()),
                   "route_piece_reads": args.route_piece if name == "unfold+lookup" else None}
            print(json.dumps(row), flush=True)
            rows.append(row)
        if res["auto"][1] >= res["unfold+lookup"][1]:
            slower.append(n)
        ctr.close()
        del buf

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# Read screen against a finished table (tools/bench_table_screen.py)\n\n")
        f.write("C3 configuration (k 31, no prefix, unordered), one MI355X, HIP events around each whole call, "
                "1 warm-up + %d calls, median (min-max).  Screened: %d synthetic reads (%d windows, %.0f MB); "
                "floor = one read of the input at 8 TB/s.  The earlier route (unfold + kmer_table_lookup_device + "
                "segment sum) ran in pieces of %d reads.  Rows were equal between all variants.  "
                "KMER_SCREEN_DIRECT_MAX = %d.\n\n" % (args.repeats, m, m * W, m * REC / 1e6, args.route_piece,
                                                      native.SCREEN_DIRECT_MAX))
        f.write("| table reads | entries | mean bucket | variant | ms median (min-max) | reads/s | windows/s | "
                "route / this | this / floor |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            name = r["variant"] + (" (-> %s)" % r["auto_route"] if r["variant"] == "auto" else "")
            f.write("| %d | %d | %.2f | %s | %.2f (%.2f-%.2f) | %.3g | %.3g | %.2f | %.0f |\n" % (
                r["table_reads"], r["table_entries"], r["bucket_mean"], name, r["ms_median"], r["ms_min"], r["ms_max"],
                r["reads_per_s"], r["windows_per_s"], r["route_over_this"], r["this_over_floor"]))
        f.write("\nA full-size C3 table (100 M reads, mean bucket ~11.4 K) was not measured.\n\n```json\n")
        for r in rows:
            f.write(json.dumps(r) + "\n")
        f.write("```\n")
    if slower:
        sys.exit("auto is slower than the earlier route at table reads %s" % slower)


if __name__ == "__main__":
    main()
