"""Benchmark of the read filter (kmer_table_filter_device, kmer_filter.hip) on
one MI355X.  Run by hand; not part of bench.py.

Table: the C3 configuration (synthetic 150-bp reads, k = 31, no prefix,
KMER_FLAG_UNORDERED) built from --table-reads reads of seed 3.
Screened: --screen-reads records of 317 bytes; a record is either a read of
the table's range (it matches: every window hits) or a read of another seed
(it does not).  Kept shares of about 1 %, 50 % and 99 %, each in a blocky
layout (all kept records first) and in an alternating one (kept and dropped
records interleaved as evenly as the share allows).
Variants: the filter call (min_hits 1, frac 0/1); the only earlier route --
kmer_table_screen_device, a torch mask on the rows, the records' extents from
the '\\n' positions, and a torch per-byte gather on the device, the index
construction included in its time; and kmer_table_screen_device alone.
Timing: HIP events on the caller's stream around each whole call; one warm-up,
then --repeats calls, median with min-max.  Numbers from one box.
"filter - screen" is the cost of mark, segments and copy; it is set against a
device-to-device copy of out_len bytes timed in the same run (the practical
floor of the copy) and against 2 x out_len over the 8 TB/s HBM peak.
Required: the outputs of the filter and of the earlier route are equal
(asserted).  Writes a markdown table and the JSON rows to --out
(profiles/table_filter.md).
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
REC = 317                                     # bytes per synthetic record


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


def layout(m, share, blocky):
    """Which of m records match: about share of them, in one block or spread evenly."""
    n_keep = int(round(m * share))
    if blocky:
        return np.arange(m) < n_keep
    return np.floor((np.arange(m) + 1) * share) > np.floor(np.arange(m) * share)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table-reads", type=int, default=200_000)
    ap.add_argument("--screen-reads", type=int, default=1_000_000)
    ap.add_argument("--shares", type=float, nargs="*", default=[0.01, 0.5, 0.99])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "table_filter.md"))
    args = ap.parse_args()

    import torch
    from kmerjs_amd import _native as native
    from kmerjs_amd import synth_fastq_device
    from kmerjs_amd.multi import _CudaArray, device_u64

    assert torch.cuda.is_available(), "bench_table_filter needs a GPU"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    n, m = args.table_reads, args.screen_reads
    tab = torch.empty(n * REC, dtype=torch.uint8, device=dev)
    synth_fastq_device(tab.data_ptr(), 3, 0, n)
    torch.cuda.synchronize()
    ctr = native.Counter(k=K, prefix=b"", flags=native.FLAG_UNORDERED)
    ctr.reset()
    ctr.feed_device(tab.data_ptr(), tab.numel())
    ctr.finish(want_result=False)
    del tab
    # the two sources, record by record: reads of the table's range (cyclically), and reads of another seed
    yes = torch.empty((n, REC), dtype=torch.uint8, device=dev)
    synth_fastq_device(yes.data_ptr(), 3, 0, n)
    no = torch.empty((m, REC), dtype=torch.uint8, device=dev)
    synth_fastq_device(no.data_ptr(), 9, 0, m)
    torch.cuda.synchronize()
    yes = yes[torch.arange(m, device=dev) % n]
    scratch = torch.empty(m * REC, dtype=torch.uint8, device=dev)
    rows = []
    for share in args.shares:
        for blocky in (True, False):
            mask = torch.from_numpy(layout(m, share, blocky)).to(dev)
            buf = torch.where(mask[:, None], yes, no).reshape(-1).contiguous()
            torch.cuda.synchronize()

            def screen():
                ptr, nr = ctr.table_screen_device(buf.data_ptr(), buf.numel(), 1, 0, stream)
                assert nr == m
                return device_u64(ptr, 4 * nr, dev).view(nr, 4)

            def filt():
                d_out, d_keep, d_rows, res = ctr.table_filter_device(buf.data_ptr(), buf.numel(), stream=stream)
                assert res.n_reads == m and res.consumed == buf.numel()
                return torch.as_tensor(_CudaArray(d_out, res.out_len, "|u1"), device=dev) if res.out_len else buf[:0]

            def route():
                keep = screen()[:, 1] >= 1
                nl = (buf == 10).nonzero().view(-1)
                ends = nl[3::4] + 1                                           # (every record here ends in '\n')
                lens = ends - torch.cat([ends.new_zeros(1), ends[:-1]])
                return buf[torch.repeat_interleave(keep, lens)]

            res = {}
            for name, f in (("filter", filt), ("screen + torch gather", route), ("screen alone", screen)):
                res[name] = timed(f, args.repeats)
                print("share %.2f %s: %s %.2f ms" % (share, "blocky" if blocky else "alternating", name, res[name][1]),
                      flush=True)
            out = res["filter"][0]
            out_len = int(out.numel())
            assert torch.equal(res["screen + torch gather"][0], filt()), "the outputs differ"
            assert out_len == int(mask.sum().item()) * REC
            _, cp_med, cp_lo, cp_hi = timed(lambda: scratch[:out_len].copy_(buf[:out_len]), args.repeats)
            extra = res["filter"][1] - res["screen alone"][1]
            row = {"share": share, "layout": "blocky" if blocky else "alternating", "screened_reads": m,
                   "input_bytes": int(buf.numel()), "n_kept": out_len // REC, "out_len": out_len,
                   "repeats": args.repeats, "memcpy_ms": cp_med, "memcpy_ms_min": cp_lo, "memcpy_ms_max": cp_hi,
                   "hbm_floor_ms": 2 * out_len / HBM_BPS * 1e3, "filter_minus_screen_ms": extra}
            for name in res:
                key = name.replace(" + ", "_").replace(" ", "_")
                row[key + "_ms"], row[key + "_ms_min"], row[key + "_ms_max"] = res[name][1:]
            print(json.dumps(row), flush=True)
            rows.append(row)
            del buf
    ctr.close()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# Read filter: kept records compacted on the device (tools/bench_table_filter.py)\n\n")
        f.write("C3 configuration (k 31, no prefix, unordered), a table of %d reads, %d screened records of %d bytes "
                "(%.0f MB), one MI355X, HIP events around each whole call, 1 warm-up + %d calls, median (min-max).  "
                "min_hits 1, frac 0/1.  \"filter - screen\" = mark + segments + copy (medians subtracted); memcpy = a "
                "device-to-device copy of out_len bytes timed in the same run; HBM floor = 2 x out_len at 8 TB/s.  "
                "The filter's output equalled the earlier route's in every row.\n\n"
                % (n, m, REC, m * REC / 1e6, args.repeats))
        f.write("| kept | layout | out MB | filter ms | screen + torch gather ms | screen alone ms | filter - screen ms | "
                "memcpy ms | HBM floor ms | (filter - screen) / memcpy | route / filter |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %.0f %% | %s | %.1f | %.2f (%.2f-%.2f) | %.2f (%.2f-%.2f) | %.2f (%.2f-%.2f) | %.3f | "
                    "%.3f (%.3f-%.3f) | %.4f | %.1f | %.2f |\n" % (
                        100 * r["share"], r["layout"], r["out_len"] / 1e6,
                        r["filter_ms"], r["filter_ms_min"], r["filter_ms_max"],
                        r["screen_torch_gather_ms"], r["screen_torch_gather_ms_min"], r["screen_torch_gather_ms_max"],
                        r["screen_alone_ms"], r["screen_alone_ms_min"], r["screen_alone_ms_max"],
                        r["filter_minus_screen_ms"], r["memcpy_ms"], r["memcpy_ms_min"], r["memcpy_ms_max"],
                        r["hbm_floor_ms"], r["filter_minus_screen_ms"] / max(r["memcpy_ms"], 1e-9),
                        r["screen_torch_gather_ms"] / r["filter_ms"]))
        f.write("\n```json\n")
        for r in rows:
            f.write(json.dumps(r) + "\n")
        f.write("```\n")


if __name__ == "__main__":
    main()
