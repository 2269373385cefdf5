"""Benchmark of the template DB built from FASTA genomes on the device
(kmer_db_open_fasta / kmer_db_open_fasta_device, kmer_dbfasta.hip) on one
MI355X.  Run by hand; not part of bench.py.

Input: --templates synthetic genomes of --bases random bases each (fixed
seed), line width 60, generated on the host.
Configurations: k 16 / ATGAC (the kmerFinder configuration: about one window
in a thousand emits) and k 21 / no prefix / canonical (every window emits).
Routes:
  device   kmer_db_open_fasta_device over the bytes in device memory, HIP
           events on the caller's stream around the whole call (DB build
           included);
  host     kmer_db_open_fasta over the bytes in host memory, wall clock;
  parent   what the library offered before: one KMER_FLAG_FASTA count per
           record, its A/C/G/T keys gathered on the host, then kmer_db_open --
           wall clock, --parent-repeats calls (it is the slow one).
One warm-up, then --repeats calls, median with min-max.  Numbers from one box.
Floor: one read of the input, its bytes over the 8 TB/s HBM peak.
Required before timing: the DBs of the new routes and of the parent route are
equal (info, entries per template, the distinct k-mers at both ends, the
k-mers of the first and last template).
Writes a markdown table and the JSON rows to --out (profiles/db_fasta.md).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_BPS = 8e12
WIDTH = 60
CONFIGS = [("k16-ATGAC", 16, b"ATGAC", 0), ("k21-canonical", 21, b"", 64)]


def make_genomes(n, bases, seed=1):
    """(the FASTA bytes, each record's start offset + the total)."""
    rng = np.random.default_rng(seed)
    lines = bases // WIDTH
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    parts, starts, pos = [], [], 0
    for t in range(n):
        body = np.empty((lines, WIDTH + 1), dtype=np.uint8)
        body[:, :WIDTH] = acgt[rng.integers(0, 4, (lines, WIDTH), dtype=np.uint8)]
        body[:, WIDTH] = 10
        rec = b">NC_%06d Genus species strain %d\n" % (t, t) + body.tobytes()
        starts.append(pos)
        pos += len(rec)
        parts.append(rec)
    return b"".join(parts), starts + [pos]


def timed_events(f, repeats):
    import torch
    f().close()                               # warm-up
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        db = f()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
        db.close()
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def timed_wall(f, repeats, warm=True):
    if warm:
        f().close()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        db = f()
        ms.append((time.perf_counter() - t0) * 1e3)
        db.close()
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def parent_route(native, kf, data, starts, k, prefix, flags):
    """One FASTA count per record, the A/C/G/T keys gathered on the host, kmer_db_open."""
    ctr = native.Counter(k=k, prefix=prefix, flags=flags | native.FLAG_FASTA)
    lut = np.zeros(256, dtype=bool)
    lut[list(b"ACGT")] = True
    blobs, tstart, meta = [], [0], []
    try:
        for t in range(len(starts) - 1):
            r = ctr.count_buffer(data[starts[t]:starts[t + 1]])
            off = r.offsets.astype(np.int64)
            assert len(off) < 2 or int(off[-1]) == (len(off) - 1) * k     # (step 1: every key has k bytes)
            keys = np.frombuffer(r.keybuf, dtype=np.uint8).reshape(-1, k)
            keep = lut[keys].all(axis=1)
            blobs.append(keys[keep].tobytes())
            tstart.append(tstart[-1] + int(keep.sum()))
            meta.append({"sequence": "NC_%06d" % t, "species": "", "lengths": int(r.counts[keep].sum()),
                         "ulength": int(keep.sum())})
    finally:
        ctr.close()
    return kf.TemplateDB.from_arrays(k, b"".join(blobs), np.asarray(tstart, dtype=np.uint64), meta,
                                     kf.default_summary(meta))


def same_db(a, b):
    ia, ib = a.info(), b.info()
    assert ia == ib, (ia, ib)
    assert a.template_stats()[1].tolist() == b.template_stats()[1].tolist()
    n = min(ia["distinct"], 1 << 16)
    assert a.kmers(0, n) == b.kmers(0, n) and a.kmers(ia["distinct"] - n, n) == b.kmers(ia["distinct"] - n, n)
    for t in (0, ia["templates"] - 1):
        assert a.template_kmers(t).tolist() == b.template_kmers(t).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--templates", type=int, default=2000)
    ap.add_argument("--bases", type=int, default=1_000_020)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-repeats", type=int, default=5)
    ap.add_argument("--configs", nargs="*", default=[c[0] for c in CONFIGS])
    ap.add_argument("--skip-parent", action="store_true", help="new routes only (for a kernel trace of them)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "db_fasta.md"))
    args = ap.parse_args()

    import torch
    from kmerjs_amd import _native as native, kmerfinder as kf

    data, starts = make_genomes(args.templates, args.bases)
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    floor_ms = len(data) / HBM_BPS * 1e3
    rows = []
    for name, k, prefix, flags in CONFIGS:
        if name not in args.configs:
            continue
        ctr = native.Counter(k=k, prefix=prefix, flags=flags)
        new_dev = lambda: kf.TemplateDB.from_fasta_device(ctr, dev.data_ptr(), len(data))     # noqa: E731
        new_host = lambda: kf.TemplateDB.from_fasta(ctr, data)                                # noqa: E731
        parent = lambda: parent_route(native, kf, data, starts, k, prefix, flags)             # noqa: E731
        a, b = new_dev(), new_host()
        same_db(a, b)
        if not args.skip_parent:
            c = parent()
            same_db(a, c)
            c.close()
        info = a.info()
        a.close(), b.close()
        res = {"device": timed_events(new_dev, args.repeats), "host": timed_wall(new_host, args.repeats)}
        if not args.skip_parent:                  # (the equality run was its warm-up)
            res["parent"] = timed_wall(parent, args.parent_repeats, warm=False)
        ctr.close()
        for route, (med, lo, hi) in res.items():
            rows.append({"config": name, "k": k, "prefix": prefix.decode(), "canonical": bool(flags & 64),
                         "templates": args.templates, "bases": args.bases, "input_bytes": len(data),
                         "distinct": info["distinct"], "entries": info["entries"], "route": route,
                         "ms_median": med, "ms_min": lo, "ms_max": hi,
                         "repeats": args.parent_repeats if route == "parent" else args.repeats,
                         "parent_over_this": res["parent"][0] / med if "parent" in res else None,
                         "this_over_floor": med / floor_ms,
                         "floor_ms": floor_ms, "input_gb_per_s": len(data) / med / 1e6})
            print(json.dumps(rows[-1]), flush=True)
    with open(args.out, "w") as f:
        f.write("# Template DB from FASTA genomes on the device (tools/bench_db_fasta.py)\n\n")
        f.write("%d synthetic genomes of %d bases (line width %d, %d MB of FASTA), one MI355X.  device: HIP events "
                "around each whole kmer_db_open_fasta_device call; host and parent: wall clock.  1 warm-up + %d calls "
                "(parent: %d), median (min-max).  floor = one read of the input at 8 TB/s.  The DBs of all routes "
                "were equal.\n\n" % (args.templates, args.bases, WIDTH, len(data) // 1_000_000, args.repeats,
                                     args.parent_repeats))
        f.write("| config | entries | route | ms median (min-max) | input GB/s | parent / this | this / floor |\n")
        f.write("|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %s | %d | %s | %.2f (%.2f-%.2f) | %.1f | %s | %.0f |\n" %
                    (r["config"], r["entries"], r["route"], r["ms_median"], r["ms_min"], r["ms_max"],
                     r["input_gb_per_s"], "%.2f" % r["parent_over_this"] if r["parent_over_this"] else "-",
                     r["this_over_floor"]))
        f.write("\n```json\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")


if __name__ == "__main__":
    main()
