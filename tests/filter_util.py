"""The read filter's definition (include/kmer_api.h, kmer_table_filter) as a
plain Python model: records from data.split(b"\\n"), the predicate in Python
integers, pairing, concatenation.  The rows it is applied to come from the
screen's models and oracle calls, never from the library's filter."""
FILTER_DROP, FILTER_PAIRED = 1, 2

_A, _B, _C = b"@a\nACGTA\n+\nIIIII\n", b"@b\nGG\n+\nII\n", b"@c\nTTT\n+\nIII\n"
# the edge inputs (test_filter_model.py states what each must give): name -> (bytes, records, consumed)
EDGE_INPUTS = {
    "empty": (b"", 0, 0),
    "no_newline": (b"@r0 ACGT", 0, 0),
    "nl1": (b"@a\n", 1, 3),
    "nl2": (b"@a\nACGTA\n", 1, 9),
    "nl3": (b"@a\nACGTA\n+\n", 1, 11),
    "nl4": (_A, 1, 17),
    "nl5": (_A + b"@b\n", 2, 20),
    "nl8": (_A + _B, 2, 28),
    "partial_header": (_A + _B + b"@c part", 2, 28),
    "no_final_newline": (_A + _B[:-1], 2, 27),
    "crlf": ((_A + _B).replace(b"\n", b"\r\n"), 2, 36),
    "three": (_A + _B + _C, 3, 41),
}


def split_records(data):
    """The records of `data`, back to back from offset 0: record r is lines
    4r .. 4r + 3 with their '\\n'; the last one runs to the end of the input
    when the '\\n' that would end line 4r + 3 is missing."""
    parts = data.split(b"\n")
    n_nl = len(parts) - 1
    n = (n_nl - 1) // 4 + 1 if n_nl else 0                # as many as data.split(b"\n")[1::4] has reads
    recs = []
    for r in range(n):
        if 4 * r + 4 <= n_nl:
            recs.append(b"".join(line + b"\n" for line in parts[4 * r:4 * r + 4]))
        else:
            recs.append(b"\n".join(parts[4 * r:]))
    return recs


def match(windows, hits, min_hits, frac):
    return hits >= min_hits and hits * frac[1] >= frac[0] * windows


def keep_flags(rows, min_hits=1, frac=(0, 1), flags=0):
    """rows: per read (windows, hits, ...) -> a list of bools."""
    m = [match(int(row[0]), int(row[1]), min_hits, frac) for row in rows]
    if flags & FILTER_PAIRED:
        m = [m[r] or (m[r ^ 1] if (r ^ 1) < len(m) else False) for r in range(len(m))]
    return [x != bool(flags & FILTER_DROP) for x in m]


def filter_model(data, rows, min_hits=1, frac=(0, 1), flags=0):
    """-> (out bytes, keep list, {n_reads, n_kept, out_len, consumed})."""
    recs = split_records(data)
    assert len(recs) == len(rows) == len(data.split(b"\n")[1::4])
    keep = keep_flags(rows, min_hits, frac, flags)
    out = b"".join(rec for rec, k in zip(recs, keep) if k)
    res = {"n_reads": len(recs), "n_kept": sum(keep), "out_len": len(out), "consumed": sum(len(x) for x in recs)}
    return out, keep, res
