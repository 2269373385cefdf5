"""The read filter's entry points (kmer_table_filter / kmer_table_filter_device)
are exported, listed, prototyped and bound; the ctypes mirrors of
kmer_filter_params and kmer_filter_result and Python's constants agree with
include/kmer_api.h; and the parameter checks answer before anything is
dereferenced (no GPU needed: a fake context pointer is never read)."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "kmer_api.h")
NAMES = ("kmer_table_filter_device", "kmer_table_filter")
BAD_PARAM = 2
CTYPES = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}


def _header():
    with open(HEADER) as f:
        return f.read()


def _members(struct):
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % struct, _header())
    assert m, struct
    out = []
    for decl in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        out += [(x.strip(), CTYPES[typ]) for x in names.split(",")]
    return out


def test_symbols_are_exported_listed_prototyped_and_bound():
    from kmerjs_amd import _native
    for name in NAMES:
        assert name in _native.EXPORTS
        f = getattr(_native.LIB, name)
        assert f.restype is ctypes.c_int and f.argtypes is not None and len(f.argtypes) == 9
        assert re.search(r"kmer_status\s+%s\s*\(" % name, _header())
    assert callable(_native.Counter.table_filter_device) and callable(_native.Counter.table_filter)


def test_structs_mirror_the_header():
    from kmerjs_amd import _native
    want = _members("kmer_filter_params")
    assert [n for n, _ in want] == ["min_count", "min_hits", "frac_num", "frac_den", "flags", "screen_flags"]
    assert list(_native.FilterParams._fields_) == want
    assert ctypes.sizeof(_native.FilterParams) == 32
    want = _members("kmer_filter_result")
    assert [n for n, _ in want] == ["n_reads", "n_kept", "out_len", "consumed"]
    assert list(_native.FilterResult._fields_) == want
    assert ctypes.sizeof(_native.FilterResult) == 32


def test_constants_equal_the_headers():
    from kmerjs_amd import _native
    h = _header()
    for name in ("DROP", "PAIRED"):
        m = re.search(r"KMER_FILTER_%s\s*=\s*(\d+)u?" % name, h)
        assert m and int(m.group(1)) == getattr(_native, "FILTER_" + name), name
    assert (_native.FILTER_DROP, _native.FILTER_PAIRED) == (1, 2)


def test_bad_calls_are_refused_before_the_context_is_read():
    from kmerjs_amd import _native
    L = _native.LIB
    fake = ctypes.c_void_p(0x10)                 # never dereferenced: every call below fails its parameter check
    data = b"@r\nACGT\n+\nIIII\n"
    dptr = ctypes.c_void_p(0x100)
    obuf, kbuf = (ctypes.c_uint8 * 64)(), (ctypes.c_uint8 * 4)()

    def params(num=0, den=1, flags=0, screen_flags=0):
        return _native.FilterParams(1, 1, num, den, flags, screen_flags)

    def device(ctx, ptr, n, p, want_res=True):
        outs = [ctypes.c_void_p(0x1234) for _ in range(3)]
        res = _native.FilterResult(7, 7, 7, 7)
        st = L.kmer_table_filter_device(ctx, ptr, n, ctypes.byref(p) if p is not None else None, None,
                                        *[ctypes.byref(o) for o in outs], ctypes.byref(res) if want_res else None)
        assert all(o.value is None for o in outs)
        if want_res:
            assert (res.n_reads, res.n_kept, res.out_len, res.consumed) == (0, 0, 0, 0)
        return st

    def host(ctx, buf, n, p, out=obuf, out_cap=64, keep=kbuf, keep_cap=4, want_res=True):
        res = _native.FilterResult(7, 7, 7, 7)
        st = L.kmer_table_filter(ctx, buf, n, ctypes.byref(p) if p is not None else None, out, out_cap, keep, keep_cap,
                                 ctypes.byref(res) if want_res else None)
        if want_res:
            assert (res.n_reads, res.n_kept, res.out_len, res.consumed) == (0, 0, 0, 0)
        return st

    ok = params()
    assert device(None, dptr, 16, ok) == BAD_PARAM
    assert device(fake, dptr, 16, None) == BAD_PARAM
    assert device(fake, dptr, 16, ok, want_res=False) == BAD_PARAM
    assert device(fake, None, 16, ok) == BAD_PARAM                      # NULL bytes with len > 0
    assert host(None, data, len(data), ok) == BAD_PARAM
    assert host(fake, data, len(data), None) == BAD_PARAM
    assert host(fake, data, len(data), ok, want_res=False) == BAD_PARAM
    assert host(fake, None, 16, ok) == BAD_PARAM
    assert host(fake, data, len(data), ok, out=None) == BAD_PARAM      # room for 64 bytes, nowhere to put them
    assert host(fake, data, len(data), ok, keep=None) == BAD_PARAM
    both = _native.SCREEN_DIRECT | _native.SCREEN_SORTED
    bad = [params(den=0), params(num=1, den=0), params(num=2, den=1), params(num=0xFFFFFFFF, den=0xFFFFFFFE)]
    bad += [params(flags=f) for f in (4, 8, 1 << 16, 1 << 31, 0xFFFFFFFF)]
    bad += [params(screen_flags=f) for f in (both, both | _native.SCREEN_PIECE_TEST, 8, 1 << 31, 0xFFFFFFFF)]
    for p in bad:
        what = (p.frac_num, p.frac_den, p.flags, p.screen_flags)
        assert device(fake, dptr, 16, p) == BAD_PARAM, what
        assert host(fake, data, len(data), p) == BAD_PARAM, what
    assert not any(obuf) and not any(kbuf)
    # len == 0: KMER_OK, a zero result, nothing touched (not even the context)
    assert device(fake, None, 0, ok) == 0
    assert host(fake, None, 0, ok) == 0
    assert host(fake, None, 0, ok, out=None, out_cap=0, keep=None, keep_cap=0) == 0
