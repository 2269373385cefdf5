"""The read screen's entry points (kmer_table_screen / kmer_table_screen_device)
are exported, listed, prototyped and bound; the ctypes mirror of
kmer_read_screen and Python's constants agree with include/kmer_api.h; and the
parameter checks answer before anything is dereferenced (no GPU needed: a fake
context pointer is never read)."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "kmer_api.h")
NAMES = ("kmer_table_screen_device", "kmer_table_screen")
BAD_PARAM = 2


def _header():
    with open(HEADER) as f:
        return f.read()


def test_symbols_are_exported_listed_prototyped_and_bound():
    from kmerjs_amd import _native
    for name in NAMES:
        assert name in _native.EXPORTS
        f = getattr(_native.LIB, name)
        assert f.restype is ctypes.c_int and f.argtypes is not None and len(f.argtypes) == 8
        assert re.search(r"kmer_status\s+%s\s*\(" % name, _header())
    assert callable(_native.Counter.table_screen_device) and callable(_native.Counter.table_screen)


def test_read_screen_mirrors_the_header_struct():
    from kmerjs_amd import _native
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*kmer_read_screen\s*;", _header())
    assert m
    members = []
    for decl in m.group(1).split(";"):
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S).strip()
        if not decl:
            continue
        assert decl.startswith("uint64_t"), decl
        members += [x.strip() for x in decl[len("uint64_t"):].split(",")]
    assert members == ["windows", "hits", "skipped", "sum"]
    assert [n for n, _ in _native.ReadScreen._fields_] == members
    assert all(t is ctypes.c_uint64 for _, t in _native.ReadScreen._fields_)
    assert ctypes.sizeof(_native.ReadScreen) == 32


def test_constants_equal_the_headers():
    from kmerjs_amd import _native
    h = _header()
    for name in ("DIRECT", "SORTED", "PIECE_TEST"):
        m = re.search(r"KMER_SCREEN_%s\s*=\s*(\d+)u?" % name, h)
        assert m and int(m.group(1)) == getattr(_native, "SCREEN_" + name), name
    m = re.search(r"#define\s+KMER_SCREEN_DIRECT_MAX\s+(\d+)u?", h)
    assert m and int(m.group(1)) == _native.SCREEN_DIRECT_MAX
    assert (_native.SCREEN_DIRECT, _native.SCREEN_SORTED, _native.SCREEN_PIECE_TEST) == (1, 2, 4)


def test_null_and_bad_flag_calls_are_refused_before_the_context_is_read():
    from kmerjs_amd import _native
    L = _native.LIB
    fake = ctypes.c_void_p(0x10)                 # never dereferenced: every call below fails its parameter check
    data = b"@r\nACGT\n+\nIIII\n"
    rows = (_native.ReadScreen * 4)()

    def device(ctx, ptr, n, flags, want_rows=True, want_n=True):
        d_rows, nr = ctypes.c_void_p(0x1234), ctypes.c_uint64(77)
        st = L.kmer_table_screen_device(ctx, ptr, n, 1, flags, None, ctypes.byref(d_rows) if want_rows else None,
                                        ctypes.byref(nr) if want_n else None)
        if want_rows:
            assert d_rows.value is None
        if want_n:
            assert nr.value == 0
        return st

    def host(ctx, buf, n, flags, out=rows, cap=4, want_n=True):
        nr = ctypes.c_uint64(77)
        st = L.kmer_table_screen(ctx, buf, n, 1, flags, out, cap, ctypes.byref(nr) if want_n else None)
        if want_n:
            assert nr.value == 0
        return st

    assert device(None, ctypes.c_void_p(0x100), 16, 0) == BAD_PARAM
    assert device(fake, None, 16, 0) == BAD_PARAM                       # NULL bytes with len > 0
    assert device(fake, ctypes.c_void_p(0x100), 16, 0, want_rows=False) == BAD_PARAM
    assert device(fake, ctypes.c_void_p(0x100), 16, 0, want_n=False) == BAD_PARAM
    assert host(None, data, len(data), 0) == BAD_PARAM
    assert host(fake, None, 16, 0) == BAD_PARAM
    assert host(fake, data, len(data), 0, want_n=False) == BAD_PARAM
    assert host(fake, data, len(data), 0, out=None) == BAD_PARAM       # room for 4 rows, nowhere to put them
    both = _native.SCREEN_DIRECT | _native.SCREEN_SORTED
    for flags in (both, both | _native.SCREEN_PIECE_TEST, 8, 1 << 16, 1 << 31, 0xFFFFFFFF):
        assert device(fake, ctypes.c_void_p(0x100), 16, flags) == BAD_PARAM, flags
        assert host(fake, data, len(data), flags) == BAD_PARAM, flags
    assert all(r.windows == r.hits == r.skipped == r.sum == 0 for r in rows)
    # len == 0: KMER_OK, zero reads, nothing touched (not even the context)
    assert device(fake, None, 0, 0) == 0
    assert host(fake, None, 0, 0) == 0
