"""The FASTA route to a template DB (kmer_db_open_fasta / _device and the
per-template readouts) is exported, listed, prototyped in include/kmer_match.h
and bound in Python; KMER_DB_PIECE_TEST equals Python's constant; and the
parameter checks that need no context answer KMER_E_BAD_PARAM before anything
is dereferenced, with *out left NULL (no GPU needed: a fake context pointer is
never read).  k > 32, step != 1 and the state checks need a real context, and
len == 0 returns a real DB: both are in tests/test_db_fasta_gpu.py."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "kmer_match.h")
NAMES = {"kmer_db_open_fasta_device": 6, "kmer_db_open_fasta": 5, "kmer_db_template_stats": 5,
         "kmer_db_template_kmers": 5, "kmer_db_template_name": 4}
BAD_PARAM = 2


def _header():
    with open(HEADER) as f:
        return f.read()


def test_symbols_are_exported_listed_prototyped_and_bound():
    from kmerjs_amd import _native, kmerfinder
    for name, nargs in NAMES.items():
        assert name in _native.MATCH_EXPORTS and name in _native.EXPORTS
        f = getattr(_native.LIB, name)
        assert f.restype is ctypes.c_int and f.argtypes is not None and len(f.argtypes) == nargs
        assert re.search(r"kmer_status\s+%s\s*\(" % name, _header())
    for meth in ("from_fasta", "from_fasta_device", "template_kmers", "template_stats", "template_name"):
        assert callable(getattr(kmerfinder.TemplateDB, meth))


def test_piece_test_flag_equals_the_headers():
    from kmerjs_amd import _native
    m = re.search(r"KMER_DB_PIECE_TEST\s*=\s*(\d+)u?", _header())
    assert m and int(m.group(1)) == _native.DB_PIECE_TEST == 1


def test_null_and_bad_flag_calls_are_refused_before_the_context_is_read():
    from kmerjs_amd import _native
    L = _native.LIB
    fake = ctypes.c_void_p(0x10)                 # never dereferenced: every call below fails its parameter check
    data = ctypes.create_string_buffer(b">a\nACGTACGTACGT\n")
    n = len(data.raw) - 1

    def device(ctx, ptr, nbytes, flags, want_out=True):
        out = ctypes.c_void_p(0x1234)
        st = L.kmer_db_open_fasta_device(ctx, ptr, nbytes, flags, None, ctypes.byref(out) if want_out else None)
        if want_out:
            assert out.value is None
        return st

    def host(ctx, buf, nbytes, flags, want_out=True):
        out = ctypes.c_void_p(0x1234)
        st = L.kmer_db_open_fasta(ctx, buf, nbytes, flags, ctypes.byref(out) if want_out else None)
        if want_out:
            assert out.value is None
        return st

    assert device(None, ctypes.c_void_p(0x100), 16, 0) == BAD_PARAM
    assert device(fake, None, 16, 0) == BAD_PARAM                       # NULL bytes with len > 0
    assert device(fake, ctypes.c_void_p(0x100), 16, 0, want_out=False) == BAD_PARAM
    assert host(None, data, n, 0) == BAD_PARAM
    assert host(fake, None, 16, 0) == BAD_PARAM
    assert host(fake, data, n, 0, want_out=False) == BAD_PARAM
    for flags in (2, 3, 4, 1 << 16, 1 << 31, 0xFFFFFFFF):
        assert device(fake, ctypes.c_void_p(0x100), 16, flags) == BAD_PARAM, flags
        assert host(fake, data, n, flags) == BAD_PARAM, flags
    assert b"kmer_db_open_fasta" in L.kmer_match_last_error()


def test_readouts_refuse_a_null_db():
    from kmerjs_amd import _native
    L = _native.LIB
    a = (ctypes.c_uint64 * 1)()
    n = ctypes.c_uint64(7)
    p, ln = ctypes.c_void_p(), ctypes.c_uint32()
    assert L.kmer_db_template_stats(None, 0, 0, a, a) == BAD_PARAM
    assert L.kmer_db_template_kmers(None, 0, 0, None, ctypes.byref(n)) == BAD_PARAM
    assert L.kmer_db_template_name(None, 0, ctypes.byref(p), ctypes.byref(ln)) == BAD_PARAM
