"""CPU-side checks of the set operation whose result stays a table
(kmer_table_setop_into): exported, listed, prototyped and bound, and the
parameter checks that need no context answer before any device call (no GPU
needed).  The handles below are fake: a call that dereferenced one would not
return."""
import ctypes
import os
import re

from tests.conftest import REPO

NAME = "kmer_table_setop_into"
BAD_PARAM = 2


def test_symbol_is_exported_listed_prototyped_and_bound():
    from kmerjs_amd import _native
    lib = ctypes.CDLL(os.path.join(REPO, "kmerjs_amd", "libkmerhip.so"))
    with open(os.path.join(REPO, "include", "kmer_api.h")) as f:
        header = f.read()
    assert hasattr(lib, NAME)
    assert NAME in _native.EXPORTS
    proto = re.search(r"kmer_status %s\(([^)]*)\)" % NAME, header)
    assert proto and len(proto.group(1).split(",")) == 6
    f = getattr(_native.LIB, NAME)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    assert f.restype is ctypes.c_int
    assert list(f.argtypes) == [vp, vp, ctypes.c_uint32, u64, u64, vp]
    assert callable(_native.Counter.table_setop_into)


def test_null_contexts_bad_operations_and_in_place_calls_without_gpu():
    from kmerjs_amd import _native
    call = _native.LIB.kmer_table_setop_into
    a, b, d = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)   # never dereferenced
    for x, y, z in ((None, b, d), (a, None, d), (a, b, None), (None, None, None)):
        for op in (0, 1, 2):
            assert call(x, y, op, 1, 1, z) == BAD_PARAM, (x, y, z, op)
    for op in (3, 4, 0xFFFFFFFF):
        assert call(a, b, op, 1, 1, d) == BAD_PARAM, op
        assert call(a, a, op, 1, 1, d) == BAD_PARAM, op
    for op in (0, 1, 2):                                      # no in-place operation
        assert call(a, b, op, 1, 1, a) == BAD_PARAM, op
        assert call(a, b, op, 1, 1, b) == BAD_PARAM, op
        assert call(a, a, op, 1, 1, a) == BAD_PARAM, op
