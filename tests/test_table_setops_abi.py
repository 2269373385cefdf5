"""CPU-side checks of the calls that relate two tables (kmer_table_compare,
kmer_table_setop_device, kmer_table_setop): exported, listed, prototyped and
bound, Python's constants equal the header's, and the parameter checks answer
before any device call (no GPU needed)."""
import ctypes
import os
import re

from tests.conftest import REPO

NAMES = ["kmer_table_compare", "kmer_table_setop_device", "kmer_table_setop"]
BAD_PARAM = 2


def _header():
    with open(os.path.join(REPO, "include", "kmer_api.h")) as f:
        return f.read()


def test_symbols_are_exported_listed_and_bound():
    from kmerjs_amd import _native
    lib = ctypes.CDLL(os.path.join(REPO, "kmerjs_amd", "libkmerhip.so"))
    header = _header()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _native.EXPORTS, name
        assert re.search(r"kmer_status %s\(" % name, header), name
        f = getattr(_native.LIB, name)
        assert f.restype is ctypes.c_int and f.argtypes and f.argtypes[0] is ctypes.c_void_p, name
        assert f.argtypes[1] is ctypes.c_void_p, name
    assert len(_native.LIB.kmer_table_compare.argtypes) == 5
    assert len(_native.LIB.kmer_table_setop_device.argtypes) == 8
    assert len(_native.LIB.kmer_table_setop.argtypes) == 6
    for method in ("table_compare", "table_setop_device", "table_setop"):
        assert callable(getattr(_native.Counter, method))
    fields = [name for name, _ in _native.TableOverlap._fields_]
    assert fields == ["keys_a", "keys_b", "keys_both", "total_a", "total_b", "shared_a", "shared_b", "sum_min"]
    assert ctypes.sizeof(_native.TableOverlap) == 64
    body = re.search(r"typedef struct \{([^}]*)\} kmer_table_overlap;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    assert re.findall(r"(\w+)\s*[,;]", body) == fields     # the header's members, in its order


def test_python_names_the_tile_and_the_operations_as_the_header_does():
    from kmerjs_amd import _native
    header = _header()
    assert _native.JOIN_TILE == int(re.search(r"#define KMER_JOIN_TILE (\d+)u", header).group(1))
    ops = {m.group(1): int(m.group(2)) for m in re.finditer(r"KMER_SETOP_(\w+) = (\d+)", header)}
    assert ops == {"INTERSECT": 0, "SUBTRACT": 1, "UNION": 2}
    assert (_native.SETOP_INTERSECT, _native.SETOP_SUBTRACT, _native.SETOP_UNION) == (0, 1, 2)
    assert _native.JOIN_TILE >= 64 and _native.JOIN_TILE & (_native.JOIN_TILE - 1) == 0


def test_null_arguments_and_bad_operations_without_gpu():
    from kmerjs_amd import _native
    L = _native.LIB
    o = _native.TableOverlap()
    keys, counts, n, res = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_void_p()
    fake = ctypes.c_void_p(0x1000)            # never dereferenced: every call below is refused on its parameters
    out3 = (ctypes.byref(keys), ctypes.byref(counts), ctypes.byref(n))
    # no context, on either side
    for a, b in ((None, fake), (fake, None), (None, None)):
        assert L.kmer_table_compare(a, b, 1, 1, ctypes.byref(o)) == BAD_PARAM
        assert L.kmer_table_setop_device(a, b, 0, 1, 1, *out3) == BAD_PARAM
        assert L.kmer_table_setop(a, b, 0, 1, 1, ctypes.byref(res)) == BAD_PARAM
    # NULL out-pointers
    assert L.kmer_table_compare(fake, fake, 1, 1, None) == BAD_PARAM
    assert L.kmer_table_setop_device(fake, fake, 0, 1, 1, None, ctypes.byref(counts), ctypes.byref(n)) == BAD_PARAM
    assert L.kmer_table_setop_device(fake, fake, 0, 1, 1, ctypes.byref(keys), None, ctypes.byref(n)) == BAD_PARAM
    assert L.kmer_table_setop_device(fake, fake, 0, 1, 1, ctypes.byref(keys), ctypes.byref(counts), None) == BAD_PARAM
    assert L.kmer_table_setop(fake, fake, 0, 1, 1, None) == BAD_PARAM
    # op = 3 (and beyond)
    for op in (3, 4, 0xFFFFFFFF):
        assert L.kmer_table_setop_device(fake, fake, op, 1, 1, *out3) == BAD_PARAM, op
        assert L.kmer_table_setop(fake, fake, op, 1, 1, ctypes.byref(res)) == BAD_PARAM, op
    assert n.value == 0 and not keys.value and not counts.value and not res.value
    assert all(getattr(o, name) == 0 for name, _ in _native.TableOverlap._fields_)
