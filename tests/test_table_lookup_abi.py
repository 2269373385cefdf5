"""The table lookup's entry points exist in the shipped library and refuse a
NULL context (no GPU needed: neither call reaches the device)."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "..", "kmerjs_amd", "libkmerhip.so")


def test_library_exports_the_lookup_calls():
    lib = ctypes.CDLL(LIB)
    for name in ("kmer_table_lookup", "kmer_table_lookup_device"):
        assert hasattr(lib, name), name


def test_lookup_refuses_a_null_context():
    lib = ctypes.CDLL(LIB)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.kmer_table_lookup.restype = ctypes.c_int
    lib.kmer_table_lookup.argtypes = [vp, ctypes.c_char_p, u64, ctypes.POINTER(u64)]
    lib.kmer_table_lookup_device.restype = ctypes.c_int
    lib.kmer_table_lookup_device.argtypes = [vp, vp, u64, vp, vp]
    out = (u64 * 1)()
    assert lib.kmer_table_lookup(None, b"A" * 16, 1, out) == 2
    assert lib.kmer_table_lookup(None, None, 0, None) == 2
    assert lib.kmer_table_lookup_device(None, None, 1, None, None) == 2
