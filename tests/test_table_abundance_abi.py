"""CPU-side checks of the table's by-value calls (kmer_table_spectrum,
kmer_table_extract_device, kmer_table_extract): exported, listed and bound,
and their parameter checks answer before any device call (no GPU needed)."""
import ctypes
import os
import re

from tests.conftest import REPO

NAMES = ["kmer_table_spectrum", "kmer_table_extract_device", "kmer_table_extract"]
BAD_PARAM = 2


def test_symbols_are_exported_listed_and_bound():
    from kmerjs_amd import _native
    lib = ctypes.CDLL(os.path.join(REPO, "kmerjs_amd", "libkmerhip.so"))
    with open(os.path.join(REPO, "include", "kmer_api.h")) as f:
        header = f.read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _native.EXPORTS, name
        assert re.search(r"kmer_status %s\(" % name, header), name
        f = getattr(_native.LIB, name)
        assert f.restype is ctypes.c_int and f.argtypes and f.argtypes[0] is ctypes.c_void_p, name
    assert len(_native.LIB.kmer_table_spectrum.argtypes) == 4
    assert len(_native.LIB.kmer_table_extract_device.argtypes) == 6
    assert len(_native.LIB.kmer_table_extract.argtypes) == 4
    for method in ("table_spectrum", "table_extract_device", "table_extract"):
        assert callable(getattr(_native.Counter, method))


def test_python_names_the_kernels_tiers_as_the_header_does():
    from kmerjs_amd import _native
    with open(os.path.join(REPO, "include", "kmer_api.h")) as f:
        header = f.read()
    reg = int(re.search(r"#define KMER_SPECTRUM_REG_MAX (\d+)u", header).group(1))
    lds = int(re.search(r"#define KMER_SPECTRUM_LDS_BINS (\d+)u", header).group(1))
    top = re.search(r"#define KMER_SPECTRUM_MAX_BINS \(1u << (\d+)\)", header)
    assert (_native.SPECTRUM_REG_MAX, _native.SPECTRUM_LDS_BINS) == (reg, lds)
    assert _native.SPECTRUM_MAX_BINS == 1 << int(top.group(1)) == 1 << 21
    assert 2 <= reg < lds < _native.SPECTRUM_MAX_BINS


def test_null_arguments_and_bad_bin_counts_without_gpu():
    from kmerjs_amd import _native
    L = _native.LIB
    hist = (ctypes.c_uint64 * 4)()
    top = ctypes.c_uint64()
    keys, counts, n, res = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_void_p()
    fake = ctypes.c_void_p(0x1000)            # never dereferenced: every call below is refused on its parameters
    # no context
    assert L.kmer_table_spectrum(None, 4, hist, ctypes.byref(top)) == BAD_PARAM
    assert L.kmer_table_extract_device(None, 1, 0, ctypes.byref(keys), ctypes.byref(counts), ctypes.byref(n)) == BAD_PARAM
    assert L.kmer_table_extract(None, 1, 0, ctypes.byref(res)) == BAD_PARAM
    # NULL out-pointers
    assert L.kmer_table_spectrum(fake, 4, None, ctypes.byref(top)) == BAD_PARAM
    assert L.kmer_table_extract_device(fake, 1, 0, None, ctypes.byref(counts), ctypes.byref(n)) == BAD_PARAM
    assert L.kmer_table_extract_device(fake, 1, 0, ctypes.byref(keys), None, ctypes.byref(n)) == BAD_PARAM
    assert L.kmer_table_extract_device(fake, 1, 0, ctypes.byref(keys), ctypes.byref(counts), None) == BAD_PARAM
    assert L.kmer_table_extract(fake, 1, 0, None) == BAD_PARAM
    # nbins outside [2, 2^21]
    for nbins in (0, 1, (1 << 21) + 1):
        assert L.kmer_table_spectrum(fake, nbins, hist, ctypes.byref(top)) == BAD_PARAM, nbins
        assert L.kmer_table_spectrum(fake, nbins, hist, None) == BAD_PARAM, nbins
    assert list(hist) == [0, 0, 0, 0] and top.value == 0 and n.value == 0
